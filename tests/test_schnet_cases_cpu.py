"""CPU: every case of tests/schnet_cases.py still has the property it exists for (a case that drifts fails here instead of passing silently on
the GPU), and the restatement's four sweeps reproduce the autograd restatement in float64 on the cases with long rows and small n_rbf."""
import math

import pytest
import torch

from oracle import spk_schnet_ref as S
from tests import schnet_cases as SC
from tests.helpers import rel_err


def _cfg(name):
    c = SC.get_case(name).cfg
    return c.n_atom_basis, c.n_interactions, c.n_rbf, c.cutoff


def test_case_list():
    assert SC.CASE_NAMES == ["long_rows-F64", "long_rows-F128", "long_rows-F256", "small_r-R2", "small_r-R12", "small_r-R13", "small_r-R14", "lds_limit",
                             "sort_limit", "one_pair", "elements", "near_cutoff"]
    for name in SC.CASE_NAMES:
        c = SC.get_case(name)
        assert c.pos.dtype == torch.float32 and c.pos.shape == c.ft.shape and c.z.shape == c.batch.shape == (c.pos.shape[0],)
        assert int(c.z.min()) >= 1 and int(c.z.max()) < c.cfg.max_z
        assert torch.equal(c.batch, torch.sort(c.batch).values) and c.y.shape == (int(c.batch.max()) + 1,)


@pytest.mark.parametrize("name", SC.LONG_ROWS)
def test_long_rows_have_rows_and_lower_lists_beyond_one_wavefront(name):
    c = SC.get_case(name)
    assert _cfg(name) == {"long_rows-F64": (64, 2, 20, 6.0), "long_rows-F128": (128, 1, 20, 6.0), "long_rows-F256": (256, 1, 20, 6.0)}[name]
    assert c.sizes == [200, 2, 70]
    deg, low = SC.row_stats(c)
    assert int(deg.max()) > 64 and int(low.max()) > 64, (int(deg.max()), int(low.max()))     # the second chunk of k_sn_conv and of k_sn_pair_rev
    assert int(deg.max()) <= 128                                                            # ... and no third: the two buckets below are all there is
    assert int(((deg >= 1) & (deg <= 64)).sum()) > 0 and int(((deg >= 65) & (deg <= 128)).sum()) > 0
    assert int(((low >= 1) & (low <= 64)).sum()) > 0 and int((low >= 65).sum()) > 0
    assert set(c.z.tolist()) <= {1, 6, 7, 8, 19}
    assert torch.equal(c.pos, SC.get_case("long_rows-F64").pos)                              # one geometry for the three widths


def test_long_rows_keep_activations_of_order_one():
    """Default initialisation, no rescaled weights: |m| stays O(1) at degree ~100 (the issue measured 2.5), energies ~1 per atom."""
    ref = SC.reference("long_rows-F64")
    for l in range(2):
        assert float(ref.sw.S["m", l].abs().max()) < 10.0
    assert float(ref.energy.abs().max()) < 10.0 * 200


@pytest.mark.parametrize("name", SC.SMALL_R_CASES)
def test_small_r_sits_on_both_sides_of_the_window(name):
    c = SC.get_case(name)
    F, L, R, cutoff = _cfg(name)
    assert (F, L, cutoff) == (64, 2, 4.0) and c.sizes == [12, 1, 2, 30]
    assert sorted(SC.get_case(n).cfg.n_rbf for n in SC.SMALL_R_CASES) == [2, 12, 13, 14] and SC.FWIN == 13
    ii, _ = SC.neighbor_list(c)
    assert 12 not in ii.tolist()                                                             # the single atom (index 12) has no pair
    deg, _ = SC.row_stats(c)
    assert int(deg[13]) == 1 and int(deg[14]) == 1                                           # the dimer has its one pair


def test_lds_limit_fills_lds_exactly():
    c = SC.get_case("lds_limit")
    F, L, R, cutoff = _cfg("lds_limit")
    assert (F, L, R, cutoff) == (256, 1, 156, 5.0) and c.sizes == [140, 1, 2, 9]
    assert R * F * 4 == SC.LDS_BYTES and (R + 1) * F * 4 > SC.LDS_BYTES
    assert R - min(R, SC.FWIN) + 1 <= SC.SORT_BINS


def test_sort_limit_fills_the_bins_exactly():
    c = SC.get_case("sort_limit")
    F, L, R, cutoff = _cfg("sort_limit")
    assert (F, L, R, cutoff) == (64, 1, 268, 5.0) and c.sizes == [40, 1, 2, 9]
    assert R - SC.FWIN + 1 == SC.SORT_BINS and R * F * 4 <= SC.LDS_BYTES


def test_one_pair():
    c = SC.get_case("one_pair")
    assert _cfg("one_pair") == (64, 2, 20, 4.0)
    ii, jj = SC.neighbor_list(c)
    assert c.pos.shape[0] == 2 and int(c.batch.max()) == 0 and ii.tolist() == [0, 1] and jj.tolist() == [1, 0]      # N = 2, E = 2, P = 1


def test_elements_has_the_last_row_and_absent_rows():
    c = SC.get_case("elements")
    assert _cfg("elements") == (64, 1, 20, 4.0) and c.cfg.max_z == 20 and 25 <= c.pos.shape[0] <= 35
    present = set(c.z.tolist())
    assert c.cfg.max_z - 1 in present and len(set(range(1, 19)) - present) >= 3
    G = SC.reference("elements").G["representation.embedding.weight"]
    for zz in range(c.cfg.max_z):
        assert (zz in present) == bool(G[zz].abs().max() > 0), zz                           # a gradient row is zero exactly where the element is absent


def test_near_cutoff_pair_is_listed_and_cut_to_nothing():
    c = SC.get_case("near_cutoff")
    assert _cfg("near_cutoff") == (64, 1, 20, 4.0) and c.sizes == [9, 2, 5]
    ref = SC.reference("near_cutoff")
    assert (9, 10) in ref.key and (10, 9) in ref.key
    e = ref.key[(10, 9)]
    d = float(ref.sw.d[e])
    assert d == 4.0 * (1.0 - 2.0 ** -20) and d < 4.0
    assert d * d < 16.0 and float(torch.tensor(d, dtype=torch.float32) ** 2) < 16.0          # inside the cutoff in float32 too (the engine compares d^2)
    assert 0.0 < float(ref.sw.rc[e]) < 1e-10
    assert math.isclose(float(ref.sw.rc[e]), 0.25 * (math.pi * 2.0 ** -20) ** 2, rel_tol=1e-4)
    assert int((ref.sw.rc > 1e-3).sum()) >= 20                                               # ... beside ordinary pairs


@pytest.mark.parametrize("name", SC.LONG_ROWS + SC.SMALL_R_CASES)
def test_sweeps_match_autograd_fp64(name):
    """To the bounds of test_schnet_cpu.py:test_schnet_sweeps_match_autograd_fp64."""
    c = SC.get_case(name)
    ref = SC.reference(name)
    e_ref, f_ref, loss_ref, g_ref = S.schnet_train_step(ref.P, c.cfg, c.pos.double(), c.z, c.batch, c.y.double(), c.ft.double())
    assert rel_err(ref.energy.numpy(), e_ref.numpy()) < 1e-12
    assert rel_err(ref.forces.numpy(), f_ref.numpy()) < 1e-11
    assert abs(float(ref.loss) - float(loss_ref)) < 1e-12 * abs(float(loss_ref))
    for k in g_ref:
        assert rel_err(ref.G[k].numpy(), g_ref[k].numpy()) < 1e-9, k


def test_stored_locals_of_the_dual_reverse_sweep():
    """The locals SchNetSweeps.dual_reverse keeps for the operator tests are the ones it computed with: gy of layer 0 reproduces the in2f gradient, the
    final gx the embedding gradient, and the per-layer gd shares add up to the total."""
    ref = SC.reference("small_r-R14")
    sw, St = ref.sw, ref.sw.S
    G = St["r_gy", 0].T @ St["x", 0] + St["r_gty", 0].T @ St["tx", 0]
    assert rel_err(G.numpy(), ref.G["representation.interactions.0.in2f.weight"].numpy()) < 1e-13
    emb = torch.zeros_like(ref.P["representation.embedding.weight"]).index_add_(0, sw.z, St["r_gx"])
    assert torch.equal(emb, ref.G["representation.embedding.weight"])
    assert rel_err((St["gd", 0] + St["gd", 1]).numpy(), St["gd"].numpy()) < 1e-13
    for k in ("r_gm", "r_gtm", "r_gt1", "r_gtt1", "r_gh2", "r_gth2", "r_gz1", "r_gtz1td"):
        assert (k, 0) in St and (k, 1) in St
