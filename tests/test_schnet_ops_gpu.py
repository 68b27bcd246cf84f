"""GPU: operator-level tests of the SchNet engine (csrc/schnet.hip) at its edge cases (tests/schnet_cases.py): every workspace buffer of the four
sweeps, read through nq_schnet_ws_lookup, against the float64 restatement oracle/spk_schnet_ref.py:SchNetSweeps, which keeps the same buffers under
the same names.  PARITY UNPINNED like tests/test_schnet_gpu.py: this pins the HIP path to the restatement only.

Tolerances (float32 engine, float64 reference; from the reference, not from the code under test): for each case and buffer the restatement also runs in
float32 on the CPU; the bound is max(8 x its error against float64, 1e-5), both measured with tests.helpers.rel_err.  1e-5 is what test_engine_gpu.py
grants the forward buffers of the PaiNN engine; the factor 8 covers another summation order, expf / cosf against libm and the dropped window taps
(< 1e-9).  Energy, forces and parameter gradients keep the bounds of test_schnet_gpu.py (2e-6, 2e-5, 2e-4 with that file's scale) except on
lds_limit and sort_limit, whose narrow Gaussians put the float32 restatement itself at 1e-5: there the rule above applies to them too.
Every figure is printed; the worst buffer per case and class goes to the suite's parity report (tests.helpers._report), from which
profiles/schnet_ops_parity.txt was taken.

Pair p of the engine has slot pair_slot[p] and atoms (dst[slot], col[slot]) = (i, j), j < i; the restatement's directed edge is looked up by its
(i, j) key, the two lists are not assumed to share an order.  Per-pair adjoints of the engine are the sum over the two directed edges."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import spk_schnet_ref as S
from tests import schnet_cases as SC
from tests.helpers import _report, rel_err
from tests.schnet_driver import Engine

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 1e-5, 8.0
E_TOL, F_TOL, G_TOL = 2e-6, 2e-5, 2e-4                       # tests/test_schnet_gpu.py
RULE_END_TO_END = ("lds_limit", "sort_limit")                  # end-to-end quantities under the float32-restatement rule

_ENGINES, _TABLE = {}, {}


def stepped(name) -> Engine:
    """The engine after one training step (forward with forces, backward with the MSE seeds) on a case; run once per case and shared.  The backward
    call leaves the primal halves, the window records, the pair tables and gd_total of the forward call as they were."""
    if name not in _ENGINES:
        eng = Engine(SC.get_case(name))
        eng.train_step()
        _ENGINES[name] = eng
    return _ENGINES[name]


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    yield
    _ENGINES.clear()
    _report("schnet_ops: worst buffer per case and buffer class; err = max|engine - ref64| / max|ref64|, own = the float32 restatement's err,")
    _report("schnet_ops: bound = max(8 own, 1e-5) or the fixed end-to-end bound of tests/test_schnet_gpu.py")
    _report(f"schnet_ops: {'case':16s} {'class':10s} {'worst buffer':44s} {'err':>10s} {'own':>10s} {'bound':>10s}")
    for (case, cls), (ratio, label, err, own, bound) in _TABLE.items():
        _report(f"schnet_ops: {case:16s} {cls:10s} {label:44s} {err:10.2e} {own:10.2e} {bound:10.2e}{'' if err <= bound else '  ABOVE'}")


def _note(case, cls, label, err, own, bound):
    print(f"{case:16s} {cls:10s} {label:44s} err {err:.2e} own {own:.2e} bound {bound:.2e}{'' if err <= bound else '  ABOVE'}")
    ratio = err / bound
    if (case, cls) not in _TABLE or ratio > _TABLE[case, cls][0]:
        _TABLE[case, cls] = (ratio, label, err, own, bound)
    return err <= bound


def _compare(case, cls, got, exp64, exp32, fixed=None):
    """got / exp64 / exp32: {label: tensor}.  Every buffer is measured and printed before anything is asserted."""
    bad = []
    for label, r64 in exp64.items():
        g = got[label].double().reshape(r64.shape)
        assert not torch.isnan(g).any(), (case, label, "never written")
        err, own = rel_err(g.numpy(), r64.numpy()), rel_err(exp32[label].double().numpy(), r64.numpy())
        bound = fixed if fixed is not None else max(FACTOR * own, FLOOR)
        if not _note(case, cls, label, err, own, bound):
            bad.append((label, err, own, bound))
    assert not bad, (case, cls, bad)


# ---- the restatement in the engine's layout ---------------------------------------------------------------------------------------------------------
def _edge_maps(eng, ref):
    """slot -> directed edge of the restatement; pair -> its two directed edges (i <- j, j < i) and (j <- i)."""
    dst, col = eng.graph("dst").tolist(), eng.graph("col").tolist()
    assert eng.E == len(ref.key) and set(zip(dst, col)) == set(ref.key), "the engine's neighbour list is not the restatement's"
    slot_e = torch.tensor([ref.key[i, j] for i, j in zip(dst, col)], dtype=torch.long)
    pair_slot = eng.buf("pair_slot").long()
    return slot_e, slot_e[pair_slot], slot_e[eng.graph("rev").long()[pair_slot]]


def _eps(ref, r1, tr1=None):
    w, b = ref.P["output_modules.0.outnet.1.weight"], ref.P["output_modules.0.outnet.1.bias"]
    if tr1 is None:
        return (S.silu(r1) @ w.T + b).squeeze(1)
    return ((S.dsilu(r1) * tr1) @ w.T).squeeze(1)


def _expected(ref, slot_e, e1, e2):
    """{class: {label: tensor}} with label = 'name[layer]' / 't:name[layer]' for the tangent half."""
    St, L = ref.sw.S, ref.sw.cfg.n_interactions
    fwd, tan, adj = {}, {}, {}
    for l in range(L + 1):
        fwd[f"x[{l}]"], tan[f"t:x[{l}]"] = St["x", l], St["tx", l]
    for l in range(L):
        fwd[f"a1[{l}]"], fwd[f"h2[{l}]"] = St["a1", l][e1], St["h2", l][e1]
        tan[f"t:a1[{l}]"], tan[f"t:h2[{l}]"] = St["ta1", l][e1], St["th2", l][e1]
        for n, t in (("y", "ty"), ("m", "tm"), ("t1", "tt1"), ("u", "tu")):
            fwd[f"{n}[{l}]"], tan[f"t:{n}[{l}]"] = St[n, l], St[t, l]
    fwd["zo[0]"], tan["t:zo[0]"] = St["r1"], St["tr1"]
    fwd["e_atom[0]"], tan["te_atom[0]"] = _eps(ref, St["r1"]), _eps(ref, St["r1"], St["tr1"])
    fwd["gd_total[0]"] = St["gd"][e1] + St["gd"][e2]
    tan["tdp[0]"], tan["td[0]"] = St["td"][e1], St["td"][slot_e]
    adj["gx[0]"], adj["t:gx[0]"] = St["r_gx"], St["r_gtx"]
    adj["gu[0]"], adj["t:gu[0]"] = St["r_gt1", 0], St["r_gtt1", 0]
    adj["gm[0]"], adj["t:gm[0]"] = St["r_gm", 0], St["r_gtm", 0]
    adj["gy[0]"], adj["t:gy[0]"] = St["r_gy", 0], St["r_gty", 0]
    adj["gh2[0]"], adj["t:gh2[0]"] = St["r_gh2", 0][e1] + St["r_gh2", 0][e2], St["r_gth2", 0][e1] + St["r_gth2", 0][e2]
    adj["ga1[0]"], adj["t:ga1[0]"] = St["r_gz1", 0][e1] + St["r_gz1", 0][e2], St["r_gtz1td", 0][e1] + St["r_gtz1td", 0][e2]
    return {"forward": fwd, "tangent": tan, "adjoint": adj}


def _engine_buffers(eng, labels):
    out = {}
    for label in labels:
        tangent = label.startswith("t:")
        name, layer = label[2 if tangent else 0:-1].split("[")
        out[label] = eng.buf(name, int(layer), int(tangent))
    return out


def _buffer_class(name, cls):
    eng = stepped(name)
    ref64, ref32 = SC.reference(name), SC.reference(name, torch.float32)
    maps = _edge_maps(eng, ref64)
    exp64, exp32 = _expected(ref64, *maps)[cls], _expected(ref32, *maps)[cls]
    _compare(name, cls, _engine_buffers(eng, exp64), exp64, exp32)


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_pairs(name):
    """k_sn_pairs rests on 'the lower neighbours are the first entries of a row'."""
    eng = stepped(name)
    E, Pn = eng.E, eng.E // 2
    row_ptr, lowptr = eng.graph("row_ptr").long(), eng.graph("lowptr").long()
    dst, col, rev = eng.graph("dst").long(), eng.graph("col").long(), eng.graph("rev").long()
    pair_of, pair_slot = eng.buf("pair_of").long(), eng.buf("pair_slot").long()
    assert E == 2 * Pn and int(lowptr[-1]) == Pn and int(row_ptr[-1]) == E
    pos_in_row = torch.arange(E) - row_ptr[dst]
    lower = col < dst
    assert torch.equal(lower, pos_in_row < (lowptr[dst + 1] - lowptr[dst]))                      # the lower neighbours come first in every row
    assert torch.equal(torch.sort(pair_of).values, torch.arange(Pn).repeat_interleave(2))       # 2P slots onto 0..P-1, two slots each ...
    assert torch.equal(pair_of[rev], pair_of) and torch.equal(rev[rev], torch.arange(E))        # ... namely a slot and its reverse
    assert bool(lower[pair_slot].all()) and torch.equal(pair_of[pair_slot], torch.arange(Pn))   # pair_slot: the one of the two with col < dst
    assert torch.equal(pair_of[lower], (lowptr[dst] + pos_in_row)[lower])                        # numbered lowptr[i] + position in row i
    geom, geomp = eng.graph("geom").view(torch.int32), eng.buf("geomp").view(Pn, 4).view(torch.int32)
    assert torch.equal(geomp, geom[pair_slot])                                                  # bitwise the geometry of that slot
    # the k0-sorted pair order of the first-layer weight gradient: a permutation, stable
    order, k0 = eng.buf("order").long(), eng.buf("rw").view(Pn, 32)[:, 13].contiguous().view(torch.int32).long()
    assert torch.equal(torch.sort(order).values, torch.arange(Pn))
    key = k0[order] * Pn + order
    assert bool((key[1:] > key[:-1]).all())


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_window_record(name):
    """k_rbf_window in mode 2 (bare Gaussians, fcut in slot 14, fcut' in slot 30) against gauss_and_cutoff in float64."""
    eng = stepped(name)
    ref64, ref32 = SC.reference(name), SC.reference(name, torch.float32)
    _, e1, _ = _edge_maps(eng, ref64)
    R, Pn = eng.case.cfg.n_rbf, eng.E // 2
    nwin = min(R, SC.FWIN)
    rw = eng.buf("rw").view(Pn, 32)
    k0 = rw[:, 13].contiguous().view(torch.int32).long()
    assert int(k0.min()) >= 0 and int(k0.max()) <= R - nwin, (int(k0.min()), int(k0.max()))
    idx = k0[:, None] + torch.arange(SC.FWIN)[None, :]
    valid = idx < R
    assert bool((valid.sum(1) == nwin).all())
    taps, dtaps = rw[:, 0:13], rw[:, 16:29]
    assert bool((taps[~valid] == 0.0).all()) and bool((dtaps[~valid] == 0.0).all())             # taps at or beyond R are exactly zero
    assert bool((rw[:, [15, 29, 31]] == 0.0).all())

    def window(ref):
        sw, zero = ref.sw, torch.zeros((), dtype=ref.sw.g.dtype)
        gi = idx.clamp(max=R - 1)
        return {"g": torch.where(valid, sw.g[e1].gather(1, gi), zero), "dg": torch.where(valid, sw.dg[e1].gather(1, gi), zero),
                "fcut": sw.rc[e1], "dfcut": sw.drc[e1]}
    _compare(name, "window", {"g": taps, "dg": dtaps, "fcut": rw[:, 14], "dfcut": rw[:, 30]}, window(ref64), window(ref32))
    outside = torch.ones(Pn, R, dtype=torch.bool)
    outside.scatter_(1, idx.clamp(max=R - 1), False)
    dropped = float(ref64.sw.g[e1][outside].max()) if bool(outside.any()) else 0.0
    print(f"{name}: largest Gaussian outside the window {dropped:.2e}")
    assert dropped < 1e-9              # the nearest dropped centre is >= 6.5 widths away: exp(-6.5^2 / 2) = 6.7e-10


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_forward_buffers(name):
    _buffer_class(name, "forward")


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_tangent_buffers(name):
    _buffer_class(name, "tangent")


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_adjoint_buffers_of_layer_0(name):
    """After nq_schnet_backward the shared adjoint buffers hold the layer processed last: the L = 1 cases pin every reverse kernel, the L = 2 cases the
    layer that runs last."""
    _buffer_class(name, "adjoint")


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_energy_forces_and_parameter_gradients(name):
    eng = stepped(name)
    ref64, ref32 = SC.reference(name), SC.reference(name, torch.float32)
    rule = name in RULE_END_TO_END
    _compare(name, "energy", {"energy": eng.energy.cpu()}, {"energy": ref64.energy}, {"energy": ref32.energy}, None if rule else E_TOL)
    _compare(name, "forces", {"forces": eng.forces.cpu()}, {"forces": ref64.forces}, {"forces": ref32.forces}, None if rule else F_TOL)
    got = eng.grads()
    assert list(got) == list(ref64.G)
    if rule:
        _compare(name, "grads", got, ref64.G, ref32.G)
        return
    bad = []
    for k, g64 in ref64.G.items():
        g = g64.numpy()
        scale = max(np.abs(g).max(), np.sqrt((g ** 2).mean()) + 1e-30)                           # the scale of tests/test_schnet_gpu.py
        err = float(np.abs(got[k].double().numpy() - g).max() / scale)
        own = float(np.abs(ref32.G[k].double().numpy() - g).max() / scale)
        if not _note(name, "grads", k, err, own, G_TOL):
            bad.append((k, err))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_every_output_is_written(name):
    """Workspace and gradient buffer were NaN before the calls: everything a step hands out is finite, and the gradient rows nobody computes are 0.0."""
    eng = stepped(name)
    L = eng.case.cfg.n_interactions
    assert bool(torch.isfinite(eng.energy).all()) and bool(torch.isfinite(eng.forces).all())
    nan = torch.isnan(eng.grad)
    assert not bool(nan.any()), f"{int(nan.sum())} of {nan.numel()} gradient elements never written"
    assert bool(torch.isfinite(eng.grad).all())
    asked = [("x", l, t) for l in range(L + 1) for t in (0, 1)]
    asked += [(n, l, t) for n in ("y", "m", "t1", "u", "a1", "h2") for l in range(L) for t in (0, 1)]
    asked += [(n, 0, t) for n in ("zo", "gx", "gu", "gm", "gy", "gh2", "ga1") for t in (0, 1)]
    asked += [(n, 0, 0) for n in ("e_atom", "te_atom", "geomp", "td", "tdp", "gd_total")]
    for n, l, t in asked:
        assert bool(torch.isfinite(eng.buf(n, l, t)).all()), (n, l, t)
    emb = eng.grads()["representation.embedding.weight"]
    present = set(eng.case.z.tolist())
    for zz in range(eng.case.cfg.max_z):
        if zz not in present:                                                                    # the padding row and every absent element
            assert bool((emb[zz] == 0.0).all()), zz
    isolated = (eng.graph("row_ptr")[1:] == eng.graph("row_ptr")[:-1]).nonzero().flatten()
    assert bool((eng.forces.cpu()[isolated] == 0.0).all())                                       # an atom without a pair feels no force


def test_absent_elements_have_exactly_zero_gradient_rows():
    eng = stepped("elements")
    emb = eng.grads()["representation.embedding.weight"]
    present = set(eng.case.z.tolist())
    assert 19 in present and len(present) < 19
    assert bool((emb[0] == 0.0).all())
    for zz in range(1, 20):
        assert bool((emb[zz] == 0.0).all()) == (zz not in present), zz
    assert float(emb[19].abs().max()) > 0.0                                                      # z = max_z - 1: the last row of the table


@pytest.mark.parametrize("name", ["small_r-R14", "one_pair"])
def test_null_argument_paths(name):
    case = SC.get_case(name)
    eng = Engine(case)
    # energy-only training: forces = NULL in forward, grad_forces = NULL in backward  ==  schnet_train_step(..., w_f = 0)
    energy, forces = eng.forward(want_forces=False)
    assert forces is None
    ge, _ = eng.mse_seeds()
    eng.backward(ge, None)
    P64 = {k: v.double() for k, v in S.make_schnet_params(case.cfg, case.param_seed).items()}
    e_ref, _, _, g_ref = S.schnet_train_step(P64, case.cfg, case.pos.double(), case.z, case.batch, case.y.double(), case.ft.double(), w_f=0.0)
    e_err = rel_err(energy.cpu().numpy(), e_ref.numpy())
    print(f"{name}: energy-only energy {e_err:.2e}")
    assert e_err < E_TOL
    got, bad = eng.grads(), []
    for k, g64 in g_ref.items():
        g = g64.numpy()
        scale = max(np.abs(g).max(), np.sqrt((g ** 2).mean()) + 1e-30)
        err = float(np.abs(got[k].double().numpy() - g).max() / scale)
        print(f"{name}: energy-only grad {k} {err:.2e}")
        assert not bool(torch.isnan(got[k]).any()), k
        if not err < G_TOL:
            bad.append((k, err))
    assert not bad, bad
    # grad_energy = NULL is a zero grad_energy, bit for bit
    eng.forward(True)
    _, gf = eng.mse_seeds()
    g_null = eng.backward(None, gf).clone()
    eng.forward(True)
    g_zero = eng.backward(torch.zeros(eng.B, device=eng.dev), gf)
    assert bool(torch.isfinite(g_null).all())
    assert torch.equal(g_null.view(torch.int32), g_zero.view(torch.int32))


@pytest.mark.parametrize("name", SC.LONG_ROWS)
def test_two_runs_are_bitwise_equal(name):
    eng = stepped(name)
    first = [t.clone() for t in (eng.energy, eng.forces, eng.grad)]
    eng.train_step()
    for a, b in zip(first, (eng.energy, eng.forces, eng.grad)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_molecule_alone_gets_the_forces_it_gets_inside_the_batch():
    """Every kernel works per pair or per atom row in a fixed order, and the dense products of these sizes stay on the exact-float32 tile engine, whose
    rows do not depend on the batch (test_engine_gpu.py:test_gemm_rows_do_not_depend_on_the_batch): the 70-atom molecule of long_rows gets bitwise the
    same energy and per-atom forces alone as inside the batch."""
    case = SC.get_case("long_rows-F64")
    full = stepped("long_rows-F64")
    alone = Engine(SC.sub_case(case, 2))
    e, f = alone.forward(True)
    keep = (case.batch == 2).nonzero().flatten()
    assert f.shape[0] == 70
    assert torch.equal(f.cpu().view(torch.int32), full.forces.cpu()[keep].view(torch.int32))
    assert torch.equal(e.cpu().view(torch.int32), full.energy.cpu()[2:3].view(torch.int32))


@pytest.mark.parametrize("F,R", [(64, 269), (128, 269), (256, 157)])
def test_n_rbf_beyond_the_sort_or_lds_is_refused_before_any_launch(F, R):
    """(64, 268) and (256, 156) run (cases sort_limit and lds_limit); one more is refused by the argument check, not by the k0 sort after the embedding,
    the pair kernel and the window kernel were launched: workspace and outputs keep their NaN fill."""
    from nabladft_amd import _lib
    base = SC.get_case("one_pair")
    case = dataclasses.replace(base, cfg=dataclasses.replace(base.cfg, n_atom_basis=F, n_interactions=1, n_rbf=R))
    eng = Engine(case)
    assert eng.forward_rc(True) == _lib.NQ_ERR_ARG
    assert b"n_rbf" in eng.lib.nq_last_error(), eng.lib.nq_last_error()
    assert bool(torch.isnan(eng.ws).all()) and bool(torch.isnan(eng.energy).all()) and bool(torch.isnan(eng.forces).all())
    ge, gf = torch.zeros(eng.B, device=eng.dev), torch.zeros(eng.N, 3, device=eng.dev)
    assert eng.backward_rc(ge, gf) == _lib.NQ_ERR_ARG
    assert b"n_rbf" in eng.lib.nq_last_error(), eng.lib.nq_last_error()
    assert bool(torch.isnan(eng.ws).all()) and bool(torch.isnan(eng.grad).all())


def test_spk_painn_long_rows():
    """The cosine-cutoff window (mode 1) of the PaiNN engine with rows over 64: the long_rows geometry through spk.PaiNN against
    oracle/spk_painn_ref.py:spk_train_step, to the bounds of tests/test_spk_gpu.py.  Default initialisation, no weight rescaled."""
    from nabladft_amd import spk
    from oracle import spk_painn_ref as SP
    case = SC.get_case("long_rows-F64")
    deg, _ = SC.row_stats(case)
    assert int(deg.max()) > 64
    scfg = SP.SpkPaiNNConfig(n_atom_basis=64, n_interactions=2, n_rbf=20, cutoff=6.0, max_z=20)
    P = SP.make_spk_params(scfg, seed=66)
    P64 = {k: v.double() for k, v in P.items()}
    e_ref, f_ref, loss_ref, g_ref = SP.spk_train_step(P64, scfg, case.pos.double(), case.z, case.batch, case.y.double(), case.ft.double())
    pot = spk.NeuralNetworkPotential(
        representation=spk.PaiNN(n_atom_basis=64, n_interactions=2, radial_basis=spk.GaussianRBF(n_rbf=20, cutoff=6.0), cutoff_fn=spk.CosineCutoff(6.0), max_z=20),
        input_modules=[spk.PairwiseDistances()], output_modules=[spk.Atomwise(n_in=64, output_key="energy"), spk.Forces(energy_key="energy", force_key="forces")])
    missing, unexpected = pot.load_state_dict(P, strict=False)
    assert not unexpected and all(("radial_basis" in m or "cutoff_fn" in m) for m in missing), (missing, unexpected)
    pot = pot.cuda().train()
    out = pot({"_positions": case.pos.cuda(), "_atomic_numbers": case.z.cuda(), "_idx_m": case.batch.cuda()})
    loss = torch.nn.functional.mse_loss(out["energy"], case.y.cuda()) + torch.nn.functional.mse_loss(out["forces"], case.ft.cuda())
    loss.backward()
    e_err, f_err = rel_err(out["energy"].detach().cpu().numpy(), e_ref.numpy()), rel_err(out["forces"].detach().cpu().numpy(), f_ref.numpy())
    _note("spk_painn_long", "energy", "energy", e_err, 0.0, E_TOL)
    _note("spk_painn_long", "forces", "forces", f_err, 0.0, F_TOL)
    bad = []
    for k, p in pot.named_parameters():
        g = g_ref[k].numpy()
        assert p.grad is not None, k
        scale = max(np.abs(g).max(), np.sqrt((g ** 2).mean()) + 1e-30)
        err = float(np.abs(p.grad.cpu().numpy().astype(np.float64) - g).max() / scale)
        if not _note("spk_painn_long", "grads", k, err, 0.0, G_TOL):
            bad.append((k, err))
    assert e_err < E_TOL and f_err < F_TOL, (e_err, f_err)
    assert abs(loss.item() - loss_ref.item()) < 2e-5 * abs(loss_ref.item())
    assert not bad, bad
