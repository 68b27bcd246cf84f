"""The GemNet-OC graph kernels (csrc/gemnet_graph.hip) through nq_gn_graph_count / nq_gn_graph_fill against numpy restatements of the same selection
(tests/gemnet_graph_cases.py), on batches built to reach what the 26-54-atom fixtures of test_gemnet_gpu.py never reach.  The a2a radius graph comes from
build_neighbor_list exactly as gemnet_oc.build_graphs makes it and is itself compared with a brute-force float32 radius graph.  Every output buffer starts
as a sentinel (-1 for index arrays, a negative garbage value for counters and pointers, 0xFF for the flags, NaN for geometry), so an element a kernel never
writes fails; count + fill run twice into fresh buffers and must agree bitwise.

Bounds: everything is exact (integer or bitwise) except the distance, which must lie within max(1 float32 ulp, the error of torch.norm in float32 on the
CPU) of the float64 norm of the float32 difference (the rule of test_escn_ops_gpu.py::test_graph).  The keep sets are the rule of utils.py:452-500 on the
distances the kernel itself wrote (after those passed that check), so a last-bit difference between two correct square roots cannot change an edge set.
tests/test_gemnet_graph_cases_cpu.py holds the same restatement against the CPU oracle and asserts that every batch still has the properties named below.

Branches and the tests that reach them (test_graph_tables[batch-configuration]):
  k_gn_geom        every a2a slot rewritten (NaN sentinel), sqrt / division rounding: all five
  k_gn_flags       the t0 loop past the first 64-lane chunk (rows of 65..129 entries; 63 and 64 too): chunks-*; eight chunks, sd[GN_MAXDEG] full but for
                   one entry: largest-yaml; cutoff and cap both selecting: chunks-caps; cap only: chunks-yaml, largest-yaml; K = 1: chunks-k1; cutoff only
                   (K = 1 << 20): chunks-nocap; d == cutoff kept and one ulp above dropped (<=): chunks-caps / -nocap (cutoff molecule); exact ties at the
                   cap, lower row position wins: chunks-caps (tie molecule); rows with no kept edge (cnt_q = 0): chunks-caps / -k1 / -nocap
  k_gn_maindeg     rows past 64 / 128 entries, members on both sides of the diagonal: chunks-*, largest-yaml; a2a row empty: largest-yaml (atom 514)
  k_gn_tin         qint rows empty / non-empty: chunks-caps
  k_gn_scan        the carry across 1024-thread passes, all five scans, the N-th entries: chunks-* (1110 atoms); one short pass: largest-yaml (515)
  k_gn_fill        om / oa / oq carried into the second and third chunk (kept edges at row positions >= 64 and >= 128): chunks-caps; into the eighth:
                   largest-yaml; mpos / apos / qpos = -1 where absent: all; the tin_main j += 64 loop past one chunk (main rows up to 124): chunks-caps,
                   -nocap; tin_ptr[Eq] written by the last block: all
  k_gn_link        m_rev, a_of_rev / q_of_rev = -1 or the flipped edge: all
  refusals (before any launch): max_degree = GN_MAXDEG + 1, NULL arguments, N <= 0, E <= 0: test_count_and_fill_refuse; build_graphs on a one-atom
                   molecule, cutoff_qint below every distance, max_neighbors_aint below the largest in-degree: test_build_graphs_refuses"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from oracle import gemnet_ref as R  # noqa: E402
from tests import gemnet_graph_cases as GC  # noqa: E402
from tests.helpers import DEV, _lib, _release_copies, bits, check, lib, nan_dev, st, twice  # noqa: E402,F401  (_release_copies: autouse)

GARBAGE = -7777                       # counters and pointers start as this
INPUTS = ("row_ptr", "col", "rev", "dst", "pos")
PER_ATOM = ("degm", "lowm", "cnt_a", "cnt_q", "tin_atom")
POINTERS = ("ptr_m", "lowptr_m", "ptr_a", "ptr_q", "tin_aptr")
PER_SLOT = ("mpos", "apos", "qpos", "a_of_rev", "q_of_rev")
_A2A = {}


def a2a(bname, cutoff_aint):
    """The a2a graph as gemnet_oc.build_graphs builds it (kept per batch and radius)."""
    key = (bname, cutoff_aint)
    if key not in _A2A:
        from nabladft_amd.painn import build_neighbor_list
        pos, sizes, _ = GC.batch(bname)
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
        z = torch.ones(len(pos), dtype=torch.long, device=DEV)
        _A2A[key] = build_neighbor_list(torch.tensor(pos, device=DEV), batch, z, cutoff_aint, 100000, None), batch, z
    return _A2A[key]


def full(n, value, dtype=torch.int32):
    return torch.full((n,), value, dtype=dtype, device=DEV)


def args(nl, cfg, out):
    """nq_gn_graphs over the a2a graph ``nl`` with the count-stage buffers (sentinels) allocated into ``out``."""
    g = _lib().GnGraphs()
    g.N, g.E, g.k_main, g.k_aea, g.k_qint, g.reserved = nl.N, nl.E, cfg["max_neighbors"], cfg["max_neighbors_aeaint"], cfg["max_neighbors_qint"], 0
    g.cutoff_main, g.cutoff_aea, g.cutoff_qint = cfg["cutoff"], cfg["cutoff_aeaint"], cfg["cutoff_qint"]
    for k in INPUTS:
        setattr(g, k, nl.t[k].data_ptr())
    out["geom"] = nan_dev(nl.E, 4)                                    # k_gn_geom rewrites every slot
    out["flags"] = full(nl.E, 0xFF, torch.uint8)
    for k in PER_ATOM:
        out[k] = full(nl.N, GARBAGE)
    for k in POINTERS:
        out[k] = full(nl.N + 1, GARBAGE)
    for k in PER_SLOT:
        out[k] = full(nl.E, -1)
    for k, v in out.items():
        setattr(g, k, v.data_ptr())
    return g


def count_and_fill(nl, cfg):
    """(out: name -> device tensor, totals) of one nq_gn_graph_count + nq_gn_graph_fill into fresh sentinel-filled buffers."""
    out = {}
    g = args(nl, cfg, out)
    totals = (C.c_int32 * 4)(GARBAGE, GARBAGE, GARBAGE, GARBAGE)
    check(lib().nq_gn_graph_count(C.byref(g), int(nl.t["deg"].max()), totals, st()))
    Em, Ea, Eq, Tin = (int(v) for v in totals)
    assert min(Em, Ea, Eq, Tin) > 0
    fill = {}
    for k in ("m_src", "m_dst", "m_rev", "m_slot"):
        fill[k] = full(Em, -1)
    for k, n in (("a_src", Ea), ("a_dst", Ea), ("q_src", Eq), ("q_dst", Eq), ("tin_main", Tin)):
        fill[k] = full(n, -1)
    for k, n in (("m_geom", Em), ("a_geom", Ea), ("q_geom", Eq)):
        fill[k] = nan_dev(n, 4)
    fill["tin_ptr"] = full(Eq + 1, GARBAGE)
    for k, v in fill.items():
        setattr(g, k, v.data_ptr())
    out.update(fill)
    check(lib().nq_gn_graph_fill(C.byref(g), st()))
    return out, [Em, Ea, Eq, Tin]


def host(t):
    a = t.detach().cpu().numpy()
    return a.astype(np.int64) if a.dtype == np.int32 else a


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32), np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


# ---- the checks, on host copies --------------------------------------------------------------------------------------------------------------------
def check_a2a(pos, sizes, cfg, col, dst, row_ptr, rev):
    """The a2a input: the brute-force float32 radius graph, rev an involution that flips (col, dst)."""
    rs, rd, rp = GC.radius_graph(pos, sizes, cfg["cutoff_aint"])
    E = len(rs)
    assert np.array_equal(col, rs) and np.array_equal(dst, rd) and np.array_equal(row_ptr, rp)
    assert rev.min() >= 0 and rev.max() < E and np.array_equal(rev[rev], np.arange(E))
    assert np.array_equal(col[rev], dst) and np.array_equal(dst[rev], col)


def check_geometry(label, h, pos, col, dst):
    geom = h["geom"]
    assert not np.isnan(geom).any()
    diff = pos[col] - pos[dst]                                        # one float32 subtraction per component
    w = geom[:, 3]
    n64 = np.sqrt((diff.astype(np.float64) ** 2).sum(-1))
    ulp = np.spacing(n64.astype(np.float32)).astype(np.float64)
    own = np.abs(torch.tensor(diff).norm(dim=1).double().numpy() - n64)
    err = np.abs(w.astype(np.float64) - n64)
    print(f"{label}: E {len(col)}  |w - n64| max {err.max():.3e} ({(err / ulp).max():.3f} ulp)  torch.norm in float32: {own.max():.3e} "
          f"({(own / ulp).max():.3f} ulp)  edges above 1 ulp {int((err > ulp).sum())}")
    assert (err <= np.maximum(ulp, own)).all()
    assert same_bits(geom[:, :3], diff / w[:, None])                  # IEEE float32 division by the kernel's own distance
    for pre in ("m", "a", "q"):                                       # the sub-graphs carry the a2a entry of their slot, vector negated
        slot = h["m_slot"] if pre == "m" else np.nonzero(h["flags"] & (2 if pre == "a" else 4))[0]
        assert same_bits(h[pre + "_geom"], np.concatenate([-geom[slot, :3], geom[slot, 3:]], axis=1)), pre


def check_tables(h, totals, col, dst, row_ptr, rev, cfg):
    """Every table against the keep sets of the reference's rule on the kernel's own distances."""
    Em, Ea, Eq, Tin = totals
    T = GC.tables(col, dst, row_ptr, rev, h["geom"][:, 3], cfg)
    assert totals == T["totals"]
    for k in ("flags",) + PER_ATOM + POINTERS + ("m_src", "m_dst", "m_slot", "a_src", "a_dst", "q_src", "q_dst", "mpos", "apos", "qpos", "m_rev",
                                                 "a_of_rev", "q_of_rev", "tin_ptr", "tin_main"):
        assert h[k].shape == T[k].shape and np.array_equal(h[k], T[k]), k
    m_rev = h["m_rev"]
    assert m_rev.min() >= 0 and np.array_equal(m_rev, h["mpos"][rev[h["m_slot"]]]) and np.array_equal(m_rev[m_rev], np.arange(Em))
    assert np.array_equal(h["m_src"][m_rev], h["m_dst"]) and np.array_equal(h["m_dst"][m_rev], h["m_src"])
    assert len(h["tin_ptr"]) == Eq + 1 and h["tin_ptr"][-1] == Tin
    for q in range(0, Eq, max(1, Eq // 997)):                         # the definition spelled out on a sample (the full array is compared above)
        s, t0 = h["q_src"][q], h["tin_ptr"][q]
        assert np.array_equal(h["tin_main"][t0:t0 + h["degm"][s]], h["ptr_m"][s] + np.arange(h["degm"][s]))


def check_named(bname, cname, named, h, col, dst, row_ptr):
    """What the batch was built for, on the device result (the statements of test_gemnet_graph_cases_cpu.py)."""
    N, E, w = len(row_ptr) - 1, len(col), h["geom"][:, 3]
    if bname == "chunks":
        GC.assert_named_chunks(cname, named, (h["q_src"], h["q_dst"]), N)
        a = named["cutoff"]
        near = {int(s): float(x) for s, x in zip(col[dst == a], w[dst == a])}
        assert near[a + 1] == 3.0 and near[a + 2] == float(np.nextafter(np.float32(3.0), np.float32(4.0))) and near[a + 3] == 1.0
        assert set(w[dst == named["tie"]].tolist()) == {1.5}
        assert N > 1024 and np.diff(row_ptr).max() > 128
        if cname == "caps":
            assert int((h["cnt_q"] == 0).sum()) == 1 and h["cnt_q"][a + 2] == 0 and h["tin_atom"][a + 2] == 0
    else:
        GC.assert_named_largest(named, (col, dst), N)
        lonely = named["lonely"]
        assert np.diff(row_ptr).max() == 511 and row_ptr[lonely] == row_ptr[lonely + 1] == E
        assert h["degm"][lonely] == h["cnt_a"][lonely] == h["cnt_q"][lonely] == h["tin_atom"][lonely] == 0


@pytest.mark.parametrize("bname,cname", GC.CASES, ids=[f"{b}-{c}" for b, c in GC.CASES])
def test_graph_tables(bname, cname):
    pos, sizes, named = GC.batch(bname)
    cfg = GC.CONFIGS[cname]
    nl, batch, z = a2a(bname, cfg["cutoff_aint"])
    col, dst, row_ptr, rev = (host(nl.t[k]) for k in ("col", "dst", "row_ptr", "rev"))
    assert nl.N == len(pos) and nl.E == len(col) == row_ptr[-1]
    check_a2a(pos, sizes, cfg, col, dst, row_ptr, rev)

    # ---- count + fill, twice, bitwise equal ----
    names, totals = [], []

    def call():
        out, tot = count_and_fill(nl, cfg)
        names[:] = list(out)
        totals.append(tot)
        return [out[k] for k in names]

    out = dict(zip(names, twice(call)))
    assert totals[0] == totals[1]
    h = {k: host(v) for k, v in out.items()}
    check_geometry(f"{bname}-{cname}", h, pos, col, dst)
    check_tables(h, totals[0], col, dst, row_ptr, rev, cfg)

    # ---- the product path writes the same tensors; its reference layout equals the oracle's, given the same distances ----
    from nabladft_amd.gemnet_oc import build_graphs
    G = build_graphs(nl.t["pos"], batch, z, cfg["cutoff"], cfg["cutoff_qint"], cfg["cutoff_aeaint"], cfg["cutoff_aint"], cfg["max_neighbors"],
                     cfg["max_neighbors_qint"], cfg["max_neighbors_aeaint"], cfg["max_neighbors_aint"])
    assert [G.Em, G.Ea, G.Eq, G.Tin] == totals[0] and G.N == nl.N and G.Ea2a == nl.E
    for k, v in out.items():
        a, b = v.cpu(), G.t[k].cpu()
        assert a.shape == b.shape and torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b), k
    for k in INPUTS[:4]:
        assert torch.equal(G.t[k].cpu(), nl.t[k].cpu()), k
    ref = G.to_reference()
    O = R.build_graphs(torch.tensor(pos), sizes, cfg, dist=h["geom"][:, 3])
    for name in ("a2a", "a2ee2a", "qint", "main"):
        assert np.array_equal(ref[name]["edge_index"], np.stack(O[name])), name
    assert np.array_equal(ref["id_swap"], O["id_swap"])
    assert np.array_equal(ref["a2a"]["distance"], h["geom"][:, 3]) and same_bits(ref["a2a"]["vector"], -h["geom"][:, :3])
    check_named(bname, cname, named, h, col, dst, row_ptr)


def test_count_and_fill_refuse():
    """max_degree above GN_MAXDEG, NULL arguments and an empty graph are refused before any launch: no buffer is touched."""
    L = _lib()
    cfg = GC.CONFIGS["caps"]
    nl, _, _ = a2a("chunks", cfg["cutoff_aint"])
    out = {}
    g = args(nl, cfg, out)
    totals = (C.c_int32 * 4)(GARBAGE, GARBAGE, GARBAGE, GARBAGE)

    def refused(code, call):
        with pytest.raises(L.NablaqError) as e:
            check(call())
        assert e.value.code == code
        torch.cuda.synchronize()
        assert list(totals) == [GARBAGE] * 4 and torch.isnan(out["geom"]).all() and (out["flags"] == 0xFF).all()
        for k in PER_ATOM + POINTERS:
            assert (out[k] == GARBAGE).all(), k
        for k in PER_SLOT:
            assert (out[k] == -1).all(), k

    refused(L.NQ_ERR_MOL_TOO_LARGE, lambda: lib().nq_gn_graph_count(C.byref(g), 513, totals, st()))
    refused(L.NQ_ERR_ARG, lambda: lib().nq_gn_graph_count(None, 100, totals, st()))
    refused(L.NQ_ERR_ARG, lambda: lib().nq_gn_graph_count(C.byref(g), 100, None, st()))
    refused(L.NQ_ERR_ARG, lambda: lib().nq_gn_graph_fill(None, st()))
    for n, e in ((0, nl.E), (-1, nl.E), (nl.N, 0), (nl.N, -5)):
        g.N, g.E = n, e
        refused(L.NQ_ERR_NO_EDGES, lambda: lib().nq_gn_graph_count(C.byref(g), 100, totals, st()))


def test_build_graphs_refuses():
    from nabladft_amd.gemnet_oc import build_graphs
    pos = torch.tensor(np.concatenate([GC.TIE_MOLECULE, GC.CUTOFF_MOLECULE + 20.0]), device=DEV)
    z = torch.ones(12, dtype=torch.long, device=DEV)

    def build(p, sizes, cutoff_qint=3.0, max_aint=1000):
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
        return build_graphs(p, batch, z[:len(p)], 5.0, cutoff_qint, 4.0, 6.0, 80, 4, 20, max_aint)

    assert build(pos, [7, 4]).Eq > 0                                  # the same batch is accepted ...
    lone = torch.cat([pos, pos[:1] + 40.0])
    with pytest.raises(ValueError):                                   # ... but not with a one-atom molecule behind it,
        build(lone, [7, 4, 1])
    with pytest.raises(ValueError):                                   # with cutoff_qint below every distance (1.0 is the shortest),
        build(pos, [7, 4], cutoff_qint=0.5)
    with pytest.raises(NotImplementedError):                          # or with fewer a2a neighbours allowed than the centre of the tie molecule has
        build(pos, [7, 4], max_aint=5)
