"""The GemNet-OC interaction kernels (csrc/gemnet.hip) one by one through the C ABI against float64 restatements of the same operation, built from the
kernel's own float32 inputs (the device graphs' CSR arrays and unit vectors, promoted): the index lists come from the oracle's builders
(oracle/gemnet_ref.py: triplets, quadruplets) run on the CSR arrays, so reference and kernel address the same rows.  Every output buffer starts as NaN,
so an element a kernel never writes fails the comparison.

Bounds (the convention of test_gemnet_gpu.py): copies / selections are exact; every summing kernel must stay within max(3 x the error of the same
formula evaluated in float32 on the CPU, 2e-6) of the float64 value AND below 1e-5, both array-relative (max |a - b| / max |b|)."""
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
from tests.helpers import DEV, D, P, _lib, _release_copies, assert_sum, check, lib, nan_dev, rnd, st  # noqa: E402,F401  (_release_copies: autouse)


# ---- graphs -------------------------------------------------------------------------------------------------------------------------------------------
def cloud(seed, sizes, spread, sep=0.9):
    """Random molecules grown atom by atom (each new atom near an earlier one, at least ``sep`` from all), one random offset per molecule."""
    rng = np.random.default_rng(seed)
    pos = []
    for n in sizes:
        p = [np.zeros(3)]
        while len(p) < n:
            c = p[rng.integers(len(p))] + rng.normal(size=3) / np.sqrt(3) * spread
            if min(np.linalg.norm(c - q) for q in p) > sep:
                p.append(c)
        pos.append(np.array(p) + rng.normal(size=3) * 3.0)
    return np.concatenate(pos).astype(np.float32)


def lattice():
    """Atoms on the three axes (and the origin): every collinear triple lies on an axis, so the float32 unit vectors of those edges are exactly +-e_i,
    their dot products exactly +-1 and their cross products exactly zero (the 1e-9 floor of the dihedral); many quadruplets are coplanar."""
    pts = [(0, 0, 0)] + [(x, 0, 0) for x in (-2, -1, 1, 2)] + [(0, y, 0) for y in (-1, 1, 2)] + [(0, 0, z) for z in (-2, -1, 1)]
    return np.array(pts, dtype=np.float32)


# name: (positions, molecule sizes, cutoff, cutoff_qint, cutoff_aeaint, cutoff_aint, max_neighbors, max_neighbors_qint, max_neighbors_aeaint)
GRAPHS = {
    # one dense molecule: main in-degrees 40..79 (two GQ_PC chunks, two GQ_PB blocks, > 16 out edges everywhere), qint in-degrees 0..4 with KQ = 4
    "dense": (lambda: cloud(5, (80,), 1.4), (80,), 12.0, 2.0, 6.0, 12.0, 50, 4, 20),
    # two small molecules, the test fixtures' caps
    "small": (lambda: cloud(11, (14, 9), 1.5), (14, 9), 5.0, 4.0, 4.5, 5.5, 6, 3, 4),
    "lattice": (lattice, (11,), 5.0, 5.0, 5.0, 5.0, 12, 12, 12),
}
_CACHE = {}


class Graph:
    pass


def graph(name):
    if name in _CACHE:
        return _CACHE[name]
    from nabladft_amd.gemnet_oc import build_graphs
    mk, sizes, cut, cq, ca, caint, k, kq, ka = GRAPHS[name]
    pos = torch.tensor(mk(), device=DEV)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    z = torch.ones(pos.shape[0], dtype=torch.long, device=DEV)
    G = build_graphs(pos, batch, z, cut, cq, ca, caint, k, kq, ka, 1000)
    g = Graph()
    g.G = G
    g.h = {k: v.cpu().numpy().astype(np.int64) if v.dtype == torch.int32 else v.cpu().numpy() for k, v in G.t.items() if torch.is_tensor(v)}
    h = g.h
    g.N = G.N
    g.main = (h["m_src"], h["m_dst"])
    g.aea = (h["a_src"], h["a_dst"])
    g.qint = (h["q_src"], h["q_dst"])
    g.vm, g.va, g.vq = (torch.tensor(h[k][:, :3]) for k in ("m_geom", "a_geom", "q_geom"))
    g.degm, g.dega, g.degq = (np.diff(h[k]) for k in ("ptr_m", "ptr_a", "ptr_q"))
    # rows of the (qint edge q, j-th main in-edge of source(q)) table: row = tin_ptr[q] + j  <->  main slot p = ptr_m[source(q)] + j
    tin = h["tin_ptr"][:G.Eq + 1]
    lens = np.diff(tin)
    assert np.array_equal(lens, g.degm[h["q_src"]])
    g.row_q = np.repeat(np.arange(G.Eq), lens)
    g.row_j = np.arange(tin[-1]) - tin[g.row_q]
    g.row_p = h["ptr_m"][h["q_src"][g.row_q]] + g.row_j
    g.T = int(tin[-1])
    assert g.T == G.Tin
    _CACHE[name] = g
    return g


# ---- triplets -------------------------------------------------------------------------------------------------------------------------------------------
_TRI = {}
FAMILIES = {"e2e": ("main", "main"), "a2e": ("main", "aea"), "e2a": ("aea", "main")}


def _sets(g, fam):
    o, i = FAMILIES[fam]
    sv = {"main": (g.G.main, g.main, g.vm, "ptr_m"), "aea": (g.G.aea, g.aea, g.va, "ptr_a")}
    return sv[o], sv[i]


def tri_ref(g, fam, X, dS, NS, scale, dtype):
    """S[o, s, c] = sum_{p: target(p) = target(o), source(p) != source(o)} Y_s(v_o . v_p) X[p, c] and its adjoint, over the oracle's triplet list."""
    (_, O, vO, _), (_, I, vI, _) = _sets(g, fam)
    key = (id(g), fam)
    if key not in _TRI:
        _TRI[key] = tuple(torch.as_tensor(a) for a in R.triplets(O, I, g.N))
    i_in, i_out = _TRI[key]
    Y = R.zonal((vO.to(dtype)[i_out] * vI.to(dtype)[i_in]).sum(-1).clamp(-1, 1), NS) * scale
    X, dS = X.to(dtype), dS.to(dtype).reshape(len(O[0]), NS, -1)
    S = R.seg_outer(Y, X[i_in], i_out, len(O[0]))
    dX = torch.zeros_like(X).index_add_(0, i_in, torch.einsum("ts,tsc->tc", Y, dS[i_out]))
    return S.reshape(len(O[0]), -1), dX


@pytest.mark.parametrize("fam", list(FAMILIES))
@pytest.mark.parametrize("Cc,NS", [(1, 2), (16, 7), (64, 8), (100, 1)])
def test_triplet_forward_backward(fam, Cc, NS):
    g = graph("dense")
    (so, O, _, _), (si, I, _, _) = _sets(g, fam)
    gen = torch.Generator().manual_seed(Cc * 10 + NS)
    scale = 0.73
    X, dS = rnd(gen, len(I[0]), Cc), rnd(gen, len(O[0]), NS * Cc)
    S, dX = nan_dev(len(O[0]), NS * Cc), nan_dev(len(I[0]), Cc)
    check(lib().nq_gn_triplet_forward(C.byref(so), C.byref(si), D(X), Cc, NS, scale, P(S), st()))
    check(lib().nq_gn_triplet_backward(C.byref(so), C.byref(si), D(dS), Cc, NS, scale, P(dX), st()))
    S64, dX64 = tri_ref(g, fam, X, dS, NS, scale, torch.float64)
    S32, dX32 = tri_ref(g, fam, X, dS, NS, scale, torch.float32)
    assert_sum(f"{fam} S", S, S64, S32)
    assert_sum(f"{fam} dX", dX, dX64, dX32)


# ---- quadruplets ----------------------------------------------------------------------------------------------------------------------------------------
_QB = {}


def quad_tables(g, name, NS, scale, dtype):
    """Padded per-(atom a, qint slot jq) tables of the oracle's quadruplet list c -> a <- b <- d:
        Yl[a, jq, oi, l]      = scale * Y_l(cos cab)   (oi = slot of the out edge in the main row of a)
        Yk[a, jq, oi, pj, k]  = Y_k(cos dihedral)      (pj = slot of the main in-edge d -> b in the row of b), zero where (o, q, p) is no quadruplet."""
    key = (name, NS, scale, dtype)
    if key in _QB:
        return _QB[key]
    if (name, "list") not in _QB:
        _QB[(name, "list")] = tuple(torch.as_tensor(a) for a in R.quadruplets(g.main, g.qint, g.N))
    qo, qq, qp = _QB[(name, "list")]
    h = g.h
    Yc, Yd = R.quad_basis(g.vm.to(dtype)[qo], g.vq.to(dtype)[qq], g.vm.to(dtype)[qp], NS)
    KQm, D = int(g.degq.max()), int(g.degm.max())
    a = torch.as_tensor(h["m_dst"])[qo]
    jq = qq - torch.as_tensor(h["ptr_q"])[a]
    oi = qo - torch.as_tensor(h["ptr_m"])[a]
    pj = qp - torch.as_tensor(h["ptr_m"])[torch.as_tensor(h["q_src"])[qq]]
    Yl = torch.zeros(g.N, KQm, D, NS, dtype=dtype)
    Yk = torch.zeros(g.N, KQm, D, D, NS, dtype=dtype)
    Yl[a, jq, oi] = Yc * scale
    Yk[a, jq, oi, pj] = Yd
    _QB[key] = (Yl, Yk)
    return Yl, Yk


def quad_ref(g, name, X, dS, NS, scale, dtype):
    """S[o, l, k, c] = sum_{(o, q, p)} Yl Yk X[tin_ptr[q] + (p - ptr_m[source(q)]), c] and the adjoint dX, both as batched products over the padded
    tables (the contraction over p per (a, jq), then over jq per out edge)."""
    h = g.h
    Yl, Yk = quad_tables(g, name, NS, scale, dtype)
    N, KQm, D = Yl.shape[:3]
    Cc = X.shape[1]
    qa = torch.as_tensor(h["q_dst"])[g.row_q]
    rq = (qa, torch.as_tensor(g.row_q) - torch.as_tensor(h["ptr_q"])[qa], torch.as_tensor(g.row_j))
    Xq = torch.zeros(N, KQm, D, Cc, dtype=dtype)
    Xq[rq] = X.to(dtype)
    tl = torch.bmm(Yk.permute(0, 1, 2, 4, 3).reshape(N * KQm, D * NS, D), Xq.reshape(N * KQm, D, Cc))          # [a jq, (oi k), c]
    tl = tl.reshape(N, KQm, D, NS * Cc).permute(0, 2, 1, 3).reshape(N * D, KQm, NS * Cc)
    Sp = torch.bmm(Yl.permute(0, 2, 3, 1).reshape(N * D, NS, KQm), tl).reshape(N, D, NS * NS * Cc)                # [a oi, l, (k c)]
    md, pm = torch.as_tensor(h["m_dst"]), torch.as_tensor(h["ptr_m"])
    o_a, o_i = md, torch.arange(len(md)) - pm[md]
    S = Sp[o_a, o_i]
    dSp = torch.zeros(N, D, NS, NS * Cc, dtype=dtype)
    dSp[o_a, o_i] = dS.to(dtype).reshape(-1, NS, NS * Cc)
    U = torch.bmm(Yl.permute(0, 2, 1, 3).reshape(N * D, KQm, NS), dSp.reshape(N * D, NS, NS * Cc))               # [a oi, jq, (k c)]
    U = U.reshape(N, D, KQm, NS, Cc).permute(0, 2, 1, 3, 4).reshape(N * KQm, D * NS, Cc)
    dXq = torch.bmm(Yk.permute(0, 1, 3, 2, 4).reshape(N * KQm, D, D * NS), U).reshape(N, KQm, D, Cc)
    return S, dXq[rq]


def quad_call(g, X, dS, Cc, NS, scale):
    G = g.G
    assert G.KQ >= int(g.degq.max())                                             # the scratch U holds KQ qint slots per out edge
    S = nan_dev(G.Em, NS * NS * Cc)
    dX = nan_dev(g.T, Cc)
    scr = torch.empty(G.Em * G.KQ * NS * Cc + 64, device=DEV)
    tin = P(G.t["tin_ptr"])
    check(lib().nq_gn_quad_forward(C.byref(G.main), C.byref(G.qint), tin, G.N, D(X), Cc, NS, scale, P(S), st()))
    check(lib().nq_gn_quad_backward(C.byref(G.main), C.byref(G.qint), tin, G.N, g.T, D(dS), Cc, NS, G.KQ, scale, P(scr), P(dX), st()))
    return S, dX


def _unwritten_rows(g, dX):
    """Positions (row of the block of 32 main in-edges) of the dX rows a kernel left unwritten -- the diagnostic of a per-block coverage gap."""
    bad = torch.isnan(dX.cpu()).any(1).numpy()
    return sorted(set((g.row_j[bad] % 32).tolist()))


def test_quad_graph_crosses_the_kernel_boundaries():
    g = graph("dense")
    h = g.h
    src_deg = g.degm[h["q_src"]]                                                 # main rows walked per qint edge
    assert src_deg.max() > 64 and ((src_deg > 32) & (src_deg <= 64)).any()    # two GQ_PC chunks / two and three GQ_PB blocks (graph "small": one)
    assert g.degm.min() > 16 and (g.degm > 64).any()                             # out edges per atom: > GQ_OC (8) and > GQ_UC (16) passes
    assert (g.degq == 0).any() and (g.degq < g.G.KQ).sum() > 1                   # an atom without qint in-edges; padding rows of U


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("Cc,NS", [(1, 8), (8, 3), (32, 7), (36, 1), (40, 8), (48, 3), (64, 7), (65, 1), (96, 3)])
def test_quad_forward_backward(variant, Cc, NS):
    g = graph("dense")
    gen = torch.Generator().manual_seed(Cc * 10 + NS)
    scale = 1.37
    X, dS = rnd(gen, g.T, Cc), rnd(gen, g.G.Em, NS * NS * Cc)
    lib().nq_gn_set_quad_variant(variant)
    try:
        S, dX = quad_call(g, X, dS, Cc, NS, scale)
        torch.cuda.synchronize()
    finally:
        lib().nq_gn_set_quad_variant(1)
    S64, dX64 = quad_ref(g, "dense", X, dS, NS, scale, torch.float64)
    S32, dX32 = quad_ref(g, "dense", X, dS, NS, scale, torch.float32)
    assert not torch.isnan(dX).any(), f"dX rows never written at block positions {_unwritten_rows(g, dX)} (C = {Cc}, variant {variant})"
    assert_sum("quad S", S, S64, S32)
    assert_sum("quad dX", dX, dX64, dX32)
    # adjoint identity on the kernel outputs: <S, dS> = <X, dX>
    lhs = float((S.cpu().double() * dS.double()).sum())
    rhs = float((X.double() * dX.cpu().double()).sum())
    scale_ip = float(S.cpu().double().norm() * dS.double().norm())
    assert abs(lhs - rhs) <= 1e-6 * scale_ip, (lhs, rhs, scale_ip)


@pytest.mark.parametrize("NS", [1, 3, 7, 8])
def test_quad_small_graph_all_num_spherical(NS):
    """The fixtures' caps (KQ = 3 > several atoms' qint in-degree) at C = 32, both variants."""
    g = graph("small")
    gen = torch.Generator().manual_seed(NS)
    X, dS = rnd(gen, g.T, 32), rnd(gen, g.G.Em, NS * NS * 32)
    S64, dX64 = quad_ref(g, "small", X, dS, NS, 0.9, torch.float64)
    S32, dX32 = quad_ref(g, "small", X, dS, NS, 0.9, torch.float32)
    for variant in (1, 0):
        lib().nq_gn_set_quad_variant(variant)
        try:
            S, dX = quad_call(g, X, dS, 32, NS, 0.9)
            torch.cuda.synchronize()
        finally:
            lib().nq_gn_set_quad_variant(1)
        assert_sum(f"quad S v{variant}", S, S64, S32)
        assert_sum(f"quad dX v{variant}", dX, dX64, dX32)


def test_degenerate_geometry_triplets_and_quadruplets():
    g = graph("lattice")
    vm = g.vm.numpy()
    i_in, i_out = R.triplets(g.main, g.main, g.N)
    dots = (vm[i_out] * vm[i_in]).sum(-1)
    assert (dots == 1.0).any() and (dots == -1.0).any()                          # exactly +-1 in float32: the clamp
    qo, qq, qp = R.quadruplets(g.main, g.qint, g.N)
    cross = np.cross(vm[qo], g.vq.numpy()[qq])
    assert (np.abs(cross).sum(-1) == 0).any()                                    # c, a, b collinear: the 1e-9 floor of the dihedral
    cross_d = np.cross(vm[qp], g.vq.numpy()[qq])
    assert (np.abs(cross_d).sum(-1) == 0).any()                                  # d, b, a collinear
    gen = torch.Generator().manual_seed(2)
    for fam in FAMILIES:
        (so, O, _, _), (si, I, _, _) = _sets(g, fam)
        X, dS = rnd(gen, len(I[0]), 16), rnd(gen, len(O[0]), 7 * 16)
        S, dX = nan_dev(len(O[0]), 7 * 16), nan_dev(len(I[0]), 16)
        check(lib().nq_gn_triplet_forward(C.byref(so), C.byref(si), D(X), 16, 7, 1.0, P(S), st()))
        check(lib().nq_gn_triplet_backward(C.byref(so), C.byref(si), D(dS), 16, 7, 1.0, P(dX), st()))
        S64, dX64 = tri_ref(g, fam, X, dS, 7, 1.0, torch.float64)
        S32, dX32 = tri_ref(g, fam, X, dS, 7, 1.0, torch.float32)
        assert_sum(f"lattice {fam} S", S, S64, S32)
        assert_sum(f"lattice {fam} dX", dX, dX64, dX32)
    for variant in (1, 0):
        X, dS = rnd(gen, g.T, 8), rnd(gen, g.G.Em, 49 * 8)
        lib().nq_gn_set_quad_variant(variant)
        try:
            S, dX = quad_call(g, X, dS, 8, 7, 1.0)
            torch.cuda.synchronize()
        finally:
            lib().nq_gn_set_quad_variant(1)
        S64, dX64 = quad_ref(g, "lattice", X, dS, 7, 1.0, torch.float64)
        S32, dX32 = quad_ref(g, "lattice", X, dS, 7, 1.0, torch.float32)
        assert_sum(f"lattice quad S v{variant}", S, S64, S32)
        assert_sum(f"lattice quad dX v{variant}", dX, dX64, dX32)


# ---- circular basis and the (qint, main-in) table --------------------------------------------------------------------------------------------------------
def cir_ref(g, RW, dcir, I, NS, scale, dtype):
    q, p = torch.as_tensor(g.row_q), torch.as_tensor(g.row_p)
    Y = R.zonal((g.vq.to(dtype)[q] * g.vm.to(dtype)[p]).sum(-1).clamp(-1, 1), NS) * scale
    W = RW.to(dtype).reshape(-1, I, NS)
    cir = torch.einsum("tis,ts->ti", W[q], Y)
    dRW = torch.zeros_like(W).index_add_(0, q, torch.einsum("ti,ts->tis", dcir.to(dtype), Y))
    return cir, dRW.reshape(len(W), -1)


@pytest.mark.parametrize("I,NS", [(1, 1), (16, 7), (32, 1), (32, 7), (1, 7), (16, 1)])
def test_cir_forward_backward(I, NS):
    g = graph("dense")
    G = g.G
    gen = torch.Generator().manual_seed(I * 10 + NS)
    RW, dcir = rnd(gen, G.Eq, I * NS), rnd(gen, g.T, I)
    cir, dRW = nan_dev(g.T, I), nan_dev(G.Eq, I * NS)
    tin = P(G.t["tin_ptr"])
    check(lib().nq_gn_cir_forward(C.byref(G.main), C.byref(G.qint), tin, g.T, D(RW), I, NS, 0.8, P(cir), st()))
    check(lib().nq_gn_cir_backward(C.byref(G.main), C.byref(G.qint), tin, D(dcir), I, NS, 0.8, P(dRW), st()))
    c64, d64 = cir_ref(g, RW, dcir, I, NS, 0.8, torch.float64)
    c32, d32 = cir_ref(g, RW, dcir, I, NS, 0.8, torch.float32)
    assert_sum("cir", cir, c64, c32)
    assert_sum("dRW", dRW, d64, d32)


@pytest.mark.parametrize("name", ["dense", "small"])
def test_tin_scatter(name):
    """out[p] = sum over the qint edges q whose source is target(p) of g[tin_ptr[q] + (p - first slot of the row)] (the adjoint of the row gather)."""
    g = graph(name)
    G = g.G
    gen = torch.Generator().manual_seed(4)
    for Cc in (1, 32):
        gr = rnd(gen, g.T, Cc)
        out = nan_dev(G.Em, Cc)
        check(lib().nq_gn_tin_scatter(C.byref(G.main), P(G.t["row_ptr"]), P(G.t["q_of_rev"]), P(G.t["tin_ptr"]), D(gr), Cc, P(out), st()))
        p = torch.as_tensor(g.row_p)
        refs = [torch.zeros(G.Em, Cc, dtype=dt).index_add_(0, p, gr.to(dt)) for dt in (torch.float64, torch.float32)]
        assert_sum("tin_scatter", out, *refs)


# ---- per-row products --------------------------------------------------------------------------------------------------------------------------------
LDS = 64 * 1024


def _rowmm_lds(I, NSS, Cc):
    return 4 * (I * NSS + NSS * Cc), 4 * (I * NSS + NSS * (Cc + 1) + I * Cc)


@pytest.mark.parametrize("I,NSS,Cc", [(16, 7, 32), (16, 49, 64), (16, 49, 32), (16, 7, 64), (16, 7, 1), (16, 49, 33), (3, 5, 1),
                                      (16, 64, 240), (16, 64, 241), (15, 1, 1023), (15, 1, 1024), (16, 49, 239)])
def test_rowmm_forward_backward(I, NSS, Cc):
    lf, lb = _rowmm_lds(I, NSS, Cc)
    n = 37
    gen = torch.Generator().manual_seed(I + NSS + Cc)
    Rm, Sm, dout = rnd(gen, n, I * NSS), rnd(gen, n, NSS * Cc), rnd(gen, n, I * Cc)
    Rd, Sd, dd = Rm.to(DEV), Sm.to(DEV), dout.to(DEV)
    refs = {}
    for dt in (torch.float64, torch.float32):
        R3, S3, d3 = Rm.to(dt).reshape(n, I, NSS), Sm.to(dt).reshape(n, NSS, Cc), dout.to(dt).reshape(n, I, Cc)
        refs[dt] = (torch.bmm(R3, S3).reshape(n, -1), torch.bmm(d3, S3.transpose(1, 2)).reshape(n, -1), torch.bmm(R3.transpose(1, 2), d3).reshape(n, -1))
    out = nan_dev(n, I * Cc)
    if lf <= LDS:
        check(lib().nq_gn_rowmm_forward(P(Rd), P(Sd), n, I, NSS, Cc, P(out), st()))
        assert_sum("rowmm out", out, refs[torch.float64][0], refs[torch.float32][0])
    else:
        with pytest.raises(_lib().NablaqError):
            check(lib().nq_gn_rowmm_forward(P(Rd), P(Sd), n, I, NSS, Cc, P(out), st()))
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    for want_r, want_s in ((True, True), (True, False), (False, True)):
        dR, dS = nan_dev(n, I * NSS), nan_dev(n, NSS * Cc)
        args = (P(Rd), P(Sd), P(dd), n, I, NSS, Cc, P(dR) if want_r else None, P(dS) if want_s else None, st())
        if lb <= LDS:
            check(lib().nq_gn_rowmm_backward(*args))
            if want_r:
                assert_sum("rowmm dR", dR, refs[torch.float64][1], refs[torch.float32][1])
            if want_s:
                assert_sum("rowmm dS", dS, refs[torch.float64][2], refs[torch.float32][2])
        else:
            with pytest.raises(_lib().NablaqError):
                check(lib().nq_gn_rowmm_backward(*args))
        torch.cuda.synchronize()
        if not want_r or lb > LDS:
            assert torch.isnan(dR).all()
        if not want_s or lb > LDS:
            assert torch.isnan(dS).all()


def test_rowmm_shapes_cover_the_lds_limit():
    fwd = [_rowmm_lds(16, 64, 240)[0], _rowmm_lds(16, 64, 241)[0]]
    bwd = [_rowmm_lds(15, 1, 1023)[1], _rowmm_lds(15, 1, 1024)[1]]
    assert fwd[0] == LDS and fwd[1] > LDS and bwd[0] == LDS and bwd[1] > LDS


# ---- atom pairs ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rr", [1, 8, 16])
def test_pair_forward_backward(Rr):
    g = graph("dense")
    G = g.G
    h = g.h
    Cc = 24
    gen = torch.Generator().manual_seed(Rr)
    RW, X, dout = rnd(gen, G.Ea2a, Rr), rnd(gen, G.N, Cc), rnd(gen, G.N, Rr * Cc)
    out, dRW, dX = nan_dev(G.N, Rr * Cc), nan_dev(G.Ea2a, Rr), nan_dev(G.N, Cc)
    check(lib().nq_gn_pair_forward(C.byref(G.a2a), D(RW), D(X), G.N, Rr, Cc, P(out), st()))
    check(lib().nq_gn_pair_backward(C.byref(G.a2a), P(G.t["rev"]), D(RW), D(X), D(dout), G.N, Rr, Cc, P(dRW), P(dX), st()))
    src, dst = torch.as_tensor(h["col"]), torch.as_tensor(h["dst"])
    refs = {}
    for dt in (torch.float64, torch.float32):
        W, x, d = RW.to(dt), X.to(dt), dout.to(dt).reshape(G.N, Rr, Cc)
        o = R.seg_outer(W, x[src], dst, G.N).reshape(G.N, -1)
        dx = torch.zeros_like(x).index_add_(0, src, torch.einsum("pr,prc->pc", W, d[dst]))
        dw = torch.einsum("pc,prc->pr", x[src], d[dst])
        refs[dt] = (o, dw, dx)
    for k, name in enumerate(("pair out", "pair dRW", "pair dX")):
        assert_sum(name, (out, dRW, dX)[k], refs[torch.float64][k], refs[torch.float32][k])


def test_pair_rejects_too_many_radial_channels():
    G = graph("small").G
    RW, X = torch.zeros(G.Ea2a, 17, device=DEV), torch.zeros(G.N, 4, device=DEV)
    out = nan_dev(G.N, 17 * 4)
    with pytest.raises(_lib().NablaqError):
        check(lib().nq_gn_pair_forward(C.byref(G.a2a), P(RW), P(X), G.N, 17, 4, P(out), st()))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- atom side -------------------------------------------------------------------------------------------------------------------------------------------
def test_cat_forward_backward():
    g = graph("dense")
    G, h = g.G, g.h
    A, Em = 32, 20
    gen = torch.Generator().manual_seed(6)
    H, M, dcat = rnd(gen, G.N, A), rnd(gen, G.Em, Em), rnd(gen, G.Em, 2 * A + Em)
    cat, dH = nan_dev(G.Em, 2 * A + Em), nan_dev(G.N, A)
    check(lib().nq_gn_cat_forward(C.byref(G.main), D(H), D(M), A, Em, P(cat), st()))
    check(lib().nq_gn_cat_backward_h(C.byref(G.main), P(G.t["m_rev"]), D(dcat), G.N, A, Em, P(dH), st()))
    src, dst = torch.as_tensor(h["m_src"]), torch.as_tensor(h["m_dst"])
    assert torch.equal(cat.cpu(), torch.cat([H[src], H[dst], M], dim=1))
    refs = [torch.zeros(G.N, A, dtype=dt).index_add_(0, src, dcat.to(dt)[:, :A]).index_add_(0, dst, dcat.to(dt)[:, A:2 * A])
            for dt in (torch.float64, torch.float32)]
    assert_sum("cat dh", dH, *refs)


def test_mulsum_forward_backward():
    g = graph("dense")
    G, h = g.G, g.h
    Cc = 48
    gen = torch.Generator().manual_seed(7)
    M, Rb, dout = rnd(gen, G.Em, Cc), rnd(gen, G.Em, Cc), rnd(gen, G.N, Cc)
    out, dM, dR = nan_dev(G.N, Cc), nan_dev(G.Em, Cc), nan_dev(G.Em, Cc)
    check(lib().nq_gn_mulsum_forward(C.byref(G.main), D(M), D(Rb), G.N, Cc, P(out), st()))
    check(lib().nq_gn_mulsum_backward(C.byref(G.main), D(M), D(Rb), D(dout), Cc, P(dM), P(dR), st()))
    dst = torch.as_tensor(h["m_dst"])
    ref = {dt: (torch.zeros(G.N, Cc, dtype=dt).index_add_(0, dst, M.to(dt) * Rb.to(dt)), dout.to(dt)[dst] * Rb.to(dt), dout.to(dt)[dst] * M.to(dt))
           for dt in (torch.float64, torch.float32)}
    for k, (name, got) in enumerate((("mulsum out", out), ("mulsum dm", dM), ("mulsum dr", dR))):
        assert_sum(name, got, ref[torch.float64][k], ref[torch.float32][k])


@pytest.mark.parametrize("coupled", [0, 1])
def test_forces_forward_backward(coupled):
    g = graph("dense")
    G, h = g.G, g.h
    gen = torch.Generator().manual_seed(8 + coupled)
    F, dout = rnd(gen, G.Em), rnd(gen, G.N, 3)
    out, dF = nan_dev(G.N, 3), nan_dev(G.Em)
    check(lib().nq_gn_forces_forward(C.byref(G.main), P(G.t["m_rev"]), D(F), G.N, coupled, P(out), st()))
    check(lib().nq_gn_forces_backward(C.byref(G.main), P(G.t["m_rev"]), D(dout), coupled, P(dF), st()))
    dst, rev = torch.as_tensor(h["m_dst"]), torch.as_tensor(h["m_rev"])
    refs = {}
    for dt in (torch.float64, torch.float32):
        v, f, d = g.vm.to(dt), F.to(dt), dout.to(dt)
        fc = (f + f[rev]) / 2 if coupled else f
        s = (d[dst] * v).sum(-1)
        refs[dt] = (torch.zeros(G.N, 3, dtype=dt).index_add_(0, dst, fc[:, None] * v), (s + s[rev]) / 2 if coupled else s)
    assert_sum("forces", out, refs[torch.float64][0], refs[torch.float32][0])
    assert_sum("forces dF", dF, refs[torch.float64][1], refs[torch.float32][1])


def test_embed_grad_with_absent_elements():
    N, T, Cc = 301, 12, 40
    gen = torch.Generator().manual_seed(9)
    z = torch.tensor(np.random.default_rng(9).choice([1, 2, 6, 7, 9], size=N), dtype=torch.int32)       # elements 3-5, 8, 10-12 never occur
    gr = rnd(gen, N, Cc)
    dW = nan_dev(T, Cc)
    check(lib().nq_gn_embed_grad(D(z), D(gr), N, T, Cc, P(dW), st()))
    refs = [torch.zeros(T, Cc, dtype=dt).index_add_(0, z.long() - 1, gr.to(dt)) for dt in (torch.float64, torch.float32)]
    assert_sum("embed dW", dW, *refs)
    absent = torch.ones(T, dtype=torch.bool)
    absent[torch.unique(z.long() - 1)] = False
    assert torch.equal(dW.cpu()[absent], torch.zeros(int(absent.sum()), Cc))


@pytest.mark.parametrize("with_order,with_y", [(True, False), (True, True), (False, False), (False, True)])
def test_segment_sum(with_order, with_y):
    rng = np.random.default_rng(10)
    Nseg, rows_n, Cc = 57, 400, 24
    lens = rng.integers(0, 12, size=Nseg)
    lens[[0, 5, 6, Nseg - 1]] = 0                                                # empty segments, first and last included
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    Q = int(ptr[-1])
    if with_order:
        order = rng.integers(0, rows_n, size=Q).astype(np.int32)
        order[rng.random(Q) < 0.25] = -1                                         # skipped entries
    else:
        rows_n = Q
        order = np.arange(Q, dtype=np.int32)
    gen = torch.Generator().manual_seed(11)
    rows, y = rnd(gen, rows_n, Cc), rnd(gen, rows_n, Cc)
    out = nan_dev(Nseg, Cc)
    check(lib().nq_gn_segment_sum(D(rows), D(y) if with_y else None, D(torch.tensor(order)) if with_order else None,
                                  D(torch.tensor(ptr)), Nseg, Cc, P(out), st()))
    keep = order >= 0
    seg = torch.as_tensor(np.repeat(np.arange(Nseg), lens)[keep])
    r = torch.as_tensor(order[keep].astype(np.int64))
    refs = [torch.zeros(Nseg, Cc, dtype=dt).index_add_(0, seg, rows.to(dt)[r] * (y.to(dt)[r] if with_y else 1)) for dt in (torch.float64, torch.float32)]
    assert_sum("segment_sum", out, *refs)
    assert torch.equal(out.cpu()[torch.as_tensor(lens == 0)], torch.zeros(int((lens == 0).sum()), Cc))


def test_gather_with_and_without_y():
    rng = np.random.default_rng(12)
    n, Pn, Cc = 90, 1001, 33
    idx = torch.tensor(rng.integers(0, n, size=Pn), dtype=torch.int32)
    gen = torch.Generator().manual_seed(12)
    x, y = rnd(gen, n, Cc), rnd(gen, Pn, Cc)
    out, outy = nan_dev(Pn, Cc), nan_dev(Pn, Cc)
    check(lib().nq_gn_gather(D(x), D(idx), None, Pn, Cc, P(out), st()))
    check(lib().nq_gn_gather(D(x), D(idx), D(y), Pn, Cc, P(outy), st()))
    assert torch.equal(out.cpu(), x[idx.long()])
    assert torch.equal(outy.cpu(), x[idx.long()] * y)                             # one float32 product per element: exact


@pytest.mark.parametrize("nr,cutoff", [(2, 5.0), (8, 6.0), (24, 5.0), (128, 12.0)])
def test_radial_basis(nr, cutoff):
    rng = np.random.default_rng(nr)
    d = np.concatenate([[0.0, cutoff * (1 - 2.0 ** -20), np.nextafter(np.float32(cutoff), np.float32(0)), cutoff, cutoff * 1.5],
                        rng.uniform(0.0, cutoff * 1.1, size=3000)]).astype(np.float32)
    geom = torch.zeros(len(d), 4)
    geom[:, 3] = torch.tensor(d)
    offset = torch.linspace(0.0, 1.0, nr)
    out = nan_dev(len(d), nr)
    check(lib().nq_gn_radial_basis(D(geom), len(d), nr, D(offset), cutoff, 5.0, 1.25, P(out), st()))
    refs = [R.radial_basis(torch.tensor(d).to(dt), cutoff, offset.to(dt), 5.0, 1.25) for dt in (torch.float64, torch.float32)]
    assert_sum("rbf", out, *refs)
    assert torch.equal(out.cpu()[3:5], torch.zeros(2, nr))                      # d = cutoff and d > cutoff: the envelope is zero


def test_elementwise_ssilu_backward_lincomb_mul():
    n = 100003
    gen = torch.Generator().manual_seed(13)
    z, g, a, b = rnd(gen, n) * 4, rnd(gen, n), rnd(gen, n), rnd(gen, n)
    zd, gd, ad, bd = z.to(DEV), g.to(DEV), a.to(DEV), b.to(DEV)
    out = nan_dev(n)
    check(lib().nq_gn_ssilu_backward(P(zd), P(gd), 0.7, n, P(out), st()))

    def dssilu(z, g):
        s = torch.sigmoid(z)
        return 0.7 / 0.6 * g * s * (1 + z * (1 - s))
    assert_sum("ssilu_backward", out, dssilu(z.double(), g.double()), dssilu(z, g))
    for beta_b in (True, False):
        out = nan_dev(n)
        check(lib().nq_gn_lincomb(P(ad), P(bd) if beta_b else None, -0.3, 1.7, n, P(out), st()))
        refs = [-0.3 * a.to(dt) + (1.7 * b.to(dt) if beta_b else 0) for dt in (torch.float64, torch.float32)]
        assert_sum("lincomb", out, *refs)
    out = nan_dev(n)
    check(lib().nq_gn_mul(P(ad), P(bd), n, P(out), st()))
    assert torch.equal(out.cpu(), a * b)


# ---- one model at a non-default width -------------------------------------------------------------------------------------------------------------------
def test_model_gradients_quad_in_48_match_float64_oracle():
    """emb_size_quad_in = 48 (quadruplet adjoint with 5 rows per pass) and emb_size_trip_in = 40 on a molecule whose main in-degrees reach 43 (a second
    32-row block of the adjoint): the GPU loss gradients against oracle/gemnet_ref.forward in float64 on the CPU (autograd)."""
    from nabladft_amd.gemnet_oc import GemNetOC
    from oracle.gemnet_params import make_state
    from tests.test_gemnet_gpu import SMALL
    cfg = dict(SMALL, emb_size_quad_in=48, emb_size_trip_in=40, cutoff=6.0, cutoff_qint=4.0, cutoff_aeaint=4.5, cutoff_aint=6.5, max_neighbors=40,
               max_neighbors_qint=3, max_neighbors_aeaint=4)
    sizes = [44, 12]
    pos = cloud(7, sizes, 1.4)
    rng = np.random.default_rng(7)
    z = rng.choice([1, 6, 7, 8], size=len(pos))
    y, ft = rng.normal(size=len(sizes)), rng.normal(size=(len(pos), 3))
    torch.manual_seed(0)
    net = GemNetOC(**cfg)
    names = [k for k, _ in net.named_parameters()]
    net.load_state_dict(make_state([(k, tuple(v.shape)) for k, v in net.named_parameters()], 5, True), strict=False)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(DEV)

    class Data:
        pass
    data = Data()
    data.pos, data.z = torch.tensor(pos, device=DEV), torch.tensor(z, device=DEV)
    data.batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    E, F = net(data)
    R.loss(E, F, torch.tensor(y, device=DEV, dtype=torch.float32), torch.tensor(ft, device=DEV, dtype=torch.float32)).backward()
    G = R.build_graphs(torch.tensor(pos), sizes, cfg)
    assert np.bincount(G["main"][1]).max() > 32
    train = [k for k in names if dict(net.named_parameters())[k].requires_grad]
    refs = {}
    for dt in (torch.float64, torch.float32):
        Pd = {k: v.to(dt) for k, v in state.items()}
        for k in Pd:
            if k.endswith("rbf.offset"):
                Pd[k] = torch.linspace(0.0, 1.0, Pd[k].numel(), dtype=dt)
        for k in train:
            Pd[k].requires_grad_(True)
        shared = {"out_blocks.%d.seq_energy_pre" % i: "out_blocks.%d.layers" % i for i in range(cfg["num_blocks"] + 1)}
        for k in list(Pd):                                                       # the state_dict aliases must be the SAME tensors for the gradients to add up
            for a, b in shared.items():
                if k.startswith(a + "."):
                    Pd[k] = Pd[b + k[len(a):]]
        Eo, Fo = R.forward(Pd, cfg, torch.tensor(pos).to(dt), torch.tensor(z), sizes)
        R.loss(Eo, Fo, torch.tensor(y, dtype=dt), torch.tensor(ft, dtype=dt)).backward()
        refs[dt] = {k: (Pd[k].grad.double() if Pd[k].grad is not None else torch.zeros(Pd[k].shape, dtype=torch.float64)) for k in train}
    params = dict(net.named_parameters())
    worst = 0.0
    for k in train:
        ref64, ref32 = refs[torch.float64][k].numpy(), refs[torch.float32][k].numpy()
        gp = params[k].grad
        got = np.zeros_like(ref64) if gp is None else gp.double().cpu().numpy()
        assert not np.isnan(got).any(), k
        scale = max(np.abs(ref64).max(), 1e-30)
        err, own = np.abs(got - ref64).max() / scale, np.abs(ref32 - ref64).max() / scale
        worst = max(worst, err)
        assert err < max(5e-5, 3 * own), (k, err, own)                          # the bound of test_gemnet_gpu.py::test_gradients_small_match_reference
    assert worst > 0.0
