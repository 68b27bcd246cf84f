"""The eSCN / EquiformerV2 kernels of csrc/escn.hip one by one through the C ABI against float64 restatements of the same operation, built from the
kernel's own float32 inputs (the J matrices as float32, the rotation matrices and Wigner rows the kernel read, the device CSR arrays, all promoted):
oracle/escn_ref.py gives the radius graph, the frames, the Wigner matrices and the S2 grids.  Every output buffer starts as NaN, so an element a kernel
never writes fails the comparison; with accumulate = 1 the output starts as random finite values that the restatement adds.

Bounds (the convention of test_gemnet_ops_gpu.py): copies / selections / index lists are exact; every summing kernel must stay within max(3 x the error
of the same formula evaluated in float32 on the CPU, 2e-6) of the float64 value AND below 1e-5, both array-relative (max |a - b| / max |b|).  Every
summing kernel runs twice and must give bitwise equal results.

Branches and the tests that reach them:
  k_es_graph cap K reached in the second 64-atom chunk: test_graph[80]; k_es_scan carry across 1024-thread passes: test_graph (1108 atoms)
  k_es_frames tie-breaks: test_frames; k_es_angles / k_es_wigner at beta = 0, pi and near the pole: test_wigner (also against a least-squares D)
  k_rowop_fwd / _tr (accumulate, index, strided rows): test_rowop_lds; segmented I side / S side, nseg 1..8: test_rowop_blocks
  k_rowmm TW 1..6, CS 32 / 64 / 128, LDS > 64 kB, persistent grid loop: test_rowmm (each case asserts the plan it reaches)
  k_s2act CS = 64 (C = 64, 192; odd item counts), MT 1 / 2 / 3 (G = 20, 32 / 33, 40, 42, 64 / 70, 96): test_s2act
  k_es_rot_fwd / _tr (C > 256, C % 64 != 0, two slots, ptr + order, ptr NULL, coef_scale, empty atoms, m = 0 only): test_rotate_and_rotate_back"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from oracle import e3nn_mini as M  # noqa: E402
from oracle import escn_ref as R  # noqa: E402
from tests.helpers import (DEV, D, P, _lib, _release_copies, assert_sum, check, host_i32, host_ptrs, i32, lib, nan_dev, rejected, rnd,  # noqa: E402,F401
                           st, twice)                                  # (_release_copies: autouse)


def m_primary(lmax, mmax):
    """(l, m) of the reduced coefficients in the m-primary order of CoefficientMapping and the rows of its m-blocks (m = 0, +1, -1, +2, -2, ...)."""
    order, rows = [(l, 0) for l in range(lmax + 1)], [lmax + 1]
    for m in range(1, mmax + 1):
        order += [(l, m) for l in range(m, lmax + 1)] + [(l, -m) for l in range(m, lmax + 1)]
        rows += [lmax - m + 1] * 2
    return order, rows


def grid_red(lmax, mmax):
    """The (to_grid, from_grid) matrices [G, n_red] of eSCN's SO3_Grid(lmax, mmax) on the reduced coefficients, columns in m-primary order (float32)."""
    T, F = R.s2(lmax, mmax, torch.float64)
    order, _ = m_primary(lmax, mmax)
    cols = [l * l + l + m for l, m in order]
    return T[:, cols].float().contiguous(), F[:, cols].float().contiguous()


# ---- radius graph -------------------------------------------------------------------------------------------------------------------------------------
def graph_batch():
    """Molecules of 1 (an isolated atom), 2, 63, 64, 65 and 130 atoms, a 3-atom molecule with one pair exactly at the cutoff (2.0) in float32 and one a
    float32 ulp inside it, and 12 more of 65 atoms: 1108 atoms, so the exclusive scan carries across its 1024-thread passes."""
    rng = np.random.default_rng(21)
    sizes, parts = [], []
    for n, side in [(1, 1.0), (2, 1.0), (63, 2.6), (64, 2.6), (65, 2.6), (130, 1.6)] + [(65, 3.0)] * 12:
        parts.append(rng.uniform(0.0, side, size=(n, 3)) + rng.normal(size=3) * 5.0)
        sizes.append(n)
    edge = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, float(np.nextafter(np.float32(2.0), np.float32(0.0))), 0.0]])
    parts.insert(3, edge)
    sizes.insert(3, 3)
    return np.concatenate(parts).astype(np.float32), sizes


_GB = {}


@pytest.mark.parametrize("K", [1, 5, 30, 80, 1 << 20])
def test_graph(K):
    if not _GB:
        _GB["pos"], _GB["sizes"] = graph_batch()
    pos, sizes = _GB["pos"], _GB["sizes"]
    N, cutoff = len(pos), 2.0
    mol_ptr = np.concatenate([[0], np.cumsum(sizes)])
    atom_mol = np.repeat(np.arange(len(sizes)), sizes)
    posd, mpd, amd = D(torch.tensor(pos)), D(i32(mol_ptr)), D(i32(atom_mol))
    deg, ptr = torch.full((N,), -1, dtype=torch.int32, device=DEV), torch.full((N + 1,), -1, dtype=torch.int32, device=DEV)
    e_host = C.c_int32(-1)
    check(lib().nq_es_graph_count(posd, mpd, amd, N, cutoff, K, P(deg), P(ptr), C.byref(e_host), st()))
    E = int(e_host.value)
    src, dst = torch.full((E,), -1, dtype=torch.int32, device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV)
    geom = nan_dev(E, 4)
    check(lib().nq_es_graph_fill(posd, mpd, amd, N, cutoff, K, P(ptr), P(src), P(dst), P(geom), st()))
    rs, rd = R.radius_graph(torch.tensor(pos), sizes, cutoff, K)
    rdeg = np.bincount(rd.numpy(), minlength=N)
    assert E == len(rs)
    assert np.array_equal(deg.cpu().numpy(), rdeg)
    assert np.array_equal(ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(rdeg)]))
    assert np.array_equal(src.cpu().numpy(), rs.numpy()) and np.array_equal(dst.cpu().numpy(), rd.numpy())
    g = geom.cpu()
    p = torch.tensor(pos)
    assert torch.equal(g[:, :3], p[rs] - p[rd])                                  # edge_distance_vec = pos[source] - pos[target], one float32 subtraction
    # |.| within 1 ulp of the float64 norm, or no further from it than the same formula in float32 on the CPU (torch.norm, which the kernel mirrors:
    # its float32 sum of squares misses by up to 1.14 ulp on 80 of the 49630 edges of this batch)
    n64 = (p[rs] - p[rd]).double().norm(dim=1).numpy()
    own = np.abs((p[rs] - p[rd]).norm(dim=1).double().numpy() - n64)
    assert (np.abs(g[:, 3].double().numpy() - n64) <= np.maximum(np.spacing(n64.astype(np.float32)).astype(np.float64), own)).all()
    # the cases the batch is built for
    a = int(mol_ptr[3])
    assert rdeg[0] == 0 and list(rs[rd == a].numpy()) == [a + 2] and rdeg[a + 1] == 0     # isolated atom; the pair at exactly the cutoff is excluded
    big = int(mol_ptr[sizes.index(130)])
    inside = np.array([int(((rd == i) & (rs < big + 64)).sum()) for i in range(big, big + 130)])
    if K == 80:
        assert ((rdeg[big:big + 130] == 80) & (inside < 80)).any()                # the cap is reached inside the second 64-atom chunk
    if K == 1 << 20:
        assert rdeg.max() > 80 and N > 1024


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------------
def _signs(v):
    s = np.array([[a, b, c] for a in (1, -1) for b in (1, -1) for c in (1, -1)], dtype=np.float32)
    return (np.asarray(v, dtype=np.float32)[None] * s)


def frame_edges():
    rng = np.random.default_rng(3)
    ties = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    tie = np.concatenate([_signs(t) * f for t in ties for f in (1.0, 0.37)])
    rand = rng.normal(size=(500, 3)).astype(np.float32) * 2.0
    axis = np.concatenate([np.eye(3, dtype=np.float32) * f for f in (0.5, 1.7, -2.3)])
    return np.concatenate([tie, axis, rand]).astype(np.float32)


def test_frames():
    v = torch.tensor(frame_edges())
    geom = torch.cat([v, v.norm(dim=1, keepdim=True)], dim=1)                   # |.| in float32, as the graph kernel writes it
    E = len(v)
    rot = nan_dev(E, 9)
    check(lib().nq_es_frames(D(geom), E, P(rot), st()))
    assert_sum("frames", rot, R.frames(v.double()).reshape(E, 9), R.frames(v).reshape(E, 9))


# ---- Wigner rows --------------------------------------------------------------------------------------------------------------------------------------
def lattice():
    pts = [(0, 0, 0)] + [(x, 0, 0) for x in (-2, -1, 1, 2)] + [(0, y, 0) for y in (-1, 1, 2)] + [(0, 0, z) for z in (-2, -1, 1)]
    return np.array(pts, dtype=np.float32)


def wigner_rots():
    """(rot [E, 3, 3] float32, mask of the polar / near-polar / lattice edges): random frames, edges exactly along +-y (beta = 0 and pi, alpha =
    atan2(0, 0)), edges 1e-3 and 1e-6 rad off the pole in several azimuths, and every edge of the axis lattice."""
    rng = np.random.default_rng(5)
    rand = rng.normal(size=(120, 3))
    pole = [(0.0, s, 0.0) for s in (1.0, -1.0, 2.5, -0.7)]
    near = [(math.sin(t) * math.cos(f) * s, math.cos(t) * s, math.sin(t) * math.sin(f) * s) for t in (1e-3, 1e-6) for f in (0.0, 1.1, 2.9, -2.0)
            for s in (1.0, -1.0)]
    L = lattice()
    i, j = np.nonzero(~np.eye(len(L), dtype=bool))
    lat = (L[j] - L[i]).astype(np.float64)
    v = np.concatenate([rand, np.array(pole), np.array(near), lat])
    rot = R.frames(torch.tensor(v, dtype=torch.float64)).float().contiguous()
    special = torch.zeros(len(v), dtype=torch.bool)
    special[len(rand):] = True
    return rot, special


def wigner_lstsq(rot, lmax):
    """The Wigner blocks without Euler angles: D_l solves Y_l(R v) = D_l Y_l(v) (the relation the oracle's D satisfies) by least squares over 64 random
    directions, R the orthonormalised float64 rotation."""
    U, _, Vh = torch.linalg.svd(rot.double())
    Ro = U @ Vh
    v = torch.nn.functional.normalize(torch.randn(64, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64), dim=-1)
    E, nf = len(rot), (lmax + 1) ** 2
    Dm = torch.zeros(E, nf, nf, dtype=torch.float64)
    for l in range(lmax + 1):
        Yv = M.spherical_harmonics([l], v, True)
        Yr = M.spherical_harmonics([l], torch.einsum("eij,pj->epi", Ro, v), True)
        Dm[:, l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = torch.linalg.lstsq(Yv.expand(E, -1, -1), Yr).solution.transpose(1, 2)
    return Dm


def wigner_call(rot, lmax, mmax, J32):
    order, _ = m_primary(lmax, mmax)
    red_l, red_row = [l for l, _ in order], [l + m for l, m in order]
    n_red, nf, E = len(order), (lmax + 1) ** 2, len(rot)
    Jall = torch.cat([j.reshape(-1) for j in J32])
    Joff = np.cumsum([0] + [j.numel() for j in J32])[:-1]
    args = (D(rot), E, D(Jall), D(i32(Joff)), D(i32(red_l)), D(i32(red_row)), n_red, nf, lmax)

    def call():
        scratch = torch.full((3 * E,), float("nan"), dtype=torch.float64, device=DEV)
        W = nan_dev(E, n_red * nf)
        check(lib().nq_es_wigner(*args, P(scratch), P(W), st()))
        return (W,)
    return twice(call)[0].reshape(E, n_red, nf), [l * l + r for l, r in zip(red_l, red_row)]


@pytest.mark.parametrize("lmax,mmax", [(l, m) for l in range(7) for m in sorted({0, 1, 2, l}) if m <= l])
def test_wigner(lmax, mmax):
    rot, special = wigner_rots()
    J32 = [j.float() for j in R.j_matrices(lmax)]
    W, rows = wigner_call(rot, lmax, mmax, J32)
    J64 = [j.double() for j in J32]
    ref64 = R.wigner(rot.double(), lmax, J64)[:, rows]
    ref32 = R.wigner(rot, lmax, J32)[:, rows]
    assert_sum(f"wigner l{lmax} m{mmax}", W, ref64, ref32)
    # polar / near-polar / lattice edges against D from the rotation itself (no Euler angles: checks the alpha = atan2(0, 0) handling independently)
    Dl = wigner_lstsq(rot[special], lmax)[:, rows]
    assert_sum(f"wigner l{lmax} m{mmax} vs lstsq", W[special], Dl, ref32[special])


def test_wigner_rejects_lmax_7_and_misaligned_scratch():
    rot, _ = wigner_rots()
    E = len(rot)
    J = torch.zeros(64 * 13, device=DEV)
    idx = torch.zeros(64, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(3 * E + 1, dtype=torch.float64, device=DEV)
    W = nan_dev(E, 64)
    rd = D(rot)
    rejected(lambda: lib().nq_es_wigner(rd, E, P(J), P(idx), P(idx), P(idx), 1, 64, 7, P(scratch), P(W), st()), W)
    W = nan_dev(E, 16)
    rejected(lambda: lib().nq_es_wigner(rd, E, P(J), P(idx), P(idx), P(idx), 1, 16, 3, C.c_void_p(scratch.data_ptr() + 4), P(W), st()), W)


# ---- smearing -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 50, 401])
def test_smearing(K):
    gen = torch.Generator().manual_seed(K)
    E = 1537
    geom = rnd(gen, E, 4)
    geom[:, 3] = torch.rand(E, generator=gen) * 6.5
    geom[:4, 3] = torch.tensor([0.0, 6.0, 3.0, 1e-3])
    offset = torch.linspace(0.0, 6.0, K) if K > 1 else torch.tensor([0.75])
    coeff = float(np.float32(-0.5 / (2.0 * (6.0 / max(K - 1, 1))) ** 2))
    out = nan_dev(E, K)
    check(lib().nq_es_smearing(D(geom), E, K, D(offset), coeff, P(out), st()))
    refs = [torch.exp(coeff * (geom[:, 3:4].to(dt) - offset.to(dt)[None]) ** 2) for dt in (torch.float64, torch.float32)]
    assert_sum("smearing", out, *refs)


# ---- row operators ------------------------------------------------------------------------------------------------------------------------------------
def rowop_ref(Rm, X, idx, I, NSS, Cc, transpose, dt):
    """out[o] = R_o X_row(o) (forward, R_o [I, NSS]) or R_o^T X_row(o) (transpose); Rm [1 or n, I * NSS], X rows [., >= K * C]."""
    K = I if transpose else NSS
    Xr = X.to(dt) if idx is None else X.to(dt)[idx.long()]
    Xr = Xr[:, :K * Cc].reshape(len(Xr), K, Cc)
    A = Rm.to(dt).reshape(-1, I, NSS)
    return torch.matmul(A.transpose(1, 2) if transpose else A, Xr).reshape(len(Xr), -1)


def rowmm_plan(I, NSS, Cc, transpose):
    """Mirror of rowmm_plan (csrc/escn.hip) for a shared matrix: (tiles per wavefront TW, channel slice CS, LDS bytes), or None."""
    if Cc % 32:
        return None
    Mr, K = (NSS, I) if transpose else (I, NSS)
    MT, Kp = (Mr + 31) // 32, (K + 1) & ~1
    cs = 128 if Cc % 128 == 0 else (64 if Cc % 64 == 0 else 32)
    while cs > 32 and (MT * (cs // 32) + 3) // 4 > 6:
        cs //= 2
    if (MT * (cs // 32) + 3) // 4 > 6:
        return None
    lds = 4 * (((MT * 32 * (Kp + 1) + 3) & ~3) + max(Kp, MT * 32) * cs)
    return ((MT * (cs // 32) + 3) // 4, cs, lds) if lds <= 150 * 1024 else None


# LDS path: per-row matrices (r_stride = I * NSS) and shared matrices with C % 32 != 0.  (per_row, I, NSS, C)
LDS_SHAPES = [(True, 29, 49, 16), (True, 9, 16, 1), (False, 70, 29, 48), (False, 20, 4, 1), (False, 14, 9, 100)]


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("per_row,I,NSS,Cc", LDS_SHAPES)
def test_rowop_lds(per_row, I, NSS, Cc, with_index, accumulate, transpose):
    n, n_src = 37, 23
    Mr, K = (NSS, I) if transpose else (I, NSS)
    assert per_row or rowmm_plan(I, NSS, Cc, transpose) is None
    gen = torch.Generator().manual_seed(I * 100 + NSS + Cc)
    Rm = rnd(gen, n if per_row else 1, I * NSS)
    xs, os_ = K * Cc + 5, Mr * Cc + 3                                             # strided rows in and out
    X = rnd(gen, n_src if with_index else n, xs)
    idx = torch.tensor(np.random.default_rng(Cc).integers(0, n_src, size=n), dtype=torch.int32) if with_index else None
    out0 = rnd(gen, n, os_) if accumulate else torch.full((n, os_), float("nan"))
    args = (D(Rm), I * NSS if per_row else 0, D(X), xs, None if idx is None else D(idx))

    def call():
        out = out0.to(DEV)
        check(lib().nq_rowop(*args, P(out), os_, n, I, NSS, Cc, transpose, accumulate, st()))
        return (out,)
    out = twice(call)[0]
    refs = [rowop_ref(Rm, X, idx, I, NSS, Cc, transpose, dt) + (out0[:, :Mr * Cc].to(dt) if accumulate else 0) for dt in (torch.float64, torch.float32)]
    assert_sum("rowop", out[:, :Mr * Cc], *refs)
    assert torch.equal(out[:, Mr * Cc:].cpu(), out0[:, Mr * Cc:]) or (not accumulate and torch.isnan(out[:, Mr * Cc:]).all())


# matrix-core path: (name, R source, transpose, C, n, index, expected (TW, CS)); the real S2 grids of (6,2), (6,6), (3,2) among them
RMM_CASES = [
    ("to_grid62-persistent", "T62", 0, 128, 3001, False, (3, 128)),
    ("from_grid62", "F62", 1, 128, 37, False, (1, 128)),
    ("to_grid66-lds101k", "T66", 0, 128, 301, False, (4, 64)),
    ("from_grid66-lds105k", "F66", 1, 64, 37, False, (1, 64)),
    ("to_grid66-c32", "T66", 0, 32, 37, False, (2, 32)),
    ("to_grid32-index", "T32", 0, 64, 41, True, (1, 64)),
    ("from_grid32-c32", "F32", 1, 32, 37, False, (1, 32)),
    ("rand150x9-tw5", (150, 9), 0, 256, 19, False, (5, 128)),
    ("rand180x49-tw6", (180, 49), 0, 128, 23, False, (6, 128)),
    ("rand7x20-tr-tw2", (7, 40), 1, 256, 21, True, (2, 128)),
    ("rand20x7-k7", (20, 7), 0, 96, 33, False, (1, 32)),
    ("rand96x33-tw3", (96, 33), 0, 128, 17, False, (3, 128)),
]


def _matrix(src, gen):
    if isinstance(src, tuple):
        return rnd(gen, *src) * 0.3
    lm = {"62": (6, 2), "66": (6, 6), "32": (3, 2)}[src[1:]]
    T, F = grid_red(*lm)
    return T if src[0] == "T" else F


@pytest.mark.parametrize("name,src,transpose,Cc,n,with_index,expect", RMM_CASES, ids=[c[0] for c in RMM_CASES])
def test_rowmm(name, src, transpose, Cc, n, with_index, expect):
    gen = torch.Generator().manual_seed(len(name) * 7 + Cc)
    Rm = _matrix(src, gen).contiguous()
    I, NSS = Rm.shape
    plan = rowmm_plan(I, NSS, Cc, transpose)
    assert plan is not None and plan[:2] == expect, plan
    if "lds10" in name:
        assert plan[2] > 64 * 1024
    Mr, K = (NSS, I) if transpose else (I, NSS)
    n_src = 29 if with_index else n
    X = rnd(gen, n_src, K * Cc)
    idx = torch.tensor(np.random.default_rng(n).integers(0, n_src, size=n), dtype=torch.int32) if with_index else None
    args = (D(Rm), 0, D(X), K * Cc, None if idx is None else D(idx))

    def call():
        out = nan_dev(n, Mr * Cc)
        check(lib().nq_rowop(*args, P(out), Mr * Cc, n, I, NSS, Cc, transpose, 0, st()))
        return (out,)
    out = twice(call)[0]
    assert_sum("rowmm", out, *[rowop_ref(Rm, X, idx, I, NSS, Cc, transpose, dt) for dt in (torch.float64, torch.float32)])


def test_rowop_rejects_over_64k_lds():
    n, I, NSS, Cc = 2, 64, 64, 256                                               # per-row matrices: 4 (64 * 64 + 64 * 256) = 80 kB
    Rm, X = torch.zeros(n, I * NSS, device=DEV), torch.zeros(n, NSS * Cc, device=DEV)
    out = nan_dev(n, I * Cc)
    rejected(lambda: lib().nq_rowop(P(Rm), I * NSS, P(X), NSS * Cc, None, P(out), I * Cc, n, I, NSS, Cc, 0, 0, st()), out)


# per-block tensors on one side: (name, R shape or grid, per_row, transpose, seg_side, segs, C, accumulate, index)
BLOCK_CASES = [
    ("to_grid62-from-blocks", "T62", False, 0, 1, [7, 6, 6, 5, 5], 128, 0, False),
    ("from_grid62-into-blocks", "F62", False, 1, 1, [7, 6, 6, 5, 5], 128, 0, False),
    ("rot-into-blocks-index", (29, 49), True, 0, 0, [7, 6, 6, 5, 5], 16, 0, True),
    ("rot-tr-from-blocks-acc", (29, 49), True, 1, 0, [7, 6, 6, 5, 5], 16, 1, False),
    ("mfma-into-8-blocks", (29, 40), False, 0, 0, [4, 4, 4, 4, 4, 3, 3, 3], 64, 0, True),
    ("lds-tr-into-1-block-acc", (20, 13), False, 1, 1, [13], 48, 1, False),
    ("lds-from-8-blocks", (20, 29), True, 0, 1, [1, 2, 3, 4, 5, 6, 7, 1], 8, 0, False),
    ("mfma-tr-from-blocks", (14, 40), False, 1, 0, [4, 3, 3, 2, 2], 64, 0, False),
    ("lds-tr-into-3-blocks-acc", (9, 30), True, 1, 1, [10, 15, 5], 33, 1, True),
]


@pytest.mark.parametrize("name,src,per_row,transpose,seg_side,segs,Cc,accumulate,with_index", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_rowop_blocks(name, src, per_row, transpose, seg_side, segs, Cc, accumulate, with_index):
    n = 31
    gen = torch.Generator().manual_seed(len(name) + Cc)
    I, NSS = src if isinstance(src, tuple) else _matrix(src, gen).shape
    Rm = rnd(gen, n, I * NSS) if per_row else _matrix(src, gen).reshape(1, -1).contiguous()
    assert sum(segs) == (I if seg_side == 0 else NSS)
    mfma = not per_row and not accumulate and rowmm_plan(I, NSS, Cc, transpose) is not None
    assert mfma == ("mfma" in name or "grid" in name)
    Mr, K = (NSS, I) if transpose else (I, NSS)
    seg_in = (transpose != 0) == (seg_side == 0)
    n_src = 19 if with_index else n
    idx = torch.tensor(np.random.default_rng(3).integers(0, n_src, size=n), dtype=torch.int32) if with_index else None
    if seg_in:                                                                   # blocks are the input, x_or_out the plain output
        assert not with_index
        xb = [rnd(gen, n, r * Cc) for r in segs]
        X = torch.cat([b.reshape(n, r, Cc) for b, r in zip(xb, segs)], dim=1).reshape(n, -1)
        out0 = rnd(gen, n, Mr * Cc) if accumulate else torch.full((n, Mr * Cc), float("nan"))
        bd = [b.to(DEV) for b in xb]
        Rd = D(Rm)

        def call():
            out = out0.to(DEV)
            check(lib().nq_rowop_blocks(Rd, I * NSS if per_row else 0, P(out), Mr * Cc, None, seg_side, len(segs), host_i32(segs), host_ptrs(bd), n, I,
                                        NSS, Cc, transpose, accumulate, st()))
            return (out,)
        got = twice(call)[0]
    else:                                                                        # x_or_out is the plain input (gathered by index), the blocks the output
        X = rnd(gen, n_src, K * Cc)
        out0s = [rnd(gen, n, r * Cc) if accumulate else torch.full((n, r * Cc), float("nan")) for r in segs]
        out0 = torch.cat([b.reshape(n, r, Cc) for b, r in zip(out0s, segs)], dim=1).reshape(n, -1)
        Rd, Xd, Id = D(Rm), D(X), None if idx is None else D(idx)

        def call():
            outs = [b.to(DEV) for b in out0s]
            check(lib().nq_rowop_blocks(Rd, I * NSS if per_row else 0, Xd, K * Cc, Id, seg_side, len(segs), host_i32(segs), host_ptrs(outs), n, I, NSS, Cc,
                                        transpose, accumulate, st()))
            return tuple(outs)
        got = torch.cat([b.reshape(n, r, Cc) for b, r in zip(twice(call), segs)], dim=1).reshape(n, -1)
    refs = [rowop_ref(Rm, X, idx, I, NSS, Cc, transpose, dt) + (out0.to(dt) if accumulate else 0) for dt in (torch.float64, torch.float32)]
    assert_sum(f"rowop_blocks {name}", got, *refs)


# ---- fused S2 activation ------------------------------------------------------------------------------------------------------------------------------
def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def s2act_ref(T, F, x, dy, dt):
    """y[o][s'][c] = sum_g F[g][s'] silu(sum_s T[g][s] x[o][s][c]); backward (dy given): dx = T^T (silu'(T x) * (F dy))."""
    T, F, x = T.to(dt), F.to(dt), x.to(dt)
    g = torch.einsum("gs,nsc->ngc", T, x)
    if dy is None:
        return torch.einsum("gs,ngc->nsc", F, torch.nn.functional.silu(g))
    return torch.einsum("gs,ngc->nsc", T, dsilu(g) * torch.einsum("gs,nsc->ngc", F, dy.to(dt)))


# (name, grid (lmax, mmax) or (G, S), C, n, m-blocks); CS = 64 when C % 128 == 64 (two items per pass), MT = ceil(G / 32)
S2_CASES = [
    ("grid11-G20-C64", (1, 1), 64, 37, [2, 1, 1]),
    ("grid32-G40-C128", (3, 2), 128, 37, [4, 3, 3, 2, 2]),
    ("grid22-G42-C192", (2, 2), 192, 31, [3, 2, 2, 1, 1]),
    ("grid62-G70-C256", (6, 2), 256, 33, [7, 6, 6, 5, 5]),
    ("grid62-G70-C64", (6, 2), 64, 41, [7, 6, 6, 5, 5]),
    ("G32-S1-C64", (32, 1), 64, 45, [1]),
    ("G33-S32-C128", (33, 32), 128, 37, [4] * 8),
    ("G64-S29-C192", (64, 29), 192, 29, [7, 6, 6, 5, 5]),
    ("G96-S14-C256", (96, 14), 256, 17, [14]),
    ("G96-S32-C64", (96, 32), 64, 23, [1, 2, 3, 4, 5, 6, 7, 4]),
    ("G42-S29-C128", (42, 29), 128, 25, [10, 19]),
]


@pytest.mark.parametrize("backward", [0, 1])
@pytest.mark.parametrize("name,src,Cc,n,segs", S2_CASES, ids=[c[0] for c in S2_CASES])
def test_s2act(name, src, Cc, n, segs, backward):
    gen = torch.Generator().manual_seed(len(name) + Cc + backward)
    if name.startswith("grid"):
        T, F = grid_red(*src)
    else:
        G, S = src
        T, F = rnd(gen, G, S) * (1.5 / math.sqrt(S)), rnd(gen, G, S) * (1.0 / G)
    G, S = T.shape
    assert sum(segs) == S and S <= 32 and G <= 96 and Cc % 64 == 0
    xb = [rnd(gen, n, r * Cc) for r in segs]
    gb = [rnd(gen, n, r * Cc) for r in segs]
    cat = lambda bs: torch.cat([b.reshape(n, r, Cc) for b, r in zip(bs, segs)], dim=1)      # noqa: E731
    xd, gd = [b.to(DEV) for b in xb], [b.to(DEV) for b in gb]
    Td, Fd = D(T), D(F)

    def call():
        outs = [nan_dev(n, r * Cc) for r in segs]
        check(lib().nq_s2_activation_blocks(Td, Fd, G, S, Cc, n, len(segs), host_i32(segs), host_ptrs(xd), host_ptrs(gd) if backward else None,
                                            host_ptrs(outs), backward, st()))
        return tuple(outs)
    got = cat(twice(call))
    refs = [s2act_ref(T, F, cat(xb), cat(gb) if backward else None, dt) for dt in (torch.float64, torch.float32)]
    assert_sum(f"s2act {name} {'bwd' if backward else 'fwd'}", got, *refs)


def test_s2act_rejects_unfusable_shapes():
    n = 3
    for G, S, Cc in [(40, 14, 32), (40, 33, 64), (97, 14, 64)]:
        T = torch.zeros(G, S, device=DEV)
        xs = [torch.zeros(n, S * Cc, device=DEV)]
        outs = [nan_dev(n, S * Cc)]
        rejected(lambda: lib().nq_s2_activation_blocks(P(T), P(T), G, S, Cc, n, 1, host_i32([S]), host_ptrs(xs), None, host_ptrs(outs), 0, st()), *outs)


# ---- rotations ----------------------------------------------------------------------------------------------------------------------------------------
def rot_graph(N=23, E=97, seed=0):
    """Edges sorted by target (atoms 0, 5 and N - 1 have no in-edges; atom 3 has no out-edges)."""
    rng = np.random.default_rng(seed)
    targets = np.array([a for a in range(N) if a not in (0, 5, N - 1)])
    dst = np.sort(rng.choice(targets, size=E))
    src = rng.integers(0, N, size=E)
    src[src == 3] = 4
    return src, dst


def degree_mask(red_l, lmax):
    col_l = torch.tensor([l for l in range(lmax + 1) for _ in range(2 * l + 1)])
    return (torch.tensor(red_l)[:, None] == col_l[None]).to(torch.float64)


def rot_fwd_ref(W, mask, x, idx, nf, Cc, dt):
    Wm = W.to(dt) * mask.to(dt)
    xr = x.to(dt)[idx] if idx is not None else x.to(dt)
    return torch.bmm(Wm, xr[:, :nf * Cc].reshape(len(Wm), nf, Cc))                 # [E, n_red, C]


def rot_back_ref(W, mask, y, ptr, order, coef, n_out, dt):
    Wm = W.to(dt) * mask.to(dt)
    per_edge = torch.bmm(Wm.transpose(1, 2), y.to(dt))                            # [E, n_full, C]
    if ptr is None:
        out = per_edge
    else:
        seg = torch.repeat_interleave(torch.arange(n_out), torch.as_tensor(np.diff(ptr)))
        rows = torch.as_tensor(order, dtype=torch.long) if order is not None else torch.arange(int(ptr[-1]))
        out = torch.zeros(n_out, *per_edge.shape[1:], dtype=dt).index_add_(0, seg, per_edge[rows])
    return out * coef.to(dt)[None, :, None] if coef is not None else out


# (lmax, mmax, C): C > 256 loops over channels; C not a multiple of 64; mmax = 0 is the m = 0 block alone (n_red = lmax + 1)
ROT_CASES = [(0, 0, 1), (1, 1, 16), (2, 2, 64), (3, 2, 100), (4, 2, 256), (5, 2, 300), (6, 2, 16), (6, 6, 64), (6, 0, 300), (3, 0, 64), (6, 2, 257)]


@pytest.mark.parametrize("lmax,mmax,Cc", ROT_CASES)
def test_rotate_and_rotate_back(lmax, mmax, Cc):
    order_lm, segs = m_primary(lmax, mmax)
    if len(segs) > 8:                                                            # at most 8 blocks: the +m and -m rows share one
        segs = segs[:1] + [segs[k] + segs[k + 1] for k in range(1, len(segs), 2)]
    red_l = [l for l, _ in order_lm]
    n_red, nf = len(red_l), (lmax + 1) ** 2
    src, dst = rot_graph()
    N, E = 23, len(src)
    gen = torch.Generator().manual_seed(lmax * 1000 + Cc)
    W = rnd(gen, E, n_red, nf)                                                   # off-block entries are random too: the kernel must not read them
    mask = degree_mask(red_l, lmax)
    x = rnd(gen, N, nf * Cc)
    xe = rnd(gen, E, nf * Cc + 7)                                                # one row per edge, strided (no index)
    coef = rnd(gen, nf)
    Wd, xd, xed = D(W), D(x), D(xe)
    srcd, dstd = D(i32(src)), D(i32(dst))
    ws = n_red * nf
    cat = lambda bs, c0: torch.cat([b.reshape(E, r, -1)[:, :, c0:c0 + Cc] for b, r in zip(bs, segs)], dim=1)      # noqa: E731
    # forward: the two-slot concatenation (source rotation at c_off = 0, target rotation at c_off = C of c_stride = 2 C)

    def fwd2():
        blocks = [nan_dev(E, r * 2 * Cc) for r in segs]
        for c_off, idx in ((0, srcd), (Cc, dstd)):
            check(lib().nq_es_rotate(Wd, ws, xd, nf * Cc, idx, len(segs), host_i32(segs), host_ptrs(blocks), 2 * Cc, c_off, E, host_i32(red_l), n_red, lmax,
                                     Cc, st()))
        return tuple(blocks)
    blocks = twice(fwd2)
    for c0, idx in ((0, src), (Cc, dst)):
        refs = [rot_fwd_ref(W, mask, x, torch.as_tensor(idx), nf, Cc, dt) for dt in (torch.float64, torch.float32)]
        assert_sum(f"rotate slot {c0 // Cc}", cat([b.cpu() for b in blocks], c0), *refs)

    # forward without index, one slot
    def fwd1():
        bl = [nan_dev(E, r * Cc) for r in segs]
        check(lib().nq_es_rotate(Wd, ws, xed, nf * Cc + 7, None, len(segs), host_i32(segs), host_ptrs(bl), Cc, 0, E, host_i32(red_l), n_red, lmax, Cc, st()))
        return tuple(bl)
    refs = [rot_fwd_ref(W, mask, xe, None, nf, Cc, dt) for dt in (torch.float64, torch.float32)]
    assert_sum("rotate (no index)", cat([b.cpu() for b in twice(fwd1)], 0), *refs)

    # rotate_back: (a) summed over the out-edges of every source atom through ptr + order (a stable sort by source), slot 0
    y = [rnd(gen, E, r * 2 * Cc) for r in segs]
    yd = [b.to(DEV) for b in y]
    order = np.argsort(src, kind="stable")
    sptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))])
    dptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))])
    cases = [("by source, ptr + order", 0, sptr, order, None, N), ("by target, ptr, coef_scale", Cc, dptr, None, coef, N), ("per edge, ptr NULL", Cc, None, None, None, E)]
    for label, c_off, ptr, order_, cf, n_out in cases:
        args = (D(i32(ptr)) if ptr is not None else None, D(i32(order_)) if order_ is not None else None, D(cf) if cf is not None else None)

        def back():
            out = nan_dev(n_out, nf * Cc)
            check(lib().nq_es_rotate_back(Wd, ws, len(segs), host_i32(segs), host_ptrs(yd), 2 * Cc, c_off, *args, P(out), n_out, host_i32(red_l), n_red, lmax, Cc,
                                          st()))
            return (out,)
        got = twice(back)[0].cpu().reshape(n_out, nf, Cc)
        refs = [rot_back_ref(W, mask, cat(y, c_off), ptr, order_, cf, n_out, dt) for dt in (torch.float64, torch.float32)]
        assert_sum(f"rotate_back {label}", got, *refs)
        if ptr is not None:
            empty = torch.as_tensor(np.diff(ptr) == 0)
            assert empty.any() and torch.equal(got[empty], torch.zeros(int(empty.sum()), nf, Cc))       # atoms without edges: zeros
        if label.startswith("by source"):
            # adjoint identity on the kernel outputs: <rotate(x), y> = <x, rotate_back(y)> (slot 0 of the two-slot rotation gathered by source)
            lhs = float((cat([b.cpu() for b in blocks], 0).double() * cat(y, 0).double()).sum())
            rhs = float((x.double().reshape(N, nf, Cc) * got.double()).sum())
            scale = float(cat([b.cpu() for b in blocks], 0).double().norm() * cat(y, 0).double().norm())
            assert abs(lhs - rhs) <= 1e-6 * scale, (lhs, rhs, scale)


def test_rotate_rejects_bad_blocks_degrees_and_channel_slots():
    lmax, Cc = 3, 16
    order_lm, segs = m_primary(lmax, 2)
    red_l = [l for l, _ in order_lm]
    n_red, nf, E = len(red_l), 16, 5
    W, x = torch.zeros(E, n_red * nf, device=DEV), torch.zeros(E, nf * Cc, device=DEV)
    ptr = torch.arange(E + 1, dtype=torch.int32, device=DEV)
    bad = [("block rows", segs[:-1] + [segs[-1] + 1], red_l, Cc, 0),
           ("degree above lmax", segs, red_l[:-1] + [lmax + 1], Cc, 0),
           ("c_off + C > c_stride", segs, red_l, Cc, 1)]
    for _, rows, rl, cstride, coff in bad:
        blocks = [nan_dev(E, r * Cc + 8) for r in rows]
        rejected(lambda: lib().nq_es_rotate(P(W), n_red * nf, P(x), nf * Cc, None, len(rows), host_i32(rows), host_ptrs(blocks), cstride, coff, E, host_i32(rl),
                                            n_red, lmax, Cc, st()), *blocks)
        out = nan_dev(E, nf * Cc)
        rejected(lambda: lib().nq_es_rotate_back(P(W), n_red * nf, len(rows), host_i32(rows), host_ptrs(blocks), cstride, coff, P(ptr), None, None, P(out), E,
                                                 host_i32(rl), n_red, lmax, Cc, st()), out)
