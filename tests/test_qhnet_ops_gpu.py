"""The QHNet kernels of csrc/qhnet.hip and csrc/qhgen.hip one by one through the C ABI against float64 references that share no code with them:
oracle/qhnet_ref.py (tensor_product, invariants, expansion; its 3j tensors come from oracle/e3nn_mini.py), torch.autograd on the float64 evaluation for
every adjoint, and the small restatements of tests/cg_ref.py where the oracle has none.  The tensor-product kernels are called the way nabladft_amd/qhnet.py
calls them, with w_kernel[r, p, c] = path_constants(paths)[p] * w[r, p, c], and must reproduce qhnet_ref.tensor_product(paths, x1, x2, w): that pins the sign
folding and the normalisation together with the arithmetic.  Every output buffer starts as NaN.

Bounds (the convention of test_escn_ops_gpu.py): copies and gathers are exact; every summing kernel within max(3 x the error of the same formula in float32
on the CPU, 2e-6) of the float64 value AND below 1e-5, array-relative (assert_sum); every kernel runs twice with bitwise equal results.

The fused generator (k_qh_tp_gen) builds its weights from two bfloat16 pieces per operand, so it is compared twice: (1) with the reference fed with the
split2_mirror weights (cg_ref.py), inside assert_sum; (2) with the reference fed with the exact float64 weights, no further away than the distance between
the two references + the assert_sum allowance.  Measured (array-relative, y / worst of the four adjoints), on an MI355X:
    K 128, C 128, R 70: mirror reference vs exact reference 3.99e-06 / 8.00e-06; kernel vs exact reference 4.04e-06 / 8.01e-06
    K  32, C  16, R  1: 1.00e-05 / 8.60e-06; 1.00e-05 / 8.56e-06        K  64, C  32, R 31: 2.36e-06 / 7.53e-06; 2.33e-06 / 7.42e-06
    K 128, C  16, R 32: 9.99e-06 / 6.60e-06; 1.00e-05 / 6.68e-06        K  32, C 128, R 33: 7.12e-06 / 1.31e-05; 7.08e-06 / 1.34e-05
    K  64, C  16, R 70: 8.02e-06 / 4.57e-06; 8.06e-06 / 4.38e-06
  i.e. the two-piece weights cost 2e-6 .. 1.3e-5 at operator level (a numpy trial of the same arithmetic on normal inputs: 3.6e-6 .. 7.7e-6), and the kernel adds nothing visible to that.

Branches and the tests that reach them:
  k_qh_inv_fwd / _bwd lmax 0..4, second_from_owner 0 / 1, C = 1 / 32 / 100, an atom without rows, an atom bonded to its whole molecule: test_invariants
  k_qh_tp<0 / 1 / 2, uvu / uuu, forward / reverse, variant 0 / 1 / 2>, w2 NULL, idx_gy NULL / gather, partial last workgroup, repeated indices: test_tp;
      weight-slot order per path set: test_tp_weight_slots; dispatch checks: test_tp_rejects
  k_qh_pair_reduce every operand combination, empty row: test_pair_reduce
  k_qh_normcat / k_qh_gate forward and reverse, lmax 0..4, zero-norm block: test_normcat_and_gate
  k_qh_act both kinds, forward / reverse, the x > 20 branch of the softplus and the far tails: test_act
  k_qh_exp_fwd / _bwd second pass of the (l1, l2, u, v) thread loop (> 256 combinations), bias NULL, grad_bias NULL, NaN in the w3j padding,
      dynamic LDS above 64 kB (forward and reverse), just below / above the 160 kB limit: test_expansion, test_expansion_lds_limit, test_expansion_rejects
  k_qhgen_presplit layouts 0 / 1, col_scale, K = 32 / 64 / 128; k_qh_tp_gen<2 / 4 / 8, forward / reverse>, bias2 NULL, single row, partial last tile,
      C = 16 (one slice) .. 128: test_generator; test_generator_rejects"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from nabladft_amd import cg  # noqa: E402
from oracle import hblock_ref  # noqa: E402
from oracle import qhnet_ref as Q  # noqa: E402
from tests import cg_ref as G  # noqa: E402
from tests.helpers import DEV, D, P, _release_copies, assert_sum, check, host_i32, i32, lib, nan_dev, rejected, rel, rnd, st, twice  # noqa: E402,F401
from tests.test_qhnet_gpu import ORBITALS  # noqa: E402

F64, F32 = torch.float64, torch.float32


def qh():
    from nabladft_amd import qhnet
    return qhnet


def allowance(ref32, ref64):
    """The distance assert_sum allows between a kernel and the float64 value."""
    return max(3 * rel(ref32.detach().double().numpy(), ref64.detach().double().numpy()), 2e-6)


# ---- graph --------------------------------------------------------------------------------------------------------------------------------------------
def graph():
    """Symmetric CSR with rev, neighbours ascending: molecules of 6, 1 (an isolated atom: empty row), 7 and 3 atoms; atom 8 is bonded to every other atom
    of its molecule, every other atom to its successor at least.  N = 17 and R is no multiple of 8 (checked in gr()), so N * C and R * C are no multiples
    of 256 for C = 1, 32, 100."""
    rng = np.random.default_rng(4)
    sizes = [6, 1, 7, 3]
    N = sum(sizes)
    adj = np.zeros((N, N), dtype=bool)
    a0 = 0
    for n in sizes:
        blk = np.triu(rng.random((n, n)) < 0.45, 1) | np.eye(n, k=1, dtype=bool)
        adj[a0:a0 + n, a0:a0 + n] = blk | blk.T
        a0 += n
    adj[8, 7:14] = adj[7:14, 8] = True
    adj[8, 8] = False
    if adj.sum() % 8 == 0:                                                        # toggling one bond keeps R off the multiples of 8
        adj[14, 16] = adj[16, 14] = not adj[14, 16]
    own, col = np.nonzero(adj)                                                    # row-major: owners ascending, their neighbours ascending
    row_ptr = np.concatenate([[0], np.cumsum(adj.sum(1))])
    slot = {(int(o), int(c)): r for r, (o, c) in enumerate(zip(own, col))}
    rev = np.array([slot[(int(c), int(o))] for o, c in zip(own, col)])
    return dict(N=N, R=len(own), own=own, col=col, row_ptr=row_ptr, rev=rev, sizes=sizes)


_G = {}


def gr():
    if not _G:
        _G.update(graph())
        g = _G
        assert g["row_ptr"][7] == g["row_ptr"][6] and all(g["row_ptr"][n + 1] > g["row_ptr"][n] for n in range(g["N"]) if n != 6)    # the one empty row
        assert g["row_ptr"][9] - g["row_ptr"][8] == 6                             # bonded to the whole molecule
        assert np.array_equal(g["own"][g["rev"]], g["col"]) and np.array_equal(g["col"][g["rev"]], g["own"])
        for Cc in (1, 32, 100):
            assert (g["N"] * Cc) % 256 and (g["R"] * Cc) % 256, (g["N"], g["R"])
    return _G


# ---- invariants ---------------------------------------------------------------------------------------------------------------------------------------
def inv_ref(x, col, own, sfo, lmax):
    """qhnet_ref.invariants on the features padded to l <= 4, cut to the slots the kernel writes ([x0[dst] | x0[src or dst] | <.,.>_l / (2l+1), l <= lmax])."""
    Cc = x.shape[-1]
    return Q.invariants(G.pad25(x), torch.as_tensor(col), torch.as_tensor(own), bool(sfo))[:, :(2 + lmax) * Cc]


@pytest.mark.parametrize("Cc", [1, 32, 100])
@pytest.mark.parametrize("sfo", [0, 1])
@pytest.mark.parametrize("ncomp", [1, 4, 9, 16, 25])
def test_invariants(ncomp, sfo, Cc):
    g = gr()
    N, R, lmax = g["N"], g["R"], G.lmax_of(ncomp)
    gen = torch.Generator().manual_seed(ncomp * 10 + sfo + Cc)
    x, gs = rnd(gen, N, ncomp, Cc), rnd(gen, R, (2 + lmax) * Cc)
    xd, gsd = D(x), D(gs)
    ownd, cold, rpd, revd = D(i32(g["own"])), D(i32(g["col"])), D(i32(g["row_ptr"])), D(i32(g["rev"]))

    def fwd():
        s0 = nan_dev(R, (2 + lmax) * Cc)
        check(lib().nq_qh_invariants_forward(xd, N, ncomp, Cc, ownd, cold, R, sfo, P(s0), st()))
        return (s0,)

    def bwd():
        gx = nan_dev(N, ncomp, Cc)
        check(lib().nq_qh_invariants_backward(xd, gsd, N, ncomp, Cc, rpd, cold, revd, sfo, P(gx), st()))
        return (gx,)
    s0, gx = twice(fwd)[0].cpu(), twice(bwd)[0].cpu()
    refs = []
    for dt in (F64, F32):
        xr = x.to(dt).requires_grad_(True)
        s = inv_ref(xr, g["col"], g["own"], sfo, lmax)
        (s * gs.to(dt)).sum().backward()
        refs.append((s.detach(), xr.grad))
    assert torch.equal(s0[:, :Cc], x[g["col"], 0]) and torch.equal(s0[:, Cc:2 * Cc], x[g["own"] if sfo else g["col"], 0])       # the copied slots: exact
    assert_sum("invariants", s0, refs[0][0], refs[1][0])
    assert_sum("invariants grad_x", gx, refs[0][1], refs[1][1])
    assert torch.equal(gx[6], torch.zeros(ncomp, Cc))                             # the isolated atom
    # adjoint identity on the kernel outputs.  The copied slots are linear in x and the inner products quadratic, so (Euler) <x, bwd(g)> =
    # <fwd(x), g> over the linear slots + 2 <fwd(x), g> over the quadratic ones
    prod = s0.double() * gs.double()
    lhs = float(prod[:, :2 * Cc].sum() + 2 * prod[:, 2 * Cc:].sum())
    rhs = float((x.double() * gx.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * float(s0.double().norm() * gs.double().norm()), (lhs, rhs)


def test_invariants_reject_10_components():
    g = gr()
    x = torch.zeros(g["N"], 10, 4, device=DEV)
    idx = torch.zeros(g["R"] + g["N"] + 1, dtype=torch.int32, device=DEV)
    s0, gx = nan_dev(g["R"], 5 * 4), nan_dev(g["N"], 10, 4)
    rejected(lambda: lib().nq_qh_invariants_forward(P(x), g["N"], 10, 4, P(idx), P(idx), g["R"], 0, P(s0), st()), s0)
    rejected(lambda: lib().nq_qh_invariants_backward(P(x), P(s0), g["N"], 10, 4, P(idx), P(idx), P(idx), 0, P(gx), st()), gx)


# ---- tensor products ----------------------------------------------------------------------------------------------------------------------------------
def tp_paths(kind):
    return {"uvu1": qh().conv_paths(False), "uvu2": qh().conv_paths(True), "uuu": list(cg.ALL_PATHS)}[kind]


def test_tp_num_paths():
    assert int(lib().nq_qh_tp_num_paths(0)) == len(cg.ALL_PATHS) == 65
    assert int(lib().nq_qh_tp_num_paths(1)) == len(qh().conv_paths(False)) == 42
    assert int(lib().nq_qh_tp_num_paths(2)) == len(qh().conv_paths(True)) == 5
    assert int(lib().nq_qh_tp_num_paths(3)) == -1


def tp_inputs(kind, Cc, R, with_w2, gather_gy, seed, w1=None):
    paths = tp_paths(kind)
    n1 = 1 if kind == "uvu2" else 25
    N = 11
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    d = dict(kind=kind, paths=paths, n1=n1, N=N, Cc=Cc, R=R, x=rnd(gen, N, n1, Cc), idx1=rng.integers(0, N, size=R), gather_gy=gather_gy)
    d["idx1"][R // 2:] = d["idx1"][:R - R // 2]                                   # repeats
    if kind == "uuu":
        d["idx2"] = rng.integers(0, N, size=R)
        d["idx2"][-1] = d["idx2"][0]
    else:
        d["sh"] = rnd(gen, R, 25)
    d["w1"] = rnd(gen, R, len(paths), Cc) if w1 is None else w1
    d["w2"] = rnd(gen, R, len(paths), Cc) if with_w2 else None
    d["gy"] = rnd(gen, N if gather_gy else R, 25, Cc)
    d["idx_gy"] = rng.integers(0, N, size=R) if gather_gy else None
    d["const"] = torch.tensor(qh().path_constants(paths), dtype=F64).view(1, -1, 1)
    d["w1_kernel"] = (d["w1"].double() * d["const"]).float().contiguous()         # what qhnet.py hands to the kernel
    return d


def tp_refs(d):
    """[(y, grad x1 rows, grad x2 rows or None, grad w1, grad w2 or None)] in float64 and float32 from qhnet_ref.tensor_product and autograd."""
    out = []
    for dt in (F64, F32):
        x1 = d["x"].to(dt)[d["idx1"]].clone().requires_grad_(True)
        w1 = d["w1"].to(dt).clone().requires_grad_(True)
        w2 = None if d["w2"] is None else d["w2"].to(dt).clone().requires_grad_(True)
        w = w1 if w2 is None else w1 * w2
        if d["kind"] == "uuu":
            x2 = d["x"].to(dt)[d["idx2"]].clone().requires_grad_(True)
            y = Q.tensor_product(d["paths"], x1, x2, w, True)
        else:
            x2 = None
            y = Q.tensor_product(d["paths"], G.pad25(x1), d["sh"].to(dt), w, False)
        gy = d["gy"].to(dt)
        (y * (gy[d["idx_gy"]] if d["gather_gy"] else gy)).sum().backward()
        out.append((y.detach(), x1.grad, None if x2 is None else x2.grad, w1.grad, None if w2 is None else w2.grad))
    return out


def tp_run(d):
    """Forward and reverse kernels on the inputs of d (twice each): y, gx1 rows, gx2 rows or None, gw1 (w.r.t. the kernel's w1), gw2 or None."""
    kind, R, Cc, n1, NP = d["kind"], d["R"], d["Cc"], d["n1"], len(d["paths"])
    pset = {"uuu": 0, "uvu1": 1, "uvu2": 2}[kind]
    xd, i1 = D(d["x"]), D(i32(d["idx1"]))
    shd = D(d["sh"]) if kind != "uuu" else None
    i2 = D(i32(d["idx2"])) if kind == "uuu" else None
    w1d = D(d["w1_kernel"])
    w2d = D(d["w2"]) if d["w2"] is not None else None
    gyd = D(d["gy"])
    igd = D(i32(d["idx_gy"])) if d["gather_gy"] else None

    def fwd():
        y = nan_dev(R, 25, Cc)
        check(lib().nq_qh_tp_forward(xd, n1, i1, shd, i2, w1d, w2d, R, Cc, pset, P(y), st()))
        return (y,)

    def bwd():
        gx1, gw1 = nan_dev(R, n1, Cc), nan_dev(R, NP, Cc)
        gx2 = nan_dev(R, 25, Cc) if kind == "uuu" else None
        gw2 = nan_dev(R, NP, Cc) if w2d is not None else None
        check(lib().nq_qh_tp_backward(xd, n1, i1, shd, i2, w1d, w2d, gyd, igd, R, Cc, pset, P(gx1), P(gx2) if gx2 is not None else None, P(gw1),
                                      P(gw2) if gw2 is not None else None, st()))
        return tuple(t for t in (gx1, gx2, gw1, gw2) if t is not None)
    y = twice(fwd)[0]
    outs = list(twice(bwd))
    gx1 = outs.pop(0)
    gx2 = outs.pop(0) if kind == "uuu" else None
    gw1 = outs.pop(0)
    gw2 = outs.pop(0) if outs else None
    return y, gx1, gx2, gw1, gw2


def tp_compare(label, d, got, refs):
    y, gx1, gx2, gw1, gw2 = got
    r64, r32 = refs
    assert_sum(f"{label} y", y, r64[0], r32[0])
    assert_sum(f"{label} grad_x1", gx1, r64[1], r32[1])
    if gx2 is not None:
        assert_sum(f"{label} grad_x2", gx2, r64[2], r32[2])
    assert_sum(f"{label} grad_w1", gw1.cpu().double() * d["const"], r64[3], r32[3])          # d/dw = const * d/dw_kernel (the chain rule of the host fold)
    if gw2 is not None:
        assert_sum(f"{label} grad_w2", gw2, r64[4], r32[4])


# (C, R, w2 given, grad_y gathered by idx_gy): C = 1 and 100 leave partial wavefronts, R * C = 300 * 100 a partial last workgroup
TP_SHAPES = [(1, 1, True, False), (16, 37, False, True), (100, 300, True, True), (128, 37, True, False), (1, 300, False, False), (128, 1, False, True)]
_TP_REFS = {}


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("Cc,R,with_w2,gather_gy", TP_SHAPES)
@pytest.mark.parametrize("kind", ["uvu1", "uvu2", "uuu"])
def test_tp(kind, Cc, R, with_w2, gather_gy, variant):
    d = tp_inputs(kind, Cc, R, with_w2, gather_gy, seed=Cc * 1000 + R)
    key = (kind, Cc, R, with_w2, gather_gy)
    if key not in _TP_REFS:                                                       # the references do not depend on the code variant
        _TP_REFS[key] = tp_refs(d)
    try:
        lib().nq_qh_set_tp_variant(variant)
        got = tp_run(d)
        torch.cuda.synchronize()
    finally:
        lib().nq_qh_set_tp_variant(2)
    tp_compare(f"tp {kind} v{variant}", d, got, _TP_REFS[key])


@pytest.mark.parametrize("kind", ["uvu1", "uvu2", "uuu"])
def test_tp_weight_slots(kind):
    """One path's weight non-zero at a time: the first path, the last path and one path per output degree; any permutation of the weight slots shows."""
    paths = tp_paths(kind)
    chosen = sorted({0, len(paths) - 1} | {min(i for i, p in enumerate(paths) if p[2] == L) for L in range(5)} | {max(i for i, p in enumerate(paths) if p[2] == L)
                                                                                                                    for L in range(5)})
    Cc, R = 16, 5
    for p in chosen:
        w1 = torch.zeros(R, len(paths), Cc)
        w1[:, p] = rnd(torch.Generator().manual_seed(p), R, Cc)
        d = tp_inputs(kind, Cc, R, False, False, seed=p + 1, w1=w1)
        got, refs = tp_run(d), tp_refs(d)
        assert float(refs[0][0].abs().max()) > 0
        assert_sum(f"tp {kind} slot {p} y", got[0], refs[0][0], refs[1][0])
        assert_sum(f"tp {kind} slot {p} grad_x1", got[1], refs[0][1], refs[1][1])
        assert_sum(f"tp {kind} slot {p} grad_w1", got[3].cpu().double() * d["const"], refs[0][3], refs[1][3])


def test_tp_rejects():
    R, Cc, N = 4, 16, 3
    x, sh = torch.zeros(N, 25, Cc, device=DEV), torch.zeros(R, 25, device=DEV)
    idx = torch.zeros(R, dtype=torch.int32, device=DEV)
    w = torch.zeros(R, 65, Cc, device=DEV)
    # (ncomp1, sh, idx2, path set): harmonics with set 0; gathered operand with set 1; ncomp1 not matching the set (both ways); set 3
    bad = [(25, sh, None, 0), (25, None, idx, 1), (1, sh, None, 1), (25, sh, None, 2), (1, None, idx, 0), (25, sh, None, 3), (25, None, idx, 3)]
    for n1, s, i2, pset in bad:
        y = nan_dev(R, 25, Cc)
        ps, pi = (P(s) if s is not None else None), (P(i2) if i2 is not None else None)
        rejected(lambda: lib().nq_qh_tp_forward(P(x), n1, P(idx), ps, pi, P(w), None, R, Cc, pset, P(y), st()), y)
        gx1, gx2, gw1 = nan_dev(R, 25, Cc), nan_dev(R, 25, Cc), nan_dev(R, 65, Cc)
        rejected(lambda: lib().nq_qh_tp_backward(P(x), n1, P(idx), ps, pi, P(w), None, P(x), None, R, Cc, pset, P(gx1), P(gx2), P(gw1), None, st()), gx1, gx2, gw1)


# ---- pair reduce --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 25 * 32, 100])
@pytest.mark.parametrize("use_a,use_b,use_base", [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0)])
def test_pair_reduce(use_a, use_b, use_base, W):
    g = gr()
    N, R = g["N"], g["R"]
    gen = torch.Generator().manual_seed(W + use_a * 4 + use_b * 2 + use_base)
    a, b, base = rnd(gen, R, W), rnd(gen, R, W), rnd(gen, N, W)
    a, b, base = (a if use_a else None), (b if use_b else None), (base if use_base else None)
    ad, bd, based = (D(t) if t is not None else None for t in (a, b, base))
    rpd, revd = D(i32(g["row_ptr"])), D(i32(g["rev"]))

    def call():
        out = nan_dev(N, W)
        check(lib().nq_qh_pair_reduce(ad, bd, based, rpd, revd, N, W, P(out), st()))
        return (out,)
    out = twice(call)[0].cpu()
    refs = [G.pair_reduce_ref(a, b, base, g["row_ptr"], g["rev"], N, W, dt) for dt in (F64, F32)]
    assert_sum("pair_reduce", out, *refs)
    assert torch.equal(out[6], base[6] if use_base else torch.zeros(W))           # the empty row: base (or 0) exactly


def test_pair_reduce_rejects_both_operands_null():
    g = gr()
    out = nan_dev(g["N"], 8)
    rejected(lambda: lib().nq_qh_pair_reduce(None, None, None, D(i32(g["row_ptr"])), D(i32(g["rev"])), g["N"], 8, P(out), st()), out)


# ---- NormGate pieces ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [1, 32, 100])
@pytest.mark.parametrize("lmax", [0, 1, 2, 3, 4])
def test_normcat_and_gate(lmax, Cc):
    ncomp = (lmax + 1) ** 2
    for rows in (1, 77):
        gen = torch.Generator().manual_seed(lmax * 100 + Cc + rows)
        x, gates = rnd(gen, rows, ncomp, Cc), rnd(gen, rows, (lmax + 1) * Cc)
        zero_row = rows > 1 and lmax >= 2
        if zero_row:
            x[5, 4:9] = 0.0                                                       # an all-zero l = 2 block
        gf, gy = rnd(gen, rows, (lmax + 1) * Cc), rnd(gen, rows, ncomp, Cc)
        xd, gtd, gfd, gyd = D(x), D(gates), D(gf), D(gy)

        def ncat():
            f0, gx = nan_dev(rows, (lmax + 1) * Cc), nan_dev(rows, ncomp, Cc)
            check(lib().nq_qh_normcat(xd, None, rows, Cc, lmax, P(f0), st()))
            check(lib().nq_qh_normcat(xd, gfd, rows, Cc, lmax, P(gx), st()))
            return f0, gx

        def gate():
            y, gx, gg = nan_dev(rows, ncomp, Cc), nan_dev(rows, ncomp, Cc), nan_dev(rows, (lmax + 1) * Cc)
            check(lib().nq_qh_gate(xd, gtd, None, rows, Cc, lmax, P(y), None, None, st()))
            check(lib().nq_qh_gate(xd, gtd, gyd, rows, Cc, lmax, None, P(gx), P(gg), st()))
            return y, gx, gg
        f0, gxn = twice(ncat)
        y, gxg, gg = twice(gate)
        refs = []
        for dt in (F64, F32):
            xa = x.to(dt).requires_grad_(True)
            f = G.normcat_ref(xa)
            (f * gf.to(dt)).sum().backward()
            xb, gt = x.to(dt).requires_grad_(True), gates.to(dt).requires_grad_(True)
            yy = G.gate_ref(xb, gt)
            (yy * gy.to(dt)).sum().backward()
            refs.append((f.detach(), xa.grad, yy.detach(), xb.grad if xb.grad is not None else torch.zeros_like(xb), gt.grad))      # lmax = 0: y does not depend on x
        assert torch.equal(f0.cpu()[:, :Cc], x[:, 0])                             # the scalar slot: a copy
        assert_sum("normcat", f0, refs[0][0], refs[1][0])
        assert_sum("normcat grad_x", gxn, refs[0][1], refs[1][1])
        assert_sum("gate", y, refs[0][2], refs[1][2])
        assert_sum("gate grad_x", gxg, refs[0][3], refs[1][3])
        assert_sum("gate grad_gates", gg, refs[0][4], refs[1][4])
        assert torch.equal(y.cpu()[:, 0], gates[:, :Cc]) and torch.equal(gxg.cpu()[:, 0], torch.zeros(rows, Cc))
        if zero_row:
            assert torch.equal(f0.cpu()[5, 2 * Cc:3 * Cc], torch.zeros(Cc)) and torch.equal(gxn.cpu()[5, 4:9], torch.zeros(5, Cc))       # exactly 0, not NaN


def test_normcat_and_gate_reject():
    rows, Cc = 3, 8
    x, gates = torch.zeros(rows, 36, Cc, device=DEV), torch.zeros(rows, 6 * Cc, device=DEV)
    out = nan_dev(rows, 36, Cc)
    rejected(lambda: lib().nq_qh_normcat(P(x), None, rows, Cc, 5, P(out), st()), out)
    rejected(lambda: lib().nq_qh_gate(P(x), P(gates), None, rows, Cc, 5, P(out), None, None, st()), out)
    gg = nan_dev(rows, 5 * Cc)
    rejected(lambda: lib().nq_qh_gate(P(x), P(gates), P(x), rows, Cc, 4, None, None, P(gg), st()), gg)      # grad_y without grad_x


# ---- activations --------------------------------------------------------------------------------------------------------------------------------------
def act_points():
    t20 = np.float32(20.0)
    return torch.tensor([0.0, 1e-4, -1e-4, 20.0, float(np.nextafter(t20, np.float32(100.0))), float(np.nextafter(t20, np.float32(0.0))), 30.0, 88.0, -30.0, -100.0],
                        dtype=F32)


@pytest.mark.parametrize("cst", [1.0, "ssp"])
@pytest.mark.parametrize("backward", [0, 1])
@pytest.mark.parametrize("kind", [0, 1])
def test_act(kind, backward, cst):
    cst = float(np.float32(qh().normalize2mom_constant("ssp"))) if cst == "ssp" else 1.0
    gen = torch.Generator().manual_seed(kind * 2 + backward)
    pts = act_points()
    x = torch.cat([rnd(gen, 1531) * 3.0, pts])
    gy = rnd(gen, len(x))
    xd, gyd = D(x), D(gy)

    def call():
        out = nan_dev(len(x))
        check(lib().nq_qh_act(xd, gyd if backward else None, kind, cst, len(x), P(out), st()))
        return (out,)
    out = twice(call)[0].cpu()
    refs = []
    for dt in (F64, F32):
        xr = x.to(dt).requires_grad_(True)
        y = G.act_ref(xr, kind, cst)
        if backward:
            (y * gy.to(dt)).sum().backward()
            refs.append(xr.grad)
        else:
            refs.append(y.detach())
    n = len(x) - len(pts)
    assert torch.isfinite(out).all()
    assert_sum("act", out[:n], refs[0][:n], refs[1][:n])
    r64 = refs[0][n:].numpy()
    err = np.abs(out[n:].double().numpy() - r64)
    own = np.abs(refs[1][n:].double().numpy() - r64)
    ulp2 = 2 * np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64)
    print("act fixed points: err", err, "allowed", np.maximum(ulp2, own))
    assert (err <= np.maximum(ulp2, own)).all(), (pts.numpy(), err, ulp2, own)


def test_act_rejects_kind_2():
    x = torch.zeros(8, device=DEV)
    out = nan_dev(8)
    rejected(lambda: lib().nq_qh_act(P(x), None, 2, 1.0, 8, P(out), st()), out)


# ---- expansion ----------------------------------------------------------------------------------------------------------------------------------------
def model_w3j(counts, Cb):
    """The [19, 5, 5, 9] float32 table nabladft_amd.qhnet.Expansion hands to the kernels, with NaN written into every padded entry."""
    w = qh().Expansion(Cb, *counts)._w3j.clone()
    for k, (li, l1, l2) in enumerate(G.EXP_INSTRUCTIONS):
        pad = torch.ones(5, 5, 9, dtype=torch.bool)
        pad[:2 * l1 + 1, :2 * l2 + 1, :2 * li + 1] = False
        assert float(w[k][pad].abs().sum()) == 0.0 and float(w[k][~pad].abs().sum()) > 0
        w[k][pad] = float("nan")
    return w


MODEL_COUNTS = tuple(hblock_ref.orbital_masks(ORBITALS)[1:])
# (shell counts, Cb, R, bias given, grad_bias given)
EXP_CASES = [((1, 1, 1), 4, 1, True, True), ((1, 1, 1), 64, 19, False, False), ((3, 2, 1), 32, 19, True, True), ((3, 2, 1), 4, 19, False, True),
             (MODEL_COUNTS, 32, 19, True, True), (MODEL_COUNTS, 64, 1, True, False), ((8, 6, 4), 32, 19, True, True), ((8, 6, 4), 4, 1, False, False),
             ((3, 2, 1), 64, 1, True, True)]


def exp_run(counts, Cb, R, x, W, b, g, want_gb):
    nw, nb, S, _, _ = G.expansion_layout(counts, Cb)
    xd, Wd, gd = D(x), D(W), D(g)
    bd = D(b) if b is not None else None
    w3d = D(model_w3j(counts, Cb))
    sh = host_i32(counts)

    def fwd():
        out = nan_dev(R, S, S)
        check(lib().nq_qh_expansion_forward(xd, Wd, bd, R, Cb, sh, nw, nb, w3d, P(out), st()))
        return (out,)

    def bwd():
        gx, gW, gb = nan_dev(R, 25, Cb), nan_dev(R, nw), nan_dev(R, nb)
        check(lib().nq_qh_expansion_backward(xd, Wd, gd, R, Cb, sh, nw, nb, w3d, P(gx), P(gW), P(gb) if want_gb else None, st()))
        return gx, gW, gb
    return (twice(fwd)[0],) + tuple(twice(bwd))


def exp_refs(counts, x, W, b, g):
    R = x.shape[0]
    nb = G.expansion_layout(counts, x.shape[-1])[1]
    out = []
    for dt in (F64, F32):
        xr, Wr = x.to(dt).requires_grad_(True), W.to(dt).requires_grad_(True)
        br = (torch.zeros(R, nb, dtype=dt) if b is None else b.to(dt)).requires_grad_(True)
        y = Q.expansion(xr, Wr, br, counts)
        (y * g.to(dt)).sum().backward()
        out.append((y.detach(), xr.grad, Wr.grad, br.grad))
    return out


@pytest.mark.parametrize("counts,Cb,R,with_bias,with_gb", EXP_CASES, ids=[f"{c[0][0]}{c[0][1]}{c[0][2]}-Cb{c[1]}-R{c[2]}-b{int(c[3])}-gb{int(c[4])}" for c in EXP_CASES])
def test_expansion(counts, Cb, R, with_bias, with_gb):
    nw, nb, S, _, combos = G.expansion_layout(counts, Cb)
    assert MODEL_COUNTS == (5, 4, 3)
    if counts == (8, 6, 4):
        assert combos > 256                                                       # second pass of the thread loop
        if Cb == 32:
            assert G.expansion_lds_forward(counts, Cb) > 64 * 1024 and G.expansion_lds_backward(counts, Cb) > 64 * 1024
    gen = torch.Generator().manual_seed(sum(counts) * 100 + Cb + R)
    x, W, g = rnd(gen, R, 25, Cb), rnd(gen, R, nw), rnd(gen, R, S, S)
    b = rnd(gen, R, nb) if with_bias else None
    out, gx, gW, gb = exp_run(counts, Cb, R, x, W, b, g, with_gb)
    r64, r32 = exp_refs(counts, x, W, b, g)
    assert_sum("expansion", out, r64[0], r32[0])
    assert_sum("expansion grad_x", gx, r64[1], r32[1])
    assert_sum("expansion grad_W", gW, r64[2], r32[2])
    if with_gb:
        assert_sum("expansion grad_bias", gb, r64[3], r32[3])
    else:
        assert torch.isnan(gb).all()
    # adjoint identity on the kernel outputs: out = B(W, x) + L(b), so <out, g> = <x, gx> + <b, gb> = <W, gW> + <b, gb>
    lhs = float((out.cpu().double() * g.double()).sum())
    bterm = float((b.double() * gb.cpu().double()).sum()) if with_bias and with_gb else (float((b.double() * r64[3]).sum()) if with_bias else 0.0)
    scale = 1e-6 * float(out.cpu().double().norm() * g.double().norm())
    assert abs(lhs - float((x.double() * gx.cpu().double()).sum()) - bterm) <= scale
    assert abs(lhs - float((W.double() * gW.cpu().double()).sum()) - bterm) <= scale


def lds_edge(fn):
    """Among the layouts (n_s, n_p, n_d, Cb = 64) the one with the largest LDS request <= 160 kB and the one with the smallest above it."""
    below = above = None
    for a in range(1, 16):
        for b in range(1, 12):
            for c in range(1, 9):
                v = fn((a, b, c), 64)
                if v <= 160 * 1024 and (below is None or v > below[0]):
                    below = (v, (a, b, c))
                if v > 160 * 1024 and (above is None or v < above[0]):
                    above = (v, (a, b, c))
    return below, above


@pytest.mark.parametrize("side", ["forward", "backward"])
def test_expansion_lds_limit(side):
    below, above = lds_edge(G.expansion_lds_forward if side == "forward" else G.expansion_lds_backward)
    assert 159 * 1024 < below[0] <= 160 * 1024 < above[0] < 161 * 1024, (below, above)
    Cb, R = 64, 1
    for (v, counts), ok in ((below, True), (above, False)):
        nw, nb, S, _, _ = G.expansion_layout(counts, Cb)
        gen = torch.Generator().manual_seed(v)
        x, W, b, g = rnd(gen, R, 25, Cb), rnd(gen, R, nw), rnd(gen, R, nb), rnd(gen, R, S, S)
        w3d, sh = D(model_w3j(counts, Cb)), host_i32(counts)
        if side == "forward":
            out = nan_dev(R, S, S)
            call = lambda: lib().nq_qh_expansion_forward(D(x), D(W), D(b), R, Cb, sh, nw, nb, w3d, P(out), st())      # noqa: E731
            outs = (out,)
        else:
            outs = (nan_dev(R, 25, Cb), nan_dev(R, nw), nan_dev(R, nb))
            call = lambda: lib().nq_qh_expansion_backward(D(x), D(W), D(g), R, Cb, sh, nw, nb, w3d, P(outs[0]), P(outs[1]), P(outs[2]), st())      # noqa: E731
        if not ok:
            rejected(call, *outs)
            continue
        check(call())
        torch.cuda.synchronize()
        r64, r32 = exp_refs(counts, x, W, b, g)
        if side == "forward":
            assert_sum("expansion at the LDS limit", outs[0], r64[0], r32[0])
        else:
            for name, t, k in (("grad_x", outs[0], 1), ("grad_W", outs[1], 2), ("grad_bias", outs[2], 3)):
                assert_sum(f"expansion {name} at the LDS limit", t, r64[k], r32[k])


def test_expansion_rejects():
    R = 2
    for counts, Cb, dnw, dnb in [((3, 2, 1), 6, 0, 0), ((3, 2, 1), 68, 0, 0), ((3, 0, 1), 8, 0, 0), ((0, 2, 1), 8, 0, 0), ((3, 2, 1), 8, 4, 0), ((3, 2, 1), 8, 0, 1)]:
        nw, nb, S, _, _ = G.expansion_layout(tuple(max(c, 1) for c in counts), Cb)
        x, W, b = torch.zeros(R, 25, Cb, device=DEV), torch.zeros(R, nw + 8, device=DEV), torch.zeros(R, nb + 8, device=DEV)
        w3 = torch.zeros(19, 5, 5, 9, device=DEV)
        out = nan_dev(R, S, S)
        rejected(lambda: lib().nq_qh_expansion_forward(P(x), P(W), P(b), R, Cb, host_i32(counts), nw + dnw, nb + dnb, P(w3), P(out), st()), out)
        gx, gW, gb = nan_dev(R, 25, Cb), nan_dev(R, nw + 8), nan_dev(R, nb + 8)
        g = torch.zeros(R, S, S, device=DEV)
        rejected(lambda: lib().nq_qh_expansion_backward(P(x), P(W), P(g), R, Cb, host_i32(counts), nw + dnw, nb + dnb, P(w3), P(gx), P(gW), P(gb), st()), gx, gW, gb)


# ---- fused generator ----------------------------------------------------------------------------------------------------------------------------------
# (K, C, R, bias2 given, layout of W1, layout of W2, col_scale given)
GEN_CASES = [(128, 128, 70, True, 0, 1, False), (32, 16, 1, False, 0, 0, True), (64, 32, 31, True, 1, 1, True), (128, 16, 32, False, 1, 0, False),
             (32, 128, 33, True, 0, 1, True), (64, 16, 70, True, 0, 1, False)]


def presplit(Wt, scale, K, Cc, layout):
    """Fragments of one generator's weights (+ a NaN guard band that must stay NaN)."""
    nfl = int(lib().nq_qh_gen_fragment_floats(Cc, K))
    assert nfl == (Cc // 16) * 33 * (K // 16) * 2 * 64 * 4
    frag = nan_dev(nfl + 64)
    check(lib().nq_qh_gen_presplit(D(Wt), D(scale) if scale is not None else None, K, Cc, layout, P(frag), st()))
    torch.cuda.synchronize()
    assert torch.isnan(frag[nfl:]).all() and not torch.isnan(frag[:nfl]).any()     # (a packed pair of finite bfloat16 values is never the NaN pattern)
    return frag


def gen_eval(x, idx1, idx2, w1, w2, gy, dt):
    """Reference tensor product with GIVEN per-row factors w1, w2 [R, 65, C] (the kernel's own weights: no path constant folded in, so the reference's
    weight is w1 w2 / path_constants) and all its adjoints."""
    const = torch.tensor(qh().path_constants(cg.ALL_PATHS), dtype=dt).view(1, -1, 1)
    x1, x2 = x.to(dt)[idx1].clone().requires_grad_(True), x.to(dt)[idx2].clone().requires_grad_(True)
    a, b = w1.to(dt).clone().requires_grad_(True), w2.to(dt).clone().requires_grad_(True)
    y = Q.tensor_product(cg.ALL_PATHS, x1, x2, a * b / const, True)
    (y * gy.to(dt)).sum().backward()
    return [y.detach(), x1.grad, x2.grad, a.grad, b.grad]


@pytest.mark.parametrize("K,Cc,R,with_bias,lay1,lay2,with_scale", GEN_CASES, ids=[f"K{c[0]}-C{c[1]}-R{c[2]}-b{int(c[3])}-l{c[4]}{c[5]}-s{int(c[6])}" for c in GEN_CASES])
def test_generator(K, Cc, R, with_bias, lay1, lay2, with_scale):
    N, ncol = 9, 65 * Cc
    gen = torch.Generator().manual_seed(K + Cc + R)
    rng = np.random.default_rng(K + Cc + R)
    x = rnd(gen, N, 25, Cc)
    idx1, idx2 = rng.integers(0, N, size=R), rng.integers(0, N, size=R)
    h1, h2 = rnd(gen, R, K), rnd(gen, R, K)
    W1, W2 = rnd(gen, K, ncol) / math.sqrt(K), rnd(gen, K, ncol) / math.sqrt(K)     # [K, columns]; handed over transposed for layout 1
    s1, s2 = (rnd(gen, ncol).abs() + 0.5, rnd(gen, ncol).abs() + 0.5) if with_scale else (None, None)
    b2 = rnd(gen, ncol) if with_bias else None
    gy = rnd(gen, R, 25, Cc)
    frags = [presplit(W.t().contiguous() if lay else W, s, K, Cc, lay) for W, s, lay in ((W1, s1, lay1), (W2, s2, lay2))]
    nfl = frags[0].numel() - 64
    xd, i1, i2, h1d, h2d, gyd = D(x), D(i32(idx1)), D(i32(idx2)), D(h1), D(h2), D(gy)
    b2d = D(b2) if b2 is not None else None

    def fwd():
        y = nan_dev(R + 32, 25, Cc)
        check(lib().nq_qh_tp_forward_gen(xd, i1, i2, h1d, h2d, P(frags[0]), P(frags[1]), b2d, R, Cc, K, P(y), st()))
        return (y,)

    def bwd():
        outs = nan_dev(R + 32, 25, Cc), nan_dev(R + 32, 25, Cc), nan_dev(R + 32, 65, Cc), nan_dev(R + 32, 65, Cc)
        check(lib().nq_qh_tp_backward_gen(xd, i1, i2, h1d, h2d, P(frags[0]), P(frags[1]), b2d, gyd, R, Cc, K, *[P(t) for t in outs], st()))
        return outs
    got = [t.cpu() for t in twice(fwd) + tuple(twice(bwd))]
    for t in got:
        assert torch.isnan(t[R:]).all()                                           # nothing behind the last row
    got = [t[:R] for t in got]
    assert torch.isnan(frags[0][nfl:]).all() and torch.isnan(frags[1][nfl:]).all()
    # the weights the kernel works from: col_scale multiplied in float32 first, then the two-piece products (mirror) or the exact float64 product
    We = [(W * s[None]) if s is not None else W for W, s in ((W1, s1), (W2, s2))]
    bias = b2.double().view(1, 65, Cc) if b2 is not None else 0.0
    mirror = [torch.tensor(G.split2_mirror(h.numpy(), W.numpy())).view(R, 65, Cc) for h, W in ((h1, We[0]), (h2, We[1]))]
    mirror[1] = mirror[1] + bias
    exact = [(h.double() @ W.double()).view(R, 65, Cc) for h, W in ((h1, We[0]), (h2, We[1]))]
    exact[1] = exact[1] + bias
    ref1 = gen_eval(x, idx1, idx2, mirror[0], mirror[1], gy, F64)
    ref1_32 = gen_eval(x, idx1, idx2, mirror[0].float(), mirror[1].float(), gy, F32)
    ref2 = gen_eval(x, idx1, idx2, exact[0], exact[1], gy, F64)
    names = ["y", "grad_x1", "grad_x2", "grad_w1", "grad_w2"]
    dist = []
    for name, g_, a, a32, e in zip(names, got, ref1, ref1_32, ref2):
        assert_sum(f"generator {name} vs mirror", g_, a, a32)                      # (1) the tight check
        d12 = rel(a.numpy(), e.numpy())
        d_k = rel(g_.double().numpy(), e.numpy())
        dist.append((d12, d_k))
        assert d_k <= d12 + allowance(a32, a), (name, d_k, d12)                    # (2) against the exact weights
    print(f"generator K={K} C={Cc} R={R}: mirror vs exact reference y {dist[0][0]:.2e}, adjoints <= {max(d[0] for d in dist[1:]):.2e}; "
          f"kernel vs exact reference y {dist[0][1]:.2e}, adjoints <= {max(d[1] for d in dist[1:]):.2e}")
    # the two library paths at operator level: the materialised kernel fed with the mirror weights
    w1m, w2m = D(mirror[0].float().contiguous()), D(mirror[1].float().contiguous())
    y_tp = nan_dev(R, 25, Cc)
    check(lib().nq_qh_tp_forward(xd, 25, i1, None, i2, w1m, w2m, R, Cc, 0, P(y_tp), st()))
    torch.cuda.synchronize()
    d_paths = rel(got[0].double().numpy(), y_tp.cpu().double().numpy())
    assert d_paths <= allowance(ref1_32[0], ref1[0]) and d_paths < 1e-5, d_paths


def test_generator_rejects():
    R, N = 4, 3
    for Cc, K in [(24, 32), (16, 48)]:
        x, idx = torch.zeros(N, 25, 32, device=DEV), torch.zeros(R, dtype=torch.int32, device=DEV)
        h, frag = torch.zeros(R, 128, device=DEV), torch.zeros(int(lib().nq_qh_gen_fragment_floats(32, 128)), device=DEV)
        y = nan_dev(R + 32, 25, 32)
        rejected(lambda: lib().nq_qh_tp_forward_gen(P(x), P(idx), P(idx), P(h), P(h), P(frag), P(frag), None, R, Cc, K, P(y), st()), y)
        outs = nan_dev(R + 32, 25, 32), nan_dev(R + 32, 25, 32), nan_dev(R + 32, 65, 32), nan_dev(R + 32, 65, 32)
        rejected(lambda: lib().nq_qh_tp_backward_gen(P(x), P(idx), P(idx), P(h), P(h), P(frag), P(frag), None, P(x), R, Cc, K, *[P(t) for t in outs], st()), *outs)
    W = torch.zeros(144, 65 * 16, device=DEV)
    for K, layout in [(144, 0), (8, 0), (32, 2)]:
        frag = nan_dev(int(lib().nq_qh_gen_fragment_floats(16, 144)) + 64)
        rejected(lambda: lib().nq_qh_gen_presplit(P(W), None, K, 16, layout, P(frag), st()), frag)
