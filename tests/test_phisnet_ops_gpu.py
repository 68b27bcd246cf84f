"""The PhiSNet basis, activation, data-movement and linear kernels (csrc/geobasis.hip, the nq_sph_linear_* entry points of csrc/gemm.hip) and
nq_hamiltonian_loss (csrc/hblock.hip) one by one through the C ABI, called the way phisnet.py, so3.py and hamiltonian.py call them, against the float64
restatements of tests/phisnet_ops_ref.py (pinned to the reference project by test_phisnet_ops_ref_cpu.py) and oracle/hblock_ref.hamiltonian_loss; adjoints
come from torch.autograd on the float64 evaluation, per row.  Every output buffer starts as NaN, scratch included; every call runs twice with bitwise
equal results.

Bounds (the convention of test_escn_ops_gpu.py): copies and gathers are bitwise; every other output within max(3 x the error of the same restatement
evaluated in float32 on the CPU, 2e-6) of the float64 value AND below 1e-5, array-relative (assert_sum).  Where the float32 formula alone is already further
than a third of 1e-5 from the float64 value, the fixed ceiling says nothing about the kernel and the bound is the yardstick alone (assert_yard: 3 x the
float32-CPU error on the same inputs, computed in the test).  These are, each with what was measured on an MI355X (array-relative distance from the
float64 value: the kernel / the float32 CPU restatement on the same inputs; ranges over the parametrised cases):
    nq_bernstein_rbf*, K = 128 (YARD_BERNSTEIN; the exponent log C_k + n_k x + v_k log(1 - e^x) sums terms of size ~80 that cancel, and log C_k itself is
      rounded to float32).  Over cutoff 5 / 12 / 15 and alpha 0.1 / 0.5 / 1.3:
        value           kernel 2.97e-6 .. 6.77e-6, restatement 2.72e-6 .. 6.78e-6; at cutoff 15: 3.57e-6 / 3.70e-6, 3.99e-6 / 3.87e-6, 3.74e-6 / 3.74e-6
        per-row d/dalpha       2.76e-6 .. 9.57e-6,             2.34e-6 .. 9.56e-6; at cutoff 15: 3.52e-6 / 3.32e-6, 2.76e-6 / 3.08e-6, 9.57e-6 / 9.56e-6
        per-row d/dr           1.28e-6 .. 4.13e-6,             9.49e-7 .. 6.31e-6; at cutoff 15: 1.28e-6 / 9.94e-7, 3.73e-6 / 4.79e-6, 3.47e-6 / 4.50e-6
      the kernel is never further than 2.4 x the restatement.  K <= 32 stays under the fixed ceiling (restatement at most 4.0e-6, d/dalpha at K = 32).
    shifted softplus at beta = 1e-4 (softplus(beta x) - ln 2 cancels to ~beta x / 2 before it is divided by beta, or by beta^2 in d/dbeta); these columns
      are compared on their own, so that they do not set the scale for the others.  Over F = 1 / 7 / 128 (nq_feature_act and nq_packed_act0 alike):
        y               kernel 9.96e-6 .. 1.24e-5, restatement 9.69e-6 .. 1.24e-5
        per-row d/dalpha       1.07e-5 .. 1.97e-5,             1.07e-5 .. 1.97e-5
        per-row d/dbeta        4.35e-3 .. 8.76e-3,             4.35e-3 .. 8.76e-3      (the kernel is never further than 1.14 x the restatement)
      gx of these columns, and every output of the other columns (beta > 0, < 0, == 0), stay under the fixed ceiling.

Branches and the tests that reach them:
  k_sph_harm orders 0..4, P = 1 / 255 / 257, the axis directions, components past (L + 1)^2 of a wider buffer untouched: test_sph_harm
  k_sph_harm_bwd unit and free (|u| in 0.5..2) vectors, random grad_out: test_sph_harm_backward; every derivative block on its own (one-hot grad_out):
      test_sph_harm_backward_one_hot
  k_bernstein_rbf<0 / 1 / 2>, host alpha and device alpha (bitwise equal), rows at / beyond the cutoff exactly 0, per-row gradients: test_bernstein
  k_radial_basis<false / true> kinds 1..4, K = 1, per-row d/dalpha of kinds 2 and 3: test_radial_basis; argument checks (kinds 1 / 4 have no
      gradient, t1 / t2 NULL, K <= 0, P < 0): test_radial_basis_rejects
  k_feature_act both kinds, beta > 0 / < 0 / 1e-4 / == 0 (limit derivatives 0.5 a, 0.5 x, a x^2 / 8), the tails at x = +-30, +-90: test_feature_act
  k_packed_act0 ncomp 1 / 9 / 25, copies bitwise, partials [rows, F] (ga_rows[r * F + f]), scalar rows bitwise nq_feature_act: test_packed_act0
  k_gather_rows, k_segment_sum (base NULL / given, empty segment, 300-row segment), k_segment_sum_perm (order = stable argsort, adjoint identity),
      base with order rejected: test_gather_and_segment_sum
  nq_sph_linear_*: batched gemm2 (a), batched gemm3 (b), row-mapped generic (c, d), generic through the alignment test (e), orders 5 and 6 (f), bias
      present / NULL, the scratch guard: test_sph_linear (each case asserts the launch path it names through sph_paths, the mirror of the host rule);
      the empty-split fallback of the weight gradient, NaN scratch, with and without gbias0, bracketed by 3840 rows and by 1921 rows at order 6:
      test_sph_linear_weight_grad_empty_splits; rows = 0: test_sph_linear_zero_rows; order 7, Fin = 0, NULL weight: test_sph_linear_rejects
  k_hb_loss_partial more than one grid-stride pass, k_hb_loss_grad d == 0, grad_scale = 0.25, grad NULL: test_hamiltonian_loss; rmse == 0 and
      total = 0: test_hamiltonian_loss_zero_and_rejects

Case (d) of the spherical linear (rows 37, order 2, Fin 8, Fout 6): the packed row stride of y is 9 * 6 floats and the component stride 6, neither a
multiple of 4, so the host rule sends the forward to the row-mapped kernel as well (Fin = 8 only lets that kernel read x with 16-byte loads); the case
asserts what the rule gives."""
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

from oracle import hblock_ref  # noqa: E402
from tests import phisnet_ops_ref as R  # noqa: E402
from tests.helpers import (DEV, NAN, D, P, _release_copies, assert_sum, assert_yard, bits, check, host_ptrs, lib, nan_dev, rejected, rel, rnd,  # noqa: E402,F401
                           st, twice)                                  # (_release_copies: autouse)

F64, F32 = torch.float64, torch.float32


def record(name, err, own):
    """One line per yardstick case on stdout (pytest -s): the numbers the module docstring quotes."""
    print(f"MEASURED {name}: kernel {err:.2e}, float32 CPU restatement {own:.2e}")


def grads(out, inputs, g):
    """torch.autograd.grad that gives zeros for an input the output does not depend on."""
    if not out.requires_grad:
        return [torch.zeros_like(i) for i in inputs]
    got = torch.autograd.grad(out, inputs, g, allow_unused=True)
    return [torch.zeros_like(i) if x is None else x for x, i in zip(got, inputs)]


# ---- spherical harmonics --------------------------------------------------------------------------------------------------------------------------------
def sph_vectors(n, free):
    """The six axis directions, (1, 1, 1) / sqrt(3) and random directions, normalised in float64; ``free``: lengths 0.5..2 instead of 1."""
    rng = np.random.default_rng(11)
    u = np.concatenate([np.eye(3), -np.eye(3), np.ones((1, 3)), rng.normal(size=(max(n, 8), 3))])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if free:
        u *= rng.uniform(0.5, 2.0, size=(len(u), 1))
    return torch.tensor(u[:n].astype(np.float32))


def sph_adjoint(L, u, g, dtype):
    x = u.to(dtype).clone().requires_grad_(True)
    return grads(R.sph_harm(L, x, dtype), [x], g.to(dtype))[0]


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("L", [0, 1, 2, 3, 4])
def test_sph_harm(L, n):
    u, nc = sph_vectors(n, False), (L + 1) ** 2
    ud = u.to(DEV)

    def call():
        buf = nan_dev(n * 25)                      # room for order 4: order L writes the first n * (L + 1)^2 floats only
        check(lib().nq_sph_harm(P(ud), n, L, P(buf), st()))
        return (buf,)
    (buf,) = twice(call)
    assert torch.isnan(buf[n * nc:]).all()
    assert_sum(f"Y L={L}", buf[:n * nc].view(n, nc), R.sph_harm(L, u, F64), R.sph_harm(L, u, F32))


@pytest.mark.parametrize("free", [False, True], ids=["unit", "free"])
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("L", [0, 1, 2, 3, 4])
def test_sph_harm_backward(L, n, free):
    u, nc = sph_vectors(n, free), (L + 1) ** 2
    g = rnd(torch.Generator().manual_seed(3), n, nc)
    ud, gd = u.to(DEV), g.to(DEV)

    def call():
        gu = nan_dev(n, 3)
        check(lib().nq_sph_harm_backward(P(ud), P(gd), n, L, P(gu), st()))
        return (gu,)
    (gu,) = twice(call)
    assert_sum(f"dY L={L}", gu, sph_adjoint(L, u, g, F64), sph_adjoint(L, u, g, F32))


@pytest.mark.parametrize("L", [0, 1, 2, 3, 4])
def test_sph_harm_backward_one_hot(L):
    """grad_out = one component at a time: gu is dY_c / d(x, y, z) itself, so a wrong term cannot hide in a sum over components."""
    n, nc = 257, (L + 1) ** 2
    u = sph_vectors(n, True)
    ud = u.to(DEV)
    for c in range(nc):
        g = torch.zeros(n, nc)
        g[:, c] = 1.0
        gd = g.to(DEV)

        def call():
            gu = nan_dev(n, 3)
            check(lib().nq_sph_harm_backward(P(ud), P(gd), n, L, P(gu), st()))
            return (gu,)
        (gu,) = twice(call)
        assert_sum(f"dY L={L} component {c}", gu, sph_adjoint(L, u, g, F64), sph_adjoint(L, u, g, F32))


# ---- radial bases ---------------------------------------------------------------------------------------------------------------------------------------
def radii(cutoff):
    """300 radii uniform in [0.3, 0.999 c], then 0.9999 c, c, the float32 below c, 1.2 c (two rows at / beyond the cutoff) and 0.5 c: 305 rows, odd, so
    that rows * K is no multiple of the 256 elements of a workgroup for any K below 256."""
    rng = np.random.default_rng(7)
    c = np.float32(cutoff)
    tail = [0.9999 * cutoff, cutoff, float(np.nextafter(c, np.float32(0.0))), 1.2 * cutoff, 0.5 * cutoff]
    return torch.tensor(np.concatenate([rng.uniform(0.3, 0.999 * cutoff, size=300), tail]).astype(np.float32))


def bernstein_reference(r, g, K, cutoff, alpha, dtype):
    """value [n, K], per-row d/dalpha [n], per-row d/dr [n] of sum(value * g)."""
    rr = r.to(dtype).clone().requires_grad_(True)
    al = torch.full((len(r), 1), alpha, dtype=dtype, requires_grad=True)
    out = R.exp_bernstein(rr, K, cutoff, al, dtype)
    gr, ga = grads(out, [rr, al], g.to(dtype))
    return out.detach(), ga.reshape(-1), gr


YARD_BERNSTEIN = {128}          # K whose float32 formula alone is further than a third of 1e-5 from the float64 value (module docstring)


@pytest.mark.parametrize("alpha", [0.1, 0.5, 1.3])
@pytest.mark.parametrize("cutoff", [5.0, 12.0, 15.0])
@pytest.mark.parametrize("K", [1, 2, 8, 32, 128])
def test_bernstein(K, cutoff, alpha):
    r = radii(cutoff)
    n = len(r)
    assert (n * K) % 256 != 0 and n % 256 != 0
    alpha = float(np.float32(alpha))                                  # the value the kernels see, host float or device scalar
    g = rnd(torch.Generator().manual_seed(K), n, K)
    tabs = [t.to(DEV) for t in R.bernstein_tables(K, F32)]
    rd, gd, ad = r.to(DEV), g.to(DEV), torch.tensor([alpha], dtype=F32, device=DEV)
    tp = [P(t) for t in tabs]

    def call():
        v_h, v_d, ga_h, ga_d, gr_d = nan_dev(n, K), nan_dev(n, K), nan_dev(n), nan_dev(n), nan_dev(n)
        check(lib().nq_bernstein_rbf(P(rd), n, K, alpha, cutoff, *tp, P(v_h), st()))
        check(lib().nq_bernstein_rbf_dev(P(rd), n, K, P(ad), cutoff, *tp, P(v_d), st()))
        check(lib().nq_bernstein_rbf_grad_alpha(P(rd), P(gd), n, K, alpha, cutoff, *tp, P(ga_h), st()))
        check(lib().nq_bernstein_rbf_grad_alpha_dev(P(rd), P(gd), n, K, P(ad), cutoff, *tp, P(ga_d), st()))
        check(lib().nq_bernstein_rbf_grad_r_dev(P(rd), P(gd), n, K, P(ad), cutoff, *tp, P(gr_d), st()))
        return v_h, v_d, ga_h, ga_d, gr_d
    v_h, v_d, ga_h, ga_d, gr_d = twice(call)
    assert torch.equal(bits(v_h), bits(v_d)) and torch.equal(bits(ga_h), bits(ga_d))
    beyond = r >= cutoff
    assert int(beyond.sum()) == 2
    for t in (v_h, ga_h, gr_d):
        assert float(t.cpu()[beyond].abs().max()) == 0.0              # exactly 0 at / beyond the cutoff, value and both gradients
    ref64, ref32 = bernstein_reference(r, g, K, cutoff, alpha, F64), bernstein_reference(r, g, K, cutoff, alpha, F32)
    for name, got, r64, r32 in zip(("value", "d/dalpha rows", "d/dr rows"), (v_h, ga_h, gr_d), ref64, ref32):
        if K in YARD_BERNSTEIN:
            record(f"bernstein K={K} cutoff={cutoff:g} alpha={alpha:.1f} {name}", *assert_yard(name, got, r64, r32))
        else:
            assert_sum(name, got, r64, r32)


RADIAL_ARGS = {1: (16, 6.0, 0.0), 2: (16, 6.0, 0.7), 3: (12, 7.0, 0.9), 4: (12, 5.0, 0.0)}      # (K, cutoff, alpha) of tests/golden/geometry_bases.npz


def radial_reference(kind, r, g, K, cutoff, alpha, dtype):
    al = torch.full((len(r), 1), alpha, dtype=dtype, requires_grad=True)
    out = R.radial_basis(kind, r, K, cutoff, al, dtype)
    return out.detach(), grads(out, [al], g.to(dtype))[0].reshape(-1)


def radial_call(kind, rd, n, K, alpha, cutoff, width, t, out):
    return lib().nq_radial_basis(kind, P(rd), n, K, alpha, cutoff, width, P(t[0]), P(t[1]), P(t[2]), P(out), st())


def radial_grad_call(kind, rd, gd, n, K, alpha, cutoff, width, t, rows):
    return lib().nq_radial_basis_grad_alpha(kind, P(rd), P(gd), n, K, alpha, cutoff, width, P(t[0]), P(t[1]), P(t[2]), P(rows), st())


@pytest.mark.parametrize("one", [False, True], ids=["K-fixture", "K-1"])
@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_radial_basis(kind, one):
    K, cutoff, alpha = RADIAL_ARGS[kind]
    K = 1 if one else K
    alpha = float(np.float32(alpha))
    r = radii(cutoff)
    n = len(r)
    assert (n * K) % 256 != 0
    g = rnd(torch.Generator().manual_seed(kind), n, K)
    *tabs, width = R.radial_tables(kind, K, cutoff, F32)
    width = float(np.float32(width))
    t = [None if x is None else x.to(DEV) for x in tabs]
    rd, gd = r.to(DEV), g.to(DEV)

    def call():
        out, rows = nan_dev(n, K), nan_dev(n)
        check(radial_call(kind, rd, n, K, alpha, cutoff, width, t, out))
        if kind in (2, 3):
            check(radial_grad_call(kind, rd, gd, n, K, alpha, cutoff, width, t, rows))
        return out, rows
    out, rows = twice(call)
    beyond = r >= cutoff
    assert float(out.cpu()[beyond].abs().max()) == 0.0
    (v64, ga64), (v32, ga32) = radial_reference(kind, r, g, K, cutoff, alpha, F64), radial_reference(kind, r, g, K, cutoff, alpha, F32)
    assert_sum(f"radial kind {kind}", out, v64, v32)
    if kind in (2, 3):
        assert float(rows.cpu()[beyond].abs().max()) == 0.0
        assert_sum(f"radial kind {kind} d/dalpha rows", rows, ga64, ga32)
    else:
        assert torch.isnan(rows).all()


def test_radial_basis_rejects():
    n, K, cutoff = 37, 12, 5.0
    rd, gd = radii(cutoff)[:n].to(DEV), rnd(torch.Generator().manual_seed(0), n, K).to(DEV)
    t = [x.to(DEV) for x in R.bernstein_tables(K, F32)]
    out, rows = nan_dev(n, K), nan_dev(n)
    for kind in (1, 4):                                               # no learnable parameter: no gradient entry
        rejected(lambda: radial_grad_call(kind, rd, gd, n, K, 0.5, cutoff, 1.0, t, rows), rows)
    for kind in (3, 4):
        for tt in ([t[0], None, t[2]], [t[0], t[1], None]):
            rejected(lambda: radial_call(kind, rd, n, K, 0.5, cutoff, 1.0, tt, out), out)
    for tt in ([t[0], None, t[2]], [t[0], t[1], None]):
        rejected(lambda: radial_grad_call(3, rd, gd, n, K, 0.5, cutoff, 1.0, tt, rows), rows)
    for kind in (0, 5):
        rejected(lambda: radial_call(kind, rd, n, K, 0.5, cutoff, 1.0, t, out), out)
    for kk, nn in ((0, n), (-1, n), (K, -1)):                         # K <= 0 and P < 0, as the Bernstein entry points reject them
        rejected(lambda: radial_call(3, rd, nn, kk, 0.5, cutoff, 1.0, t, out), out)
        rejected(lambda: radial_grad_call(3, rd, gd, nn, kk, 0.5, cutoff, 1.0, t, rows), rows)
        rejected(lambda: lib().nq_bernstein_rbf(P(rd), nn, kk, 0.5, cutoff, P(t[0]), P(t[1]), P(t[2]), P(out), st()), out)


# ---- activations ----------------------------------------------------------------------------------------------------------------------------------------
TINY = 1e-4
ACT_ROWS = 37


def act_params(F):
    """alpha [Fc] random; beta [Fc] cycling through positive, negative, tiny and exactly 0.  Fc = F, except that one feature (F = 1) is run once per class
    of beta: Fc = 4 columns, one launch each, compared as one array like the wider cases."""
    Fc = 4 if F == 1 else F
    rng = np.random.default_rng(F)
    cls = np.arange(Fc) % 4
    beta = np.select([cls == 0, cls == 1, cls == 2], [rng.uniform(0.5, 2.0, Fc), -rng.uniform(0.5, 2.0, Fc), np.full(Fc, TINY)], 0.0)
    alpha = rng.normal(size=Fc) + np.where(rng.normal(size=Fc) > 0, 0.5, -0.5)
    return torch.tensor(alpha.astype(np.float32)), torch.tensor(beta.astype(np.float32)), torch.tensor(cls)


def act_input(rows, Fc, seed):
    """x [rows, Fc] ~ 3 N(0, 1) with the rows 0..3 set to +30, -30, +90, -90 in every column (the softplus and sigmoid tails, both signs of beta x)."""
    gen = torch.Generator().manual_seed(seed)
    x = 3.0 * rnd(gen, rows, Fc)
    for i, v in enumerate((30.0, -30.0, 90.0, -90.0)):
        x[i] = v
    return x, rnd(gen, rows, Fc)


def launches(F, Fc):
    """Column ranges of the launches that cover the Fc columns with F features each."""
    return [slice(j, j + F) for j in range(0, Fc, F)]


def act_reference(kind, x, alpha, beta, gy, dtype):
    """y, gx and the per-row partials of dL/dalpha, dL/dbeta [rows, F] by autograd; at beta == 0 the shifted softplus is defined piecewise, so its d/dbeta is
    the limit (a x^2 / 8): the mean of the float64 derivative at beta = +1e-6 and -1e-6."""
    rows, F = x.shape
    xr = x.to(dtype).clone().requires_grad_(True)
    A, B = (t.to(dtype).expand(rows, F).clone().requires_grad_(True) for t in (alpha, beta))
    y = R.activation(kind, xr, A, B, dtype)
    gx, ga, gb = grads(y, [xr, A, B], gy.to(dtype))
    zero = beta == 0
    if kind == 1 and bool(zero.any()):
        lim = torch.zeros(rows, F, dtype=F64)
        for eps in (1e-6, -1e-6):
            Be = torch.where(zero, torch.tensor(eps, dtype=F64), beta.double()).expand(rows, F).clone().requires_grad_(True)
            ye = R.activation(1, x.double(), alpha.double().expand(rows, F), Be, F64)
            lim += 0.5 * grads(ye, [Be], gy.double())[0]
        gb = torch.where(zero, lim.to(dtype), gb)
    return y.detach(), gx, ga, gb


def check_act(tag, kind, x, alpha, beta, cls, gy, outs):
    """outs = (y, gx, ga_rows, gb_rows) [rows, F] from a kernel.  The beta = 1e-4 columns of the shifted softplus are compared on their own against the
    yardstick alone (module docstring); everything else through assert_sum."""
    ref64, ref32 = act_reference(kind, x, alpha, beta, gy, F64), act_reference(kind, x, alpha, beta, gy, F32)
    tiny = cls == 2
    for name, got, r64, r32 in zip(("y", "gx", "ga rows", "gb rows"), outs, ref64, ref32):
        got = got.cpu()
        assert not torch.isnan(got).any(), (tag, name)
        if kind == 1 and bool(tiny.any()):
            if name == "gx":
                assert_sum(f"{tag} {name} (beta 1e-4)", got[:, tiny], r64[:, tiny], r32[:, tiny])
            else:
                record(f"{tag} ssp beta=1e-4 {name}", *assert_yard(f"{tag} {name} (beta 1e-4)", got[:, tiny], r64[:, tiny], r32[:, tiny]))
            if bool((~tiny).any()):
                assert_sum(f"{tag} {name}", got[:, ~tiny], r64[:, ~tiny], r32[:, ~tiny])
        else:
            assert_sum(f"{tag} {name}", got, r64, r32)
    z = (beta == 0).nonzero().reshape(-1)
    if kind == 1 and len(z):                                          # the beta == 0 branch by its closed forms: 0.5 a x, 0.5 a, 0.5 x, a x^2 / 8 (times gy)
        xd, a, g = x.double()[:, z], alpha.double()[z], gy.double()[:, z]
        for got, want in zip(outs, (0.5 * a * xd, 0.5 * a * g, 0.5 * xd * g, a * xd * xd * g / 8)):
            assert rel(got.cpu()[:, z].double().numpy(), want.numpy()) < 1e-6, tag


def feature_act_run(kind, x, alpha, beta, gy, F):
    """nq_feature_act and its reverse on [rows, Fc] inputs, F features per launch; device outputs [rows, Fc]."""
    rows, Fc = x.shape
    cols = []
    for sl in launches(F, Fc):
        xd, ad, bd, gd = (t.contiguous().to(DEV) for t in (x[:, sl], alpha[sl], beta[sl], gy[:, sl]))

        def call():
            y, gx, ga, gb = (nan_dev(rows, F) for _ in range(4))
            check(lib().nq_feature_act(P(xd), P(ad), P(bd), rows, F, kind, P(y), st()))
            check(lib().nq_feature_act_backward(P(xd), P(ad), P(bd), P(gd), rows, F, kind, P(gx), P(ga), P(gb), st()))
            return y, gx, ga, gb
        cols.append(twice(call))
    return tuple(torch.cat(c, dim=1) for c in zip(*cols))


@pytest.mark.parametrize("F", [1, 7, 128])
@pytest.mark.parametrize("kind", [0, 1], ids=["swish", "ssp"])
def test_feature_act(kind, F):
    rows = ACT_ROWS
    assert (rows * F) % 256 != 0
    alpha, beta, cls = act_params(F)
    x, gy = act_input(rows, len(cls), 10 * F + kind)
    outs = feature_act_run(kind, x, alpha, beta, gy, F)
    check_act(f"act kind {kind} F {F}", kind, x, alpha, beta, cls, gy, outs)


@pytest.mark.parametrize("ncomp", [1, 9, 25])
@pytest.mark.parametrize("F", [1, 7, 128])
@pytest.mark.parametrize("kind", [0, 1], ids=["swish", "ssp"])
def test_packed_act0(kind, F, ncomp):
    rows = ACT_ROWS
    assert (rows * ncomp * F) % 256 != 0
    alpha, beta, cls = act_params(F)
    x0, g0 = act_input(rows, len(cls), 10 * F + kind)
    cols = []
    for sl in launches(F, len(cls)):
        gen = torch.Generator().manual_seed(ncomp)
        x, gy = rnd(gen, rows, ncomp, F), rnd(gen, rows, ncomp, F)
        x[:, 0], gy[:, 0] = x0[:, sl], g0[:, sl]
        xd, gd, ad, bd = x.to(DEV), gy.to(DEV), alpha[sl].contiguous().to(DEV), beta[sl].contiguous().to(DEV)

        def call():
            y, gx, part = nan_dev(rows, ncomp, F), nan_dev(rows, ncomp, F), nan_dev(2, rows * ncomp * F)
            ga, gb = part[0, :rows * F].view(rows, F), part[1, :rows * F].view(rows, F)      # partials: one row of F per packed row, nothing after them
            check(lib().nq_packed_act0(P(xd), P(ad), P(bd), rows, ncomp, F, kind, P(y), st()))
            check(lib().nq_packed_act0_backward(P(xd), P(ad), P(bd), P(gd), rows, ncomp, F, kind, P(gx), P(ga), P(gb), st()))
            torch.cuda.synchronize()
            assert torch.isnan(part[:, rows * F:]).all(), "partials written at the packed index"
            return y, gx, ga, gb
        y, gx, ga, gb = twice(call)
        assert torch.equal(bits(y[:, 1:]), bits(xd[:, 1:])) and torch.equal(bits(gx[:, 1:]), bits(gd[:, 1:]))      # every other component: a copy, both ways
        cols.append((y[:, 0], gx[:, 0], ga, gb))
    outs = tuple(torch.cat(c, dim=1) for c in zip(*cols))
    plain = feature_act_run(kind, x0, alpha, beta, g0, F)
    for name, a, b in zip(("y", "gx", "ga", "gb"), outs, plain):
        assert torch.equal(bits(a), bits(b)), (name, "scalar rows differ from nq_feature_act on the sliced input")
    check_act(f"packed kind {kind} F {F} ncomp {ncomp}", kind, x0, alpha, beta, cls, g0, outs)


# ---- gather / segment sum -------------------------------------------------------------------------------------------------------------------------------
def pair_index():
    """12 atoms; pairs sorted by the centre atom with 0 (an empty segment), 1 and 300 pairs among the counts; neighbours with repeats, atom 5 never one."""
    rng = np.random.default_rng(2)
    counts = np.array([3, 0, 300, 1, 7, 2, 0, 5, 9, 4, 1, 6])
    idx_i = np.repeat(np.arange(12), counts)
    idx_j = rng.choice([a for a in range(12) if a != 5], size=len(idx_i))
    return torch.tensor(idx_i), torch.tensor(idx_j), 12


@pytest.mark.parametrize("Cw", [1, 25 * 7, 128])
def test_gather_and_segment_sum(Cw):
    idx_i, idx_j, N = pair_index()
    npair = len(idx_i)
    gen = torch.Generator().manual_seed(Cw)
    x, g, base = rnd(gen, N, Cw), rnd(gen, npair, Cw), rnd(gen, N, Cw)
    ptr_i = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(idx_i, minlength=N).cumsum(0)])
    order_j = torch.argsort(idx_j, stable=True)                       # as phisnet.PairIndex builds them
    cnt_j = torch.bincount(idx_j, minlength=N)
    ptr_j = torch.cat([torch.zeros(1, dtype=torch.long), cnt_j.cumsum(0)])
    assert int(cnt_j[5]) == 0 and int(cnt_j.max()) > 1 and 300 in torch.bincount(idx_i, minlength=N).tolist()
    xd, gd, bd, jd, pid, pjd, od = (t.to(DEV) for t in (x, g, base, idx_j, ptr_i, ptr_j, order_j))

    def call():
        gat, s0, s1, sp = nan_dev(npair, Cw), nan_dev(N, Cw), nan_dev(N, Cw), nan_dev(N, Cw)
        check(lib().nq_gather_rows(P(xd), P(jd), npair, Cw, P(gat), st()))
        check(lib().nq_segment_sum(P(gd), None, P(pid), None, N, Cw, P(s0), st()))
        check(lib().nq_segment_sum(P(gd), None, P(pid), P(bd), N, Cw, P(s1), st()))
        check(lib().nq_segment_sum(P(gd), P(od), P(pjd), None, N, Cw, P(sp), st()))
        return gat, s0, s1, sp
    gat, s0, s1, sp = twice(call)
    assert torch.equal(bits(gat), bits(x[idx_j]))

    def seg(idx, dtype, start=None):
        out = torch.zeros(N, Cw, dtype=dtype) if start is None else start.to(dtype).clone()
        return out.index_add_(0, idx, g.to(dtype))
    assert_sum("segment sum", s0, seg(idx_i, F64), seg(idx_i, F32))
    assert_sum("segment sum + base", s1, seg(idx_i, F64, base), seg(idx_i, F32, base))
    assert_sum("segment sum through order", sp, seg(idx_j, F64), seg(idx_j, F32))
    empty = [1, 6]
    assert float(s0.cpu()[empty].abs().max()) == 0.0 and torch.equal(bits(s1[empty]), bits(base[empty])) and float(sp.cpu()[5].abs().max()) == 0.0
    # <gather(x), g> == <x, segment_sum(g)> on the kernel outputs in float64: every output element is a float32 chain of at most max(cnt_j) additions
    lhs, rhs = float((gat.cpu().double() * g.double()).sum()), float((x.double() * sp.cpu().double()).sum())
    bound = int(cnt_j.max()) * 2.0 ** -24 * float((x.double().abs()[idx_j] * g.double().abs()).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    out = nan_dev(N, Cw)
    rejected(lambda: lib().nq_segment_sum(P(gd), P(od), P(pjd), P(bd), N, Cw, P(out), st()), out)      # base is not supported together with order


# ---- spherical linear -----------------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def sph_splits(rows, order):
    """(splits per component, rows per split, every split holds rows) of the weight gradient: the host rule of nq_sph_linear_weight_grad."""
    ncomp = (order + 1) ** 2
    sps = max(1, min(768 // ncomp, cdiv(rows, 128)))
    kper = cdiv(cdiv(rows, sps), 32) * 32
    return sps, kper, cdiv(rows, kper) == sps


def sph_paths(rows, order, Fin, Fout, aligned=True):
    """Launch paths (forward, input gradient, weight gradient) by shape and alignment alone: 'gemm2' / 'gemm3' = batched tile launch, 'generic' = the
    row-mapped kernel.  Mirrors launch_batched / gemm2_ok and the split rule of csrc/gemm.hip (the 32-bit offset limits are far away at these sizes)."""
    ncomp = (order + 1) ** 2
    vec = Fin % 4 == 0 and Fout % 4 == 0              # operand rows, leading dimensions and component strides in whole float4s

    def tiles(N, K):
        return "gemm3" if cdiv(rows, 128) * cdiv(N, 128) * ncomp >= 192 and K % 16 == 0 else "gemm2"
    fwd = tiles(Fout, Fin) if vec and aligned else "generic"
    gin = tiles(Fin, Fout) if vec and aligned else "generic"
    gw = "gemm2" if vec and sph_splits(rows, order)[2] else "generic"      # partial slabs go to the scratch: the weights' alignment does not matter
    return fwd, gin, gw


def sph_data(rows, order, Fin, Fout, misaligned=False, seed=0):
    gen = torch.Generator().manual_seed(seed + rows + order)
    ncomp = (order + 1) ** 2
    x, gy = rnd(gen, rows, ncomp, Fin), rnd(gen, rows, ncomp, Fout)
    ws = [rnd(gen, Fout, Fin) / math.sqrt(Fin) for _ in range(order + 1)]
    return x, gy, ws, rnd(gen, Fout)


def weight_views(ws, misaligned):
    """Device copies of the weights; ``misaligned``: each a view that starts one float into a larger buffer."""
    out = []
    for w in ws:
        if misaligned:
            buf = torch.zeros(w.numel() + 4, device=DEV, dtype=F32)
            v = buf[1:1 + w.numel()].view(w.shape)
            v.copy_(w)
            assert v.data_ptr() % 16 == 4
        else:
            v = w.to(DEV)
            assert v.data_ptr() % 16 == 0
        out.append(v)
    return out


def nan_weight_views(ws, misaligned):
    out = []
    for w in ws:
        buf = nan_dev(w.numel() + 4)
        out.append(buf[1:1 + w.numel()].view(w.shape) if misaligned else buf[:w.numel()].view(w.shape))
    return out


GUARD = 4096


def sph_reference(x, gy, ws, bias, dtype):
    xr = x.to(dtype).clone().requires_grad_(True)
    wr = [w.to(dtype).clone().requires_grad_(True) for w in ws]
    br = None if bias is None else bias.to(dtype).clone().requires_grad_(True)
    y = R.sph_linear(xr, wr, br, dtype)
    got = grads(y, [xr, *wr] + ([] if br is None else [br]), gy.to(dtype))
    return y.detach(), got[0], got[1:1 + len(ws)], (None if br is None else got[-1])


def sph_run(x, gy, ws, bias, misaligned=False):
    """forward, input gradient and weight gradient (twice, bitwise equal), the scratch exactly as long as nq_sph_weight_grad_scratch_floats says and followed
    by a NaN guard inside the same tensor that must survive."""
    rows, ncomp, Fin = x.shape
    Fout, order = ws[0].shape[0], len(ws) - 1
    xd, gd = x.to(DEV), gy.to(DEV)
    wd = weight_views(ws, misaligned)
    bd = None if bias is None else bias.to(DEV)
    wp = host_ptrs(wd)
    nscr = int(lib().nq_sph_weight_grad_scratch_floats(rows, order, Fin, Fout))

    def call():
        y, gx = nan_dev(rows, ncomp, Fout), nan_dev(rows, ncomp, Fin)
        gws = nan_weight_views(ws, misaligned)
        gb = None if bias is None else nan_dev(Fout)
        scr = nan_dev(nscr + GUARD)
        check(lib().nq_sph_linear_forward(P(xd), wp, P(bd), P(y), rows, order, Fin, Fout, st()))
        check(lib().nq_sph_linear_input_grad(P(gd), wp, P(gx), rows, order, Fin, Fout, st()))
        check(lib().nq_sph_linear_weight_grad(P(gd), P(xd), host_ptrs(gws), P(gb), rows, order, Fin, Fout, P(scr), st()))
        torch.cuda.synchronize()
        assert torch.isnan(scr[nscr:]).all(), "the weight gradient wrote past nq_sph_weight_grad_scratch_floats"
        return (y, gx, *gws) + (() if gb is None else (gb,))
    outs = twice(call)
    return outs[0], outs[1], outs[2:3 + order], (None if bias is None else outs[-1])


def sph_compare(tag, x, gy, ws, bias, got, parts=("y", "gx", "gw", "gb")):
    y, gx, gws, gb = got
    (y64, gx64, gw64, gb64), (y32, gx32, gw32, gb32) = sph_reference(x, gy, ws, bias, F64), sph_reference(x, gy, ws, bias, F32)
    if "y" in parts:
        assert_sum(f"{tag} y", y, y64, y32)
    if "gx" in parts:
        assert_sum(f"{tag} gx", gx, gx64, gx32)
    for L in range(len(ws)):
        assert_sum(f"{tag} gW_{L}", gws[L].contiguous(), gw64[L], gw32[L])
    if bias is not None:
        assert_sum(f"{tag} gbias0", gb, gb64, gb32)
        assert_sum(f"{tag} gbias0 = column sums of the scalar rows", gb, gy[:, 0].double().sum(0), gy[:, 0].sum(0))


# name -> (rows, order, Fin, Fout, misaligned weights, the paths the case is there for)
SPH_CASES = {
    "a-gemm2": (37, 2, 12, 20, False, ("gemm2", "gemm2", "gemm2")),
    "b-gemm3": (900, 4, 16, 16, False, ("gemm3", "gemm3", "gemm2")),
    "c-generic": (37, 3, 7, 5, False, ("generic", "generic", "generic")),
    "d-fout-6": (37, 2, 8, 6, False, ("generic", "generic", "generic")),
    "e-misaligned": (37, 2, 12, 20, True, ("generic", "generic", "gemm2")),
    "f-orders-5-6": (5, 6, 4, 4, False, ("gemm2", "gemm2", "gemm2")),
    "g-empty-splits": (3841, 4, 8, 8, False, ("gemm2", "gemm2", "generic")),
}


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("name", list(SPH_CASES))
def test_sph_linear(name, with_bias):
    rows, order, Fin, Fout, misaligned, paths = SPH_CASES[name]
    assert sph_paths(rows, order, Fin, Fout, not misaligned) == paths
    if name == "b-gemm3":
        assert cdiv(rows, 128) * (order + 1) ** 2 == 200
    x, gy, ws, bias = sph_data(rows, order, Fin, Fout)
    bias = bias if with_bias else None
    got = sph_run(x, gy, ws, bias, misaligned)
    sph_compare(name, x, gy, ws, bias, got)
    if with_bias:                                                     # the bias reaches the scalar row only: without it every other row is bitwise the same
        y0 = sph_run(x, gy, ws, None, misaligned)[0]
        assert torch.equal(bits(got[0][:, 1:]), bits(y0[:, 1:])) and not torch.equal(bits(got[0][:, 0]), bits(y0[:, 0]))


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("rows,order,empty", [(3841, 4, True), (3840, 4, False), (1921, 6, True)])
def test_sph_linear_weight_grad_empty_splits(rows, order, empty, with_bias):
    """Rounding the rows per split up to 32 leaves trailing splits without rows (3841 rows at order 4: 30 splits of 160, 25 hold rows): the row-mapped
    launch must write those slabs and bias partials as zeros, because the reduction sums all of them.  The scratch starts as NaN."""
    Fin = Fout = 8
    sps, kper, full = sph_splits(rows, order)
    assert full == (not empty) and sph_paths(rows, order, Fin, Fout)[2] == ("generic" if empty else "gemm2")
    if rows == 3841:
        assert (sps, kper, cdiv(rows, kper)) == (30, 160, 25)
    x, gy, ws, bias = sph_data(rows, order, Fin, Fout)
    bias = bias if with_bias else None
    got = sph_run(x, gy, ws, bias)
    for t in (*got[2], *(() if got[3] is None else (got[3],))):
        assert not torch.isnan(t).any(), "a slab or bias partial without rows was left as the scratch held it"
    sph_compare(f"rows {rows} order {order}", x, gy, ws, bias, got)


def test_sph_linear_zero_rows():
    order, Fin, Fout = 3, 8, 12
    ws = [rnd(torch.Generator().manual_seed(L), Fout, Fin) for L in range(order + 1)]
    wd = weight_views(ws, False)
    dummy = torch.zeros(16, device=DEV)
    y, gx, gb, scr = nan_dev(64), nan_dev(64), nan_dev(Fout), nan_dev(GUARD)
    gws = nan_weight_views(ws, False)
    check(lib().nq_sph_linear_forward(P(dummy), host_ptrs(wd), P(gb), P(y), 0, order, Fin, Fout, st()))
    check(lib().nq_sph_linear_input_grad(P(dummy), host_ptrs(wd), P(gx), 0, order, Fin, Fout, st()))
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(gx).all() and torch.isnan(gb).all()      # nothing to write
    check(lib().nq_sph_linear_weight_grad(P(dummy), P(dummy), host_ptrs(gws), P(gb), 0, order, Fin, Fout, P(scr), st()))
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) == 0.0 for g in gws) and float(gb.abs().max()) == 0.0 and torch.isnan(scr).all()


def test_sph_linear_rejects():
    rows, order, Fin, Fout = 5, 2, 4, 4
    x, gy, ws, bias = sph_data(rows, order, Fin, Fout)
    xd, gd = x.to(DEV), gy.to(DEV)
    wd = weight_views(ws + ws + ws, False)                            # enough pointers for order 7
    y, gx, scr = nan_dev(rows * 64 * Fout), nan_dev(rows * 64 * Fin), nan_dev(1 << 16)
    gws = nan_weight_views(ws + ws + ws, False)
    holes = list(wd[:order + 1])
    holes[1] = None
    gholes = list(gws[:order + 1])
    gholes[2] = None

    def ptrs(ts):
        return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    for o, fi, w, gw in ((7, Fin, wd, gws), (order, 0, wd, gws), (order, Fin, holes, gholes)):
        rejected(lambda: lib().nq_sph_linear_forward(P(xd), ptrs(w), None, P(y), rows, o, fi, Fout, st()), y)
        rejected(lambda: lib().nq_sph_linear_input_grad(P(gd), ptrs(w), P(gx), rows, o, fi, Fout, st()), gx)
        rejected(lambda: lib().nq_sph_linear_weight_grad(P(gd), P(xd), ptrs(gw), None, rows, o, fi, Fout, P(scr), st()), scr, *[g for g in gws])


# ---- HamiltonianLoss ------------------------------------------------------------------------------------------------------------------------------------
def loss_reference(pred, target, scale, dtype):
    p = pred.to(dtype).clone().requires_grad_(True)
    loss = hblock_ref.hamiltonian_loss(p, target.to(dtype), torch.ones(len(pred), dtype=dtype))
    d = (p - target.to(dtype)).detach()
    stats = torch.stack([loss.detach(), torch.sqrt((d * d).mean()), d.abs().sum()])
    return stats, scale * torch.autograd.grad(loss, p)[0]


def loss_call(pd, td, total, scale, stats, grad, scr):
    return lib().nq_hamiltonian_loss(P(pd), P(td), total, scale, P(stats), P(grad), P(scr), st())


@pytest.mark.parametrize("total", [1, 255, 65537, 256 * 256 * 2 + 3])      # the last: a third pass of the 256 x 256 grid-stride loop
def test_hamiltonian_loss(total):
    gen = torch.Generator().manual_seed(total)
    pred, target = rnd(gen, total), rnd(gen, total)
    if total > 1:
        same = torch.arange(0, total, 7)
        target[same] = pred[same]                                     # d == 0 exactly: gradient 0, not +-1 / total
    pd, td, scale = pred.to(DEV), target.to(DEV), 0.25

    def call():
        stats, grad, scr = nan_dev(3), nan_dev(total), torch.full((512,), NAN, device=DEV, dtype=F64)
        check(loss_call(pd, td, total, scale, stats, grad, scr))
        stats_only, sentinel = nan_dev(3), nan_dev(total)
        check(loss_call(pd, td, total, scale, stats_only, None, torch.full((512,), NAN, device=DEV, dtype=F64)))      # grad_packed NULL: statistics only
        assert torch.isnan(sentinel).all()
        return stats, grad, stats_only
    stats, grad, stats_only = twice(call)
    assert torch.equal(bits(stats), bits(stats_only))
    (s64, g64), (s32, g32) = loss_reference(pred, target, scale, F64), loss_reference(pred, target, scale, F32)
    for i, name in enumerate(("loss", "rmse", "sum |d|")):
        assert_sum(name, stats[i:i + 1], s64[i:i + 1], s32[i:i + 1])
    assert_sum("gradient", grad, g64, g32)
    if total > 1:
        assert float(grad.cpu()[same].abs().max()) == 0.0 and float(g64[same].abs().max()) == 0.0


def test_hamiltonian_loss_zero_and_rejects():
    total = 255
    pd = rnd(torch.Generator().manual_seed(1), total).to(DEV)
    stats, grad, scr = nan_dev(3), nan_dev(total), torch.full((512,), NAN, device=DEV, dtype=F64)
    check(loss_call(pd, pd.clone(), total, 1.0, stats, grad, scr))    # pred == target everywhere: rmse = 0, the loss is 0 and the gradient all zeros, not NaN
    torch.cuda.synchronize()
    assert torch.equal(bits(stats), bits(torch.zeros(3))) and torch.equal(bits(grad), bits(torch.zeros(total)))
    stats, grad = nan_dev(3), nan_dev(total)
    rejected(lambda: loss_call(pd, pd, 0, 1.0, stats, grad, scr), stats, grad)
    rejected(lambda: loss_call(pd, pd, -3, 1.0, stats, grad, scr), stats, grad)
