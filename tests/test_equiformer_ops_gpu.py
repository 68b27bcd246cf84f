"""The EquiformerV2 kernels of csrc/equiformer.hip one by one through the C ABI against float64 restatements of the same operation, built from the
kernel's own float32 inputs (promoted).  Every output buffer and every scratch buffer starts as NaN: an element a kernel never writes fails the
comparison, and so does a split-reduction partial that is never written (the backward reductions sum their scratch partials).

Bounds (the convention of test_gemnet_ops_gpu.py): copies / selections / single products are exact; every summing kernel must stay within
max(3 x the error of the same formula evaluated in float32 on the CPU, 2e-6) of the float64 value AND below 1e-5, both array-relative
(max |a - b| / max |b|).  Every summing kernel runs twice and must give bitwise equal results.

Branches and the tests that reach them:
  k_eq_ln_*: strided rows (test_layernorm[*-True-*]), W % 64 != 0, > 8192 rows (rows_per_chunk > 64: [8193-*], [20000-*]), mean offset 50
  k_eq_normsh_*: C = 1024 (16 wavefronts), C % 64 != 0, N % 4 != 0, lmax 1..6: test_norm_sh
  k_eq_logits_*: A > 64 or A % 64 != 0, E > 16384: test_logits; k_eq_softmax_*: in-degree 0 / 1 / 2 / 63..65 / 300, |logits| <= 100, ties: test_softmax
  k_eq_headscale*: nseg 1..8, H V up to 1024, grad_alpha NULL: test_head_scale; k_eq_scale: every NULL combination: test_scale"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from tests.helpers import (DEV, D, P, _lib, _release_copies, assert_sum, check, host_i32, host_ptrs, i32, lib, nan_dev, rejected, rnd,  # noqa: E402,F401
                           st, twice)                                  # (_release_copies: autouse)

EPS = 1e-5


def at(t, floats):
    """Device pointer ``floats`` elements into t (a row view that starts inside a wider tensor)."""
    return C.c_void_p(t.data_ptr() + 4 * floats)


# ---- torch.nn.LayerNorm over rows -----------------------------------------------------------------------------------------------------------------------
def ln_ref(x, w, b, gy, dt):
    x, w, b, gy = x.to(dt), w.to(dt), b.to(dt), gy.to(dt)
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS)
    xh = (x - mean) * rstd
    gh = gy * w
    gx = rstd * (gh - gh.mean(1, keepdim=True) - xh * (gh * xh).mean(1, keepdim=True))
    return xh * w + b, mean[:, 0], rstd[:, 0], gx, (gy * xh).sum(0), gy.sum(0)


# (rows, W, strided, mean offset): > 8192 rows makes rows_per_chunk > 64; strided rows are views into a wider tensor (x, y, grad_y and grad_x); the mean
# offset of 50 fails a one-pass variance (E[x^2] - E[x]^2 cancels 2500 against 2500 in float32)
LN_CASES = [(1, 64, False, 0.0), (3, 1, True, 0.0), (4, 63, False, 0.0), (5, 8, True, 0.0), (8192, 65, False, 0.0), (8193, 128, True, 0.0),
            (20000, 200, True, 50.0), (5, 200, False, 50.0), (4, 65, True, 0.0)]


@pytest.mark.parametrize("rows,W,strided,offset", LN_CASES)
def test_layernorm(rows, W, strided, offset):
    gen = torch.Generator().manual_seed(rows + W)
    c0, ws = (5, W + 13) if strided else (0, W)
    xb, gb = rnd(gen, rows, ws) * 1.3 + offset, rnd(gen, rows, ws)
    x, gy = xb[:, c0:c0 + W], gb[:, c0:c0 + W]
    w, b = rnd(gen, W), rnd(gen, W)
    xd, gd, wd, bd = xb.to(DEV), gb.to(DEV), D(w), D(b)

    def fwd():
        y, stats = nan_dev(rows, ws), nan_dev(rows, 2)
        check(lib().nq_eq_layernorm_forward(at(xd, c0), ws, wd, bd, rows, W, EPS, at(y, c0), ws, P(stats), st()))
        return y, stats
    y, stats = twice(fwd)
    nscr = lib().nq_eq_layernorm_scratch_floats(rows, W)

    def bwd():
        gx, gw, gbias = nan_dev(rows, ws), nan_dev(W), nan_dev(W)
        check(lib().nq_eq_layernorm_backward(at(xd, c0), ws, wd, at(gd, c0), ws, P(stats), rows, W, at(gx, c0), ws, P(gw), P(gbias), P(nan_dev(nscr)), st()))
        return gx, gw, gbias
    gx, gw, gbias = twice(bwd)
    r64, r32 = ln_ref(x, w, b, gy, torch.float64), ln_ref(x, w, b, gy, torch.float32)
    got = (y[:, c0:c0 + W], stats[:, 0], stats[:, 1], gx[:, c0:c0 + W], gw, gbias)
    for k, name in enumerate(("y", "mean", "rstd", "grad_x", "grad_weight", "grad_bias")):
        assert_sum(f"layernorm {name}", got[k], r64[k], r32[k])
    for t in (y, gx):                                                            # the columns outside the rows' views stay untouched
        assert torch.isnan(t[:, :c0]).all() and torch.isnan(t[:, c0 + W:]).all()


# ---- EquivariantLayerNormArraySphericalHarmonics ---------------------------------------------------------------------------------------------------------
def balance_weight(lmax):
    return torch.cat([torch.full((2 * l + 1,), 1.0 / (2 * l + 1) / lmax) for l in range(1, lmax + 1)])


def norm_sh_ref(x, w0, b0, aw, bw, gy, lmax, dt):
    """The nested norm_sh of oracle/equiformer_ref.forward (layer_norm.py:169-215) restated with an explicit LayerNorm on the l = 0 row; float64 autograd
    gives the four gradients.  Returns (y, mean, rstd, s, grad_x, grad_w0, grad_b0, grad_affine_weight)."""
    x, w0, b0, aw = (t.to(dt).requires_grad_(True) for t in (x, w0, b0, aw))
    expand = torch.tensor([l for l in range(1, lmax + 1) for _ in range(2 * l + 1)])
    x0 = x[:, 0:1]
    mean = x0.mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x0 - mean) ** 2).mean(2, keepdim=True) + EPS)
    out0 = (x0 - mean) * rstd * w0 + b0
    fn = (x[:, 1:] ** 2 * bw.to(dt).view(1, -1, 1)).sum(1, keepdim=True).mean(2, keepdim=True)
    s = (fn + EPS) ** -0.5
    y = torch.cat([out0, x[:, 1:] * s * aw[expand - 1].unsqueeze(0)], dim=1)
    (y * gy.to(dt)).sum().backward()
    return (y.detach(), mean.detach().view(-1), rstd.detach().view(-1), s.detach().view(-1), x.grad, w0.grad, b0.grad, aw.grad)


# (N, lmax, C): N not a multiple of atoms_per_block = 4; C = 1024 is 16 wavefronts (red[17]); C not a multiple of 64
NSH_CASES = [(1, 1, 1), (3, 2, 16), (4, 3, 63), (5, 4, 64), (37, 5, 65), (37, 6, 128), (5, 6, 1024), (3, 6, 1), (37, 3, 1024), (4, 1, 65), (5, 2, 200)]


@pytest.mark.parametrize("N,lmax,Cc", NSH_CASES)
def test_norm_sh(N, lmax, Cc):
    I = (lmax + 1) ** 2
    gen = torch.Generator().manual_seed(N * 10 + lmax + Cc)
    x, gy = rnd(gen, N, I, Cc), rnd(gen, N, I, Cc)
    x[:, 0] += 0.7
    w0, b0, aw, bw = rnd(gen, Cc), rnd(gen, Cc), rnd(gen, lmax, Cc), balance_weight(lmax)
    xd, gd, w0d, b0d, awd, bwd_ = D(x), D(gy), D(w0), D(b0), D(aw), D(bw)

    def fwd():
        y, stats = nan_dev(N, I, Cc), nan_dev(N, 3)
        check(lib().nq_eq_norm_sh_forward(xd, w0d, b0d, awd, bwd_, N, lmax, Cc, EPS, P(y), P(stats), st()))
        return y, stats
    y, stats = twice(fwd)
    nscr = lib().nq_eq_norm_sh_scratch_floats(N, lmax, Cc)

    def bwd():
        gx, gw0, gb0, gaw = nan_dev(N, I, Cc), nan_dev(Cc), nan_dev(Cc), nan_dev(lmax, Cc)
        check(lib().nq_eq_norm_sh_backward(xd, w0d, awd, bwd_, gd, P(stats), N, lmax, Cc, P(gx), P(gw0), P(gb0), P(gaw), P(nan_dev(nscr)), st()))
        return gx, gw0, gb0, gaw
    grads = twice(bwd)
    r64, r32 = norm_sh_ref(x, w0, b0, aw, bw, gy, lmax, torch.float64), norm_sh_ref(x, w0, b0, aw, bw, gy, lmax, torch.float32)
    got = (y, stats[:, 0], stats[:, 1], stats[:, 2]) + tuple(grads)
    for k, name in enumerate(("y", "mean", "rstd", "s", "grad_x", "grad_w0", "grad_b0", "grad_affine_weight")):
        assert_sum(f"norm_sh {name}", got[k], r64[k], r32[k])


def test_norm_sh_rejects_lmax_0_7_and_more_than_1024_channels():
    N = 2
    for lmax, Cc in [(0, 16), (7, 16), (2, 1025)]:
        I = (max(lmax, 1) + 1) ** 2
        x = torch.zeros(N, I * Cc, device=DEV)
        w = torch.zeros(max(lmax, 1) * Cc + I, device=DEV)
        y, stats = nan_dev(N, I * Cc), nan_dev(N, 3)
        rejected(lambda: lib().nq_eq_norm_sh_forward(P(x), P(w), P(w), P(w), P(w), N, lmax, Cc, EPS, P(y), P(stats), st()), y, stats)
        gx, g1, g2, g3, scr = nan_dev(N, I * Cc), nan_dev(Cc), nan_dev(Cc), nan_dev(max(lmax, 1) * Cc), nan_dev(64)
        rejected(lambda: lib().nq_eq_norm_sh_backward(P(x), P(w), P(w), P(w), P(x), P(w), N, lmax, Cc, P(gx), P(g1), P(g2), P(g3), P(scr), st()),
                 gx, g1, g2, g3)


# ---- attention logits -----------------------------------------------------------------------------------------------------------------------------------
def sleaky(x):
    return 0.6 * x + 0.4 * x * (2 * torch.sigmoid(x) - 1)


def dsleaky(x):
    s = torch.sigmoid(x)
    return 0.6 + 0.4 * ((2 * s - 1) + 2 * x * s * (1 - s))


def logits_ref(x, ad, gz, dt):
    x, ad, gz = x.to(dt), ad.to(dt), gz.to(dt)
    return (sleaky(x) * ad).sum(-1), gz[..., None] * ad * dsleaky(x), torch.einsum("eh,eha->ha", gz, sleaky(x))


# (E, H, A): A > 64 or not a multiple of 64; E > 16384 puts more than 64 edges in a chunk of the weight gradient
LOGIT_CASES = [(1, 8, 100), (63, 2, 65), (64, 8, 64), (65, 1, 1), (16385, 2, 8), (40000, 1, 65), (65, 8, 100), (64, 2, 1), (63, 1, 8)]


@pytest.mark.parametrize("E,H,A", LOGIT_CASES)
def test_logits(E, H, A):
    gen = torch.Generator().manual_seed(E + H * 7 + A)
    x, ad, gz = rnd(gen, E, H, A) * 2.0, rnd(gen, H, A), rnd(gen, E, H)
    xd, add, gzd = D(x), D(ad), D(gz)

    def fwd():
        z = nan_dev(E, H)
        check(lib().nq_eq_logits_forward(xd, add, E, H, A, P(z), st()))
        return (z,)
    z = twice(fwd)[0]
    nscr = lib().nq_eq_logits_scratch_floats(E, H, A)

    def bwd():
        gx, gad = nan_dev(E, H, A), nan_dev(H, A)
        check(lib().nq_eq_logits_backward(xd, add, gzd, E, H, A, P(gx), P(gad), P(nan_dev(nscr)), st()))
        return gx, gad
    gx, gad = twice(bwd)
    r64, r32 = logits_ref(x, ad, gz, torch.float64), logits_ref(x, ad, gz, torch.float32)
    for k, (name, got) in enumerate((("z", z), ("grad_x", gx), ("grad_alpha_dot", gad))):
        assert_sum(f"logits {name}", got, r64[k], r32[k])


# ---- softmax over the in-edges of every atom --------------------------------------------------------------------------------------------------------------
def softmax_case(H):
    """In-degrees 0, 1, 2, 63, 64, 65 and 300 (and a few more) in one CSR; logits in [-100, 100] (exp overflows float32 above 88.7 without the max
    shift), the 64-edge atom all tied, the 2-edge atom tied at its maximum, the 300-edge atom with several logits above 95."""
    degs = np.array([0, 1, 2, 63, 64, 65, 300, 0, 5, 1, 17, 2])
    ptr = np.concatenate([[0], np.cumsum(degs)])
    rng = np.random.default_rng(H)
    z = rng.uniform(-100.0, 100.0, size=(int(ptr[-1]), H)).astype(np.float32)
    z[ptr[4]:ptr[5]] = 37.5
    z[ptr[2]:ptr[3]] = 5.0
    z[ptr[6]:ptr[6] + 8] = rng.uniform(95.0, 100.0, size=(8, H))
    z[ptr[6] + 20:ptr[6] + 23] = 99.25                                           # ties at a large value
    return torch.tensor(z), ptr


def softmax_ref(z, ptr, dt):
    z = z.to(dt)
    seg = torch.repeat_interleave(torch.arange(len(ptr) - 1), torch.as_tensor(np.diff(ptr)))
    H = z.shape[1]
    mx = torch.full((len(ptr) - 1, H), -float("inf"), dtype=dt).scatter_reduce(0, seg.view(-1, 1).expand(-1, H), z, "amax", include_self=True)
    ex = (z - mx[seg]).exp()
    return ex / (torch.zeros(len(ptr) - 1, H, dtype=dt).index_add_(0, seg, ex)[seg] + 1e-16), seg      # torch_geometric.utils.softmax


@pytest.mark.parametrize("H", [1, 3])
def test_softmax(H):
    z, ptr = softmax_case(H)
    E, N = z.shape[0], len(ptr) - 1
    gy = rnd(torch.Generator().manual_seed(H), E, H)
    zd, pd, gyd = D(z), D(i32(ptr)), D(gy)

    def fwd():
        y = nan_dev(E, H)
        check(lib().nq_eq_softmax_forward(zd, pd, N, H, P(y), st()))
        return (y,)
    y = twice(fwd)[0]
    assert_sum("softmax", y, softmax_ref(z, ptr, torch.float64)[0], softmax_ref(z, ptr, torch.float32)[0])
    yk = y.cpu()
    tied = yk[ptr[4]:ptr[5]]
    assert torch.equal(tied, tied[:1].expand_as(tied))                           # exact ties give exactly equal weights
    yd = D(yk)

    def bwd():
        gz = nan_dev(E, H)
        check(lib().nq_eq_softmax_backward(yd, gyd, pd, N, H, P(gz), st()))
        return (gz,)
    gz = twice(bwd)[0]
    seg = softmax_ref(z, ptr, torch.float64)[1]
    refs = []
    for dt in (torch.float64, torch.float32):
        yy, gg = yk.to(dt), gy.to(dt)
        refs.append(yy * (gg - torch.zeros(N, H, dtype=dt).index_add_(0, seg, yy * gg)[seg]))
    assert_sum("softmax backward", gz, *refs)


# ---- messages times attention weights -------------------------------------------------------------------------------------------------------------------
# (H, V, rows of the blocks): nseg 1..8, H V = 8, 128, 1000, 1024
HS_CASES = [(1, 8, [3]), (8, 16, [2, 5, 1]), (8, 125, [7, 6, 6, 5, 5]), (4, 256, [1, 2, 1, 3, 1, 2, 1, 4]), (2, 4, [4, 9]), (1, 1024, [1] * 7),
            (2, 64, [3, 3, 3, 3, 3, 3])]


@pytest.mark.parametrize("with_grad_alpha", [True, False])
@pytest.mark.parametrize("H,V,rows", HS_CASES)
def test_head_scale(H, V, rows, with_grad_alpha):
    E, HV, k = 29, H * V, len(rows)
    gen = torch.Generator().manual_seed(HV + k)
    xs, gs, alpha = [rnd(gen, E, r * HV) for r in rows], [rnd(gen, E, r * HV) for r in rows], rnd(gen, E, H)
    xd, gd, ad = [t.to(DEV) for t in xs], [t.to(DEV) for t in gs], D(alpha)
    scale = lambda t, r: (t.reshape(E, r, H, V) * alpha.view(E, 1, H, 1)).reshape(E, -1)      # noqa: E731  (one float32 product per element)

    outs = [nan_dev(E, r * HV) for r in rows]
    check(lib().nq_eq_head_scale(k, host_i32(rows), host_ptrs(xd), None, ad, E, H, V, host_ptrs(outs), None, st()))
    for o, x_, r in zip(outs, xs, rows):
        assert torch.equal(o.cpu(), scale(x_, r))

    def bwd():
        douts, ga = [nan_dev(E, r * HV) for r in rows], nan_dev(E, H)
        check(lib().nq_eq_head_scale(k, host_i32(rows), host_ptrs(xd), host_ptrs(gd), ad, E, H, V, host_ptrs(douts), P(ga) if with_grad_alpha else None, st()))
        return tuple(douts) + (ga,)
    res = twice(bwd)
    for o, g_, r in zip(res[:-1], gs, rows):
        assert torch.equal(o.cpu(), scale(g_, r))
    if with_grad_alpha:
        refs = [sum((g_.to(dt) * x_.to(dt)).reshape(E, r, H, V).sum((1, 3)) for g_, x_, r in zip(gs, xs, rows)) for dt in (torch.float64, torch.float32)]
        assert_sum("head_scale grad_alpha", res[-1], *refs)
    else:
        assert torch.isnan(res[-1]).all()


def test_head_scale_rejects_wide_heads_and_nine_blocks():
    E = 3
    for H, V, k in [(1, 1025, 1), (2, 513, 2), (1, 8, 9)]:
        xs = [torch.zeros(E, H * V, device=DEV) for _ in range(k)]
        alpha = torch.zeros(E, H, device=DEV)
        outs = [nan_dev(E, H * V) for _ in range(k)]
        rejected(lambda: lib().nq_eq_head_scale(k, host_i32([1] * k), host_ptrs(xs), None, P(alpha), E, H, V, host_ptrs(outs), None, st()), *outs)


# ---- out = x * row_scale[row_index] * coef_scale ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_scale,row_index,coef_scale", [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)])
def test_scale(row_scale, row_index, coef_scale):
    N, I, Cc, n_src = 37, 16, 33, 11
    gen = torch.Generator().manual_seed(row_scale * 4 + row_index * 2 + coef_scale)
    x = rnd(gen, N, I, Cc)
    idx = torch.tensor(np.random.default_rng(0).integers(0, n_src, size=N), dtype=torch.int32)
    rs, cs = rnd(gen, n_src if row_index else N), rnd(gen, I)
    out = nan_dev(N, I, Cc)
    check(lib().nq_eq_scale(D(x), D(rs) if row_scale else None, D(idx) if row_index else None, D(cs) if coef_scale else None, N, I, Cc, P(out), st()))
    refs = []
    for dt in (torch.float32, torch.float64):
        f = torch.ones(N, I, 1, dtype=dt)
        if row_scale:
            f = f * rs.to(dt)[idx.long() if row_index else torch.arange(N)].view(N, 1, 1)
        if coef_scale:
            f = f * cs.to(dt).view(1, I, 1)
        refs.append(x.to(dt) * f)
    assert torch.equal(out.cpu(), refs[0])                                       # the kernel's two float32 products, in its order
    assert_sum("scale", out, refs[1], refs[0])
