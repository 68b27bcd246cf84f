"""The kernels around the PaiNN engine that every training step runs (csrc/node.hip), one entry point at a time through the C ABI on device buffers:
  nq_loss_l1_l2 / nq_loss_mse            k_loss<false / true>
  nq_adamw_step                          k_sqnorm_partial, k_sqnorm_final, k_adamw
  nq_scaled_silu, nq_geb_cat(_backward), nq_geb_gate(_backward)      the GatedEquivariantBlock pieces of the direct-force head
and one direct-force model on molecules of 1 / 5 / 12 atoms (the single atom keeps vec == 0 through the head).

References are plain torch restatements written here, run in float64; the same restatement in float32 on the CPU is the yardstick.  Bound
(tests.helpers.assert_sum, taken as it is): err <= max(3 x the float32 restatement's error, 2e-6) and err < 1e-5, err = max|got - ref64| / max|ref64|.
Outputs start as NaN (an element never written fails), every call runs twice into fresh buffers and must agree bitwise, refusals leave every buffer
untouched.  Every figure is printed; the worst per class goes to the suite's parity report, from which profiles/painn_periphery_parity.txt was taken.

AdamW.  The restatement is clip_grad_norm_ followed by torch.optim.AdamW (single tensor): bias corrections 1 - beta ** step in Python double in the
float32 run too, as torch takes them.  What is compared is the UPDATE p_after - p_before (and exp_avg, exp_avg_sq): lr = 1e-2 on parameters of size
1e-2, so that float32 resolves the update to 2e-7 of itself (parameters of order 1 would hide a step of order lr behind their own rounding) while
the decoupled decay lr * wd * p is still 1e-4 of it.  The C ABI takes lr, the betas and eps as float: the restatement is given the values that cross
it (beta2 = float32(0.999) = 0.99900001287...), so the comparison measures the kernels' arithmetic, not the rounding of the arguments.  With an
all-zero gradient and weight decay the update is lr * wd * p = 1e-4 |p|, below what float32 resolves in p: there the parameter itself is compared.
Measured on the MI355X while nq_adamw_impl still took the bias corrections in float32 (1 - powf(beta, step)): update error up to 3.95e-6 at step 2
and 3.43e-6 at step 3 against a bound of 2e-6 at every count, 4.9e-7 at step 1 (where the error of 1 - beta2 cancels against exp_avg_sq) and inside
at step 1000; with the corrections taken in double on the host the worst update error of all cases is 6.6e-7 (the float32 restatement: 5.5e-7).

Force head.  ScaledSiLU at z = 0, +-20, +-88, +-100 must stay finite; those inputs put max|ref| at 100 / 0.6, so the precision of ordinary
elements is measured on a second input without them.  Rows v1 == 0: the norm is exactly 0.0 and grad_v1 exactly 0.0 (the subgradient torch takes)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from oracle import painn_ref as R  # noqa: E402
from tests.helpers import (DEV, D, P, _release_copies, _report, assert_parity, assert_sum, bits, check, lib, nan_dev, rejected, rel, rnd, st,  # noqa: E402,F401
                           twice)

_TABLE = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    yield
    _report("train_ops: worst figure per class; err = max|kernel - ref64| / max|ref64|, own = the float32 restatement's err, bound = min(max(3 own, 2e-6), 1e-5)")
    _report(f"train_ops: {'class':22s} {'worst case':58s} {'err':>10s} {'own':>10s} {'bound':>10s}")
    for cls, (ratio, label, err, own, bound) in _TABLE.items():
        _report(f"train_ops: {cls:22s} {label:58s} {err:10.2e} {own:10.2e} {bound:10.2e}{'' if err <= bound else '  ABOVE'}")


class Measure:
    """Prints and records every figure, asserts (helpers.assert_sum) only at the end so that one figure above its bound does not hide the others."""

    def __init__(self):
        self.bad = []

    def __call__(self, cls, label, got, ref64, ref32):
        got, ref64, ref32 = got.detach().reshape(-1), ref64.detach().reshape(-1), ref32.detach().reshape(-1)
        err, own = rel(got.cpu().double().numpy(), ref64.numpy()), rel(ref32.double().numpy(), ref64.numpy())
        bound = min(max(3 * own, 2e-6), 1e-5)
        print(f"{cls:22s} {label:58s} err {err:.2e} own {own:.2e} bound {bound:.2e}{'' if err <= bound else '  ABOVE'}")
        ratio = err / bound if not math.isnan(err) else math.inf
        if cls not in _TABLE or ratio > _TABLE[cls][0]:
            _TABLE[cls] = (ratio, label, err, own, bound)
        try:
            assert_sum(label, got, ref64, ref32)
        except AssertionError as e:
            self.bad.append(str(e))

    def done(self):
        assert not self.bad, self.bad


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- loss -------------------------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1), (37, 1023), (1023, 1024), (1024, 1025), (1025, 4097), (2049, 1)]
COEFS = [(0.7, 1.3), (0.0, 1.0), (1.0, 0.0)]


def loss_ref(kind, E, y, F, Ft, ce, cf, dtype):
    """node.hip:300-301: L1 on the energies + the mean Euclidean norm of the force residual rows, or torch.nn.MSELoss on both; seeds by autograd."""
    E, F = E.to(dtype).requires_grad_(), F.to(dtype).requires_grad_()
    y, Ft = y.to(dtype), Ft.to(dtype)
    if kind == "mse":
        le, lf = torch.nn.MSELoss()(E, y), torch.nn.MSELoss()(F, Ft)
    else:
        le, lf = (E - y).abs().mean(), torch.linalg.vector_norm(F - Ft, dim=-1).mean()
    loss = ce * le + cf * lf
    gE, gF = torch.autograd.grad(loss, [E, F])
    return loss.detach().reshape(1), gE, gF


def loss_call(kind, E, y, F, Ft, ce, cf):
    B, N = E.numel(), F.shape[0]
    out, gE, gF = nan_dev(1), nan_dev(B), nan_dev(N, 3)
    fn = lib().nq_loss_mse if kind == "mse" else lib().nq_loss_l1_l2
    check(fn(D(E), D(y), B, D(F), D(Ft), N, ce, cf, P(out), P(gE), P(gF), st()))
    return [out, gE, gF]


def loss_inputs(B, N, seed, zeros=True):
    g = gen(seed)
    E, y, F, Ft = rnd(g, B) * 3.0, rnd(g, B) * 3.0, rnd(g, N, 3), rnd(g, N, 3)
    if zeros and B >= 3:
        y[::5] = E[::5]                                               # exact-zero energy residuals
    if zeros and N >= 3:
        Ft[::7] = F[::7]                                              # whole force rows with a zero residual
    return E, y, F, Ft


@pytest.mark.parametrize("ce,cf", COEFS)
@pytest.mark.parametrize("B,N", LOSS_SHAPES)
@pytest.mark.parametrize("kind", ["l1_l2", "mse"])
def test_loss(kind, B, N, ce, cf):
    E, y, F, Ft = loss_inputs(B, N, 100 + B + N)
    out, gE, gF = twice(lambda: loss_call(kind, E, y, F, Ft, ce, cf))
    r64, r32 = loss_ref(kind, E, y, F, Ft, ce, cf, torch.float64), loss_ref(kind, E, y, F, Ft, ce, cf, torch.float32)
    M = Measure()
    tag = f"{kind} B {B} N {N} coef ({ce}, {cf})"
    for name, got, a, b in zip(("loss", "grad_energy", "grad_forces"), (out, gE, gF), r64, r32):
        M("loss " + kind, f"{name} {tag}", got, a, b)
    assert torch.isfinite(gE).all() and torch.isfinite(gF).all() and torch.isfinite(out).all()
    ze, zf = (E == y), (F == Ft).all(dim=1)
    assert int(ze.sum()) == (len(range(0, B, 5)) if B >= 3 else 0) and int(zf.sum()) == (len(range(0, N, 7)) if N >= 3 else 0)
    assert (gE.cpu()[ze] == 0).all() and (gF.cpu()[zf] == 0).all()    # sign(0) = 0; the subgradient of the norm at 0
    assert (r64[1][ze] == 0).all() and (r64[2][zf] == 0).all()
    if ce == 0.0:
        assert (gE == 0).all()
    if cf == 0.0:
        assert (gF == 0).all()
    M.done()


@pytest.mark.parametrize("kind", ["l1_l2", "mse"])
def test_loss_all_residuals_zero(kind):
    """E == y and F == Ft everywhere, B = 1 and N = 1 included: loss and both seeds exactly 0.0 and finite."""
    for B, N in ((1, 1), (37, 1025)):
        E, _, F, _ = loss_inputs(B, N, 7, zeros=False)
        out, gE, gF = twice(lambda: loss_call(kind, E, E.clone(), F, F.clone(), 0.7, 1.3))
        for t in (out, gE, gF):
            assert (t == 0).all(), (kind, B, N)


def test_loss_refuses_null_arguments():
    E, y, F, Ft = loss_inputs(37, 100, 1)
    out, gE, gF = nan_dev(1), nan_dev(37), nan_dev(100, 3)
    for fn in (lib().nq_loss_l1_l2, lib().nq_loss_mse):
        for hole in range(7):
            a = [D(E), D(y), D(F), D(Ft), P(out), P(gE), P(gF)]
            a[hole] = None
            rejected(lambda: fn(a[0], a[1], 37, a[2], a[3], 100, 0.7, 1.3, a[4], a[5], a[6], st()), out, gE, gF)


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------------------------
f32 = lambda x: float(np.float32(x))                                  # noqa: E731  (what crosses the float ABI)
LR, B1, B2, EPS = f32(1e-2), f32(0.9), f32(0.999), f32(1e-8)
COUNTS = [1, 255, 256, 257, 65537, 100003]
MODES = ("none", "inactive", "active", "zero_grad")


def adamw_ref(p, g, m, v, step, max_norm, wd, dtype):
    """torch.nn.utils.clip_grad_norm_ (skipped for max_norm <= 0) + torch.optim.AdamW.step of one tensor, scalars as Python doubles."""
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    if max_norm > 0:
        g = g * torch.clamp(max_norm / (torch.linalg.vector_norm(g) + 1e-6), max=1.0)
    p = p * (1 - LR * wd)
    m = torch.lerp(m, g, 1 - B1)
    v = v * B2 + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + EPS
    return p - (LR / bc1) * (m / denom), m, v


def adamw_call(p, g, m, v, step, max_norm, wd, scratch=None):
    """One nq_adamw_step on device copies; returns the new (p, m, v)."""
    pd, md, vd = p.to(DEV).clone(), m.to(DEV).clone(), v.to(DEV).clone()
    scr = torch.zeros(512, device=DEV) if scratch is None else scratch
    check(lib().nq_adamw_step(P(pd), D(g), P(md), P(vd), p.numel(), max_norm, LR, B1, B2, EPS, wd, step, P(scr), st()))
    return pd, md, vd


def adamw_inputs(count, mode):
    g = gen(count)
    p0 = rnd(g, count) * 1e-2
    grads = [torch.zeros(count) if mode == "zero_grad" else rnd(g, count) * 0.05 for _ in range(3)]
    norms = [float(x.double().norm()) for x in grads]
    max_norm = {"none": 0.0, "inactive": 2.0 * max(norms), "active": 0.5 * min(norms), "zero_grad": 1.0}[mode]
    return p0, grads, f32(max_norm), norms


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", COUNTS)
def test_adamw_three_steps(count, mode, wd):
    """Steps 1, 2, 3 from zero state; kernel and restatements each carry their own state."""
    p0, grads, max_norm, norms = adamw_inputs(count, mode)
    if mode == "none" and wd > 0:
        max_norm = -1.0                                               # both spellings of "no clipping"
    wdf = f32(wd)

    def call():
        p, m, v = p0, torch.zeros(count), torch.zeros(count)
        out = []
        for t, g in enumerate(grads, 1):
            p, m, v = adamw_call(p, g, m, v, t, max_norm, wdf)
            out += [p, m, v]
        return out

    got = twice(call)
    M = Measure()
    s64, s32 = (p0, torch.zeros(count), torch.zeros(count)), (p0, torch.zeros(count), torch.zeros(count))
    before = p0
    for t, g in enumerate(grads, 1):
        n64, n32 = adamw_ref(*s64[:1], g, *s64[1:], t, max_norm, wdf, torch.float64), adamw_ref(*s32[:1], g, *s32[1:], t, max_norm, wdf, torch.float32)
        p, m, v = got[3 * (t - 1):3 * t]
        tag = f"count {count} {mode} wd {wd} step {t}"
        if mode == "zero_grad":
            assert (m == 0).all() and (v == 0).all()
            if wd == 0.0:
                assert torch.equal(bits(p), bits(p0))                 # scale 1, 0 / (0 + eps): nothing moves
            else:
                M("adamw decay only", f"param {tag}", p, n64[0], n32[0])
        else:
            M("adamw update", f"update {tag}", p.cpu().double() - before.double(), n64[0] - s64[0].double(), n32[0].double() - s32[0].double())
            M("adamw exp_avg", f"exp_avg {tag}", m, n64[1], n32[1])
            M("adamw exp_avg_sq", f"exp_avg_sq {tag}", v, n64[2], n32[2])
        assert torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all()
        if mode in ("inactive", "active"):
            assert (max_norm < norms[t - 1]) == (mode == "active")
        s64, s32, before = n64, n32, p.cpu()
    M.done()


@pytest.mark.parametrize("mode,wd", [("active", 0.01), ("none", 0.0)])
@pytest.mark.parametrize("count", [257, 100003])
def test_adamw_step_1000(count, mode, wd):
    """One step at step = 1000 from a given state (exp_avg_sq >= 0): bias corrections 0.632 and 1 - 1.7e-46."""
    g = gen(1000 + count)
    p0, grad, m0, v0 = rnd(g, count) * 1e-2, rnd(g, count) * 0.05, rnd(g, count) * 0.02, (rnd(g, count) * 0.03) ** 2
    max_norm = f32(0.5 * float(grad.double().norm())) if mode == "active" else 0.0
    p, m, v = twice(lambda: list(adamw_call(p0, grad, m0, v0, 1000, max_norm, f32(wd))))
    n64, n32 = adamw_ref(p0, grad, m0, v0, 1000, max_norm, f32(wd), torch.float64), adamw_ref(p0, grad, m0, v0, 1000, max_norm, f32(wd), torch.float32)
    M = Measure()
    tag = f"count {count} {mode} wd {wd} step 1000"
    M("adamw update", f"update {tag}", p.cpu().double() - p0.double(), n64[0] - p0.double(), n32[0].double() - p0.double())
    M("adamw exp_avg", f"exp_avg {tag}", m, n64[1], n32[1])
    M("adamw exp_avg_sq", f"exp_avg_sq {tag}", v, n64[2], n32[2])
    M.done()


def test_adamw_refuses():
    """step = 0, a negative step and NULL pointers: nothing written."""
    count = 257
    p, m, v, scr = nan_dev(count), nan_dev(count), nan_dev(count), nan_dev(512)
    g = rnd(gen(2), count)

    def call(step=1, **hole):
        a = dict(p=P(p), g=D(g), m=P(m), v=P(v), scr=P(scr))
        a.update(hole)
        return lib().nq_adamw_step(a["p"], a["g"], a["m"], a["v"], count, 1.0, LR, B1, B2, EPS, 0.01, step, a["scr"], st())

    rejected(lambda: call(step=0), p, m, v, scr)
    rejected(lambda: call(step=-1), p, m, v, scr)
    for k in ("p", "g", "m", "v", "scr"):
        rejected(lambda: call(**{k: None}), p, m, v, scr)


# ---- the direct-force head pieces -------------------------------------------------------------------------------------------------------------------
SILU_COUNTS = [1, 255, 256, 257, 100003]
SPECIAL_Z = [0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
HEAD_SHAPES = [(N, h) for N in (1, 7, 257) for h in (1, 32, 100)]


def scaled_silu_ref(z, gy, dtype):
    z = z.to(dtype).requires_grad_()
    out = torch.nn.functional.silu(z) * (1 / 0.6)                     # oracle/painn_ref.py: scaled_silu
    return out.detach(), torch.autograd.grad(out, z, gy.to(dtype))[0]


def scaled_silu_call(z, gy):
    fwd, bwd = nan_dev(z.numel()), nan_dev(z.numel())
    check(lib().nq_scaled_silu(D(z), None, P(fwd), z.numel(), st()))
    check(lib().nq_scaled_silu(D(z), D(gy), P(bwd), z.numel(), st()))
    return [fwd, bwd]


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("count", SILU_COUNTS)
def test_scaled_silu(count, special):
    g = gen(count)
    z, gy = rnd(g, count) * 3.0, rnd(g, count)
    if special:
        k = min(count, len(SPECIAL_Z))
        z[:k] = torch.tensor(SPECIAL_Z[:k])
    fwd, bwd = twice(lambda: scaled_silu_call(z, gy))
    assert torch.isfinite(fwd).all() and torch.isfinite(bwd).all()
    (f64, b64), (f32_, b32) = scaled_silu_ref(z, gy, torch.float64), scaled_silu_ref(z, gy, torch.float32)
    M = Measure()
    tag = f"count {count}{' with z = 0, +-20, +-88, +-100' if special else ''}"
    M("scaled_silu", f"forward {tag}", fwd, f64, f32_)
    M("scaled_silu", f"backward {tag}", bwd, b64, b32)
    M.done()


def geb_cat_ref(x, v1, gcat, dtype):
    x, v1 = x.to(dtype).requires_grad_(), v1.to(dtype).requires_grad_()
    cat = torch.cat([x, torch.norm(v1, dim=-2)], dim=-1)              # oracle/painn_ref.py: painn_output_head
    gx, gv1 = torch.autograd.grad(cat, [x, v1], gcat.to(dtype))
    return cat.detach(), gx, gv1


def geb_cat_call(x, v1, gcat):
    N, h = x.shape
    cat, gx, gv1 = nan_dev(N, 2 * h), nan_dev(N, h), nan_dev(N, 3, h)
    check(lib().nq_geb_cat(D(x), D(v1), N, h, P(cat), st()))
    check(lib().nq_geb_cat_backward(D(gcat), D(v1), N, h, P(gx), P(gv1), st()))
    return [cat, gx, gv1]


@pytest.mark.parametrize("N,h", HEAD_SHAPES)
def test_geb_cat(N, h):
    g = gen(10 * N + h)
    x, v1, gcat = rnd(g, N, h), rnd(g, N, 3, h), rnd(g, N, 2 * h)
    if N > 1:
        v1[::3] = 0.0                                                 # whole atoms with v1 == 0 (an atom without neighbours)
    if h > 1:
        v1[:, :, ::5] = 0.0                                           # and single channels
    if N * h == 1:
        v1[:] = 0.0                                                   # the only element
    zero = (v1 == 0).all(dim=1)
    cat, gx, gv1 = twice(lambda: geb_cat_call(x, v1, gcat))
    assert zero.any() and (N * h == 1 or not zero.all())
    assert (cat.cpu()[:, h:][zero] == 0).all()                        # the norm is 0.0
    assert torch.isfinite(gv1).all() and (gv1.cpu().permute(0, 2, 1)[zero] == 0).all()     # and its adjoint 0.0, not NaN
    assert torch.equal(bits(cat[:, :h]), bits(x)) and torch.equal(bits(gx), bits(gcat[:, :h]))  # copies
    r64, r32 = geb_cat_ref(x, v1, gcat, torch.float64), geb_cat_ref(x, v1, gcat, torch.float32)
    assert (r64[2].permute(0, 2, 1)[zero] == 0).all()
    M = Measure()
    for name, got, a, b in zip(("cat", "grad_x", "grad_v1"), (cat, gx, gv1), r64, r32):
        M("geb_cat", f"{name} N {N} h {h}", got, a, b)
    M.done()


def geb_gate_ref(o2, v2, gx, gv, dtype):
    o2, v2 = o2.to(dtype).requires_grad_(), v2.to(dtype).requires_grad_()
    xo, gate = torch.split(o2, v2.shape[-1], dim=-1)                  # oracle/painn_ref.py: painn_output_head
    vout, xout = gate.unsqueeze(1) * v2, torch.nn.functional.silu(xo) * (1 / 0.6)
    go2, gv2 = torch.autograd.grad([xout, vout], [o2, v2], [gx.to(dtype), gv.to(dtype)])
    return xout.detach(), vout.detach(), go2, gv2


def geb_gate_call(o2, v2, gx, gv):
    N, _, o = v2.shape
    xout, vout, go2, gv2 = nan_dev(N, o), nan_dev(N, 3, o), nan_dev(N, 2 * o), nan_dev(N, 3, o)
    check(lib().nq_geb_gate(D(o2), D(v2), N, o, P(xout), P(vout), st()))
    check(lib().nq_geb_gate_backward(D(o2), D(v2), D(gx), D(gv), N, o, P(go2), P(gv2), st()))
    return [xout, vout, go2, gv2]


@pytest.mark.parametrize("N,o", HEAD_SHAPES)
def test_geb_gate(N, o):
    g = gen(20 * N + o)
    o2, v2, gx, gv = rnd(g, N, 2 * o) * 2.0, rnd(g, N, 3, o), rnd(g, N, o), rnd(g, N, 3, o)
    v2[::3] = 0.0
    got = twice(lambda: geb_gate_call(o2, v2, gx, gv))
    r64, r32 = geb_gate_ref(o2, v2, gx, gv, torch.float64), geb_gate_ref(o2, v2, gx, gv, torch.float32)
    assert (got[1].cpu()[::3] == 0).all() and (got[2].cpu()[::3, o:] == 0).all()       # vec == 0: no vector output, no adjoint of the gate
    M = Measure()
    for name, t, a, b in zip(("xout", "vout", "grad_o2", "grad_v2"), got, r64, r32):
        assert torch.isfinite(t).all()
        M("geb_gate", f"{name} N {N} o {o}", t, a, b)
    M.done()


def test_head_pieces_refuse():
    """NULL pointers, negative N and h <= 0 (o <= 0): nothing written.  N = 0 and count = 0 are accepted and launch nothing."""
    N, h = 7, 32
    g = gen(3)
    x, v, w, gvec = rnd(g, N, h), rnd(g, N, 3, h), rnd(g, N, 2 * h), rnd(g, N, 3, h)
    a, b, c, d = nan_dev(N, 2 * h), nan_dev(N, h), nan_dev(N, 3, h), nan_dev(N, 3, h)
    L = lib()
    outs = (a, b, c, d)
    rejected(lambda: L.nq_scaled_silu(None, None, P(b), N * h, st()), *outs)
    rejected(lambda: L.nq_scaled_silu(D(x), None, None, N * h, st()), *outs)
    rejected(lambda: L.nq_scaled_silu(D(x), None, P(b), -1, st()), *outs)
    for n_, h_ in ((-1, h), (N, 0), (N, -4)):
        rejected(lambda: L.nq_geb_cat(D(x), D(v), n_, h_, P(a), st()), *outs)
        rejected(lambda: L.nq_geb_cat_backward(D(w), D(v), n_, h_, P(b), P(c), st()), *outs)
        rejected(lambda: L.nq_geb_gate(D(w), D(v), n_, h_, P(b), P(c), st()), *outs)
        rejected(lambda: L.nq_geb_gate_backward(D(w), D(v), D(x), D(gvec), n_, h_, P(a), P(c), st()), *outs)
    for hole in range(3):
        q = [D(x), D(v), P(a)]
        q[hole] = None
        rejected(lambda: L.nq_geb_cat(q[0], q[1], N, h, q[2], st()), *outs)
    for hole in range(4):
        q = [D(w), D(v), P(b), P(c)]
        q[hole] = None
        rejected(lambda: L.nq_geb_cat_backward(q[0], q[1], N, h, q[2], q[3], st()), *outs)
        rejected(lambda: L.nq_geb_gate(q[0], q[1], N, h, q[2], q[3], st()), *outs)
    for hole in range(6):
        q = [D(w), D(v), D(x), D(gvec), P(a), P(c)]
        q[hole] = None
        rejected(lambda: L.nq_geb_gate_backward(q[0], q[1], q[2], q[3], N, h, q[4], q[5], st()), *outs)
    check(L.nq_scaled_silu(D(x), None, P(b), 0, st()))
    check(L.nq_geb_cat(D(x), D(v), 0, h, P(a), st()))
    check(L.nq_geb_cat_backward(D(w), D(v), 0, h, P(b), P(c), st()))
    check(L.nq_geb_gate(D(w), D(v), 0, h, P(b), P(c), st()))
    check(L.nq_geb_gate_backward(D(w), D(v), D(x), D(gvec), 0, h, P(a), P(c), st()))
    torch.cuda.synchronize()
    for t in outs:
        assert torch.isnan(t).all()


# ---- one model: the head on an atom without neighbours ----------------------------------------------------------------------------------------------
def test_direct_force_model_with_single_atom_molecule():
    """direct_forces=True, F = 64, L = 2 on molecules of 1, 5 and 12 atoms: the single atom has no neighbour, its vec stays 0 through both gated
    blocks (norm 0 in k_geb_cat, the nr > 0 guard in k_geb_cat_rev).  Reference: oracle/painn_ref.py: train_step in float64 (it covers the direct-force
    head), its float32 run the yardstick; energy, forces and every parameter gradient finite and inside helpers.assert_parity."""
    import nabladft_amd as nq
    cfg = R.PaiNNConfig(hidden_channels=64, num_layers=2, num_rbf=20, cutoff=4.0, max_neighbors=100, direct_forces=True)
    params = R.make_params(cfg, seed=17)
    rng = np.random.Generator(np.random.PCG64(17))
    sizes = [1, 5, 12]
    pos = torch.tensor(np.concatenate([rng.uniform(0, 1.3 * n ** (1 / 3) + 0.8, size=(n, 3)) for n in sizes]).astype(np.float32))
    z = torch.tensor(rng.integers(1, 10, size=sum(sizes)))
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    y, ft = torch.tensor(rng.normal(size=3).astype(np.float32)), torch.tensor(rng.normal(size=(sum(sizes), 3)).astype(np.float32))
    edge_index, nbrs, _ = R.build_graph(pos, batch, cfg.cutoff, cfg.max_neighbors)
    assert nbrs.tolist()[0] == 0 and min(nbrs.tolist()[1:]) > 0
    ref = {}
    for dtype in (torch.float64, torch.float32):
        Pd = {k: v.to(dtype) for k, v in params.items()}
        ref[dtype] = R.train_step(Pd, cfg, pos.to(dtype), z, batch, y.to(dtype), ft.to(dtype), edge_index)
    e64, f64, l64, g64 = ref[torch.float64]
    e32, f32_, l32, g32 = ref[torch.float32]
    assert (f64[0] == 0).all() and all(torch.isfinite(g).all() for g in g64.values())      # vec == 0: no direct force on the lone atom

    model = nq.PaiNN(cfg.hidden_channels, cfg.num_layers, cfg.num_rbf, cfg.cutoff, cfg.max_neighbors, {"name": cfg.rbf},
                     {"name": "polynomial", "exponent": cfg.envelope_exponent}, True, True, False, True, cfg.num_elements)
    missing, unexpected = model.load_state_dict(params, strict=False)
    assert list(missing) == ["radial_basis.rbf.offset"] and not unexpected
    model.to(DEV).train()
    b = nq.Batch(pos, z, batch, y, ft).to(DEV)
    energy, forces = model(b)
    loss = torch.nn.L1Loss()(energy, b.y) + nq.L2Loss()(forces, b.forces)
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    assert list(grads) == list(g64)
    assert torch.isfinite(energy).all() and torch.isfinite(forces).all() and all(torch.isfinite(g).all() for g in grads.values())
    assert (forces[0] == 0).all()
    bad = []
    for name, got, a, b_ in [("energy", energy, e64, e32), ("forces", forces, f64, f32_), ("loss", loss.reshape(1), l64.reshape(1), l32.reshape(1))] + \
                            [("grad " + k, grads[k], g64[k], g32[k]) for k in grads]:
        try:
            err, own = assert_parity(f"train_ops direct-force [1, 5, 12] {name}", got.detach().cpu().numpy(), a.numpy(), b_.numpy())
            print(f"{name:60s} err {err:.2e} own {own:.2e}")
        except AssertionError as e:
            print(f"{name:60s} ABOVE {e}")
            bad.append(str(e))
    assert not bad, bad
