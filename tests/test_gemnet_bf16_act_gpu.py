"""GemNet-OC "bf16_act" mode on the MI355X: the Dense-only activations are bf16 in memory.  The operator tests compare the new entry points BITWISE with the
existing bf16 kernels (already tested against float64 in test_gemnet_gpu.py): an output stored as bf16 is the fp32 kernel's output rounded to nearest even, a
bf16 input gives what the fp32-input kernel gives on the widened values.  The node and model tests pin which tensors are bf16, that the forward pass equals
"bf16" bit for bit, and that the gradients stay as close to the fp32 path as the "bf16" mode's do."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")

from tests.test_gemnet_gpu import FULL, SMALL, Data, _loss, build  # noqa: E402

BF = torch.bfloat16
# a last M tile of one row; N below a tile; odd N (rows only 2-byte aligned); one and many k-tiles; (257, 50, 32): N even but no multiple of 4
SHAPES = [(257, 48, 32), (257, 33, 32), (300, 200, 64), (1000, 512, 512), (257, 50, 32)]
SENTINEL = 12345.0
GUARD = 64


def _dev():
    return torch.device("cuda:0")


def _guarded(M, N, shift=0):
    """A bf16 [M, N] view between two sentinel regions; shift = 1 makes it only 2-byte aligned (an epilogue with wider stores must not take them then)."""
    buf = torch.full((GUARD + shift + M * N + GUARD,), SENTINEL, device=_dev(), dtype=BF)
    return buf, buf[GUARD + shift:GUARD + shift + M * N].view(M, N)


def _guards_intact(buf, M, N, shift=0):
    lo, hi = buf[:GUARD + shift], buf[GUARD + shift + M * N:]
    return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()) and hi.numel() == GUARD


def _operands(M, N, K, seed=0):
    from nabladft_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(seed)
    x, W, res = torch.randn(M, K, generator=g).to(_dev()), torch.randn(N, K, generator=g).to(_dev()), torch.randn(M, N, generator=g).to(_dev())
    Wb, WbT = torch.empty(N, K, device=_dev(), dtype=BF), torch.empty(K, N, device=_dev(), dtype=BF)
    _lib.check(_lib.load().nq_bf16_pack(_lib.ptr(W), N, K, _lib.ptr(Wb), _lib.ptr(WbT), _lib.stream_ptr()))
    return x, Wb, res


def _fwd_f32(x, Wb, res, alpha, beta):
    from nabladft_amd import _lib
    M, K = x.shape
    N = Wb.shape[0]
    pre, act = torch.empty(M, N, device=_dev()), torch.empty(M, N, device=_dev())
    _lib.check(_lib.load().nq_linear_forward_bf16(_lib.ptr(x), _lib.ptr(Wb), _lib.ptr(pre), _lib.ptr(act), None if res is None else _lib.ptr(res), alpha, beta,
                                                  M, N, K, _lib.stream_ptr()))
    return pre, act


def _fwd_out(x, Wb, res, alpha, beta, act_bf16, shift=0):
    """The new entry point; returns (pre, act, guards intact)."""
    from nabladft_amd import _lib
    M, K = x.shape
    N = Wb.shape[0]
    pbuf, pre = _guarded(M, N, shift)
    if act_bf16:
        abuf, act = _guarded(M, N, shift)
    else:
        act = torch.empty(M, N, device=_dev())
    _lib.check(_lib.load().nq_linear_forward_bf16_out(_lib.ptr(x), int(x.dtype == BF), _lib.ptr(Wb), _lib.ptr(pre), _lib.ptr(act), int(act_bf16),
                                                      None if res is None else _lib.ptr(res), alpha, beta, M, N, K, _lib.stream_ptr()))
    torch.cuda.synchronize()
    ok = _guards_intact(pbuf, M, N, shift) and (not act_bf16 or _guards_intact(abuf, M, N, shift))
    return pre, act, ok


CASES = [("res", 0.5, 0.25), ("nores", 0.0, 1.0 / 0.6)]          # asymmetric alpha / beta with a residual; the plain ScaledSiLU without


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_forward_bf16_outputs_are_the_rounded_f32_outputs(M, N, K):
    x, Wb, res = _operands(M, N, K)
    for name, alpha, beta in CASES:
        r = res if name == "res" else None
        pre32, act32 = _fwd_f32(x, Wb, r, alpha, beta)
        for shift in (0, 1):                                      # shift 1: outputs only 2-byte aligned
            pre, act, ok = _fwd_out(x, Wb, r, alpha, beta, True, shift)
            assert ok, ("guard overwritten", name, shift)
            assert torch.equal(pre, pre32.to(BF)), (name, shift)
            assert torch.equal(act, act32.to(BF)), (name, shift)
            pre, act, ok = _fwd_out(x, Wb, r, alpha, beta, False, shift)
            assert ok, ("guard overwritten", name, shift)
            assert torch.equal(pre, pre32.to(BF)) and torch.equal(act, act32), (name, shift)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_forward_bf16_a_operand_equals_f32_operand_rounded_in_staging(M, N, K):
    x, Wb, res = _operands(M, N, K, seed=1)
    xb = x.to(BF)
    for name, alpha, beta in CASES:
        r = res if name == "res" else None
        for act_bf16 in (True, False):
            pre_f, act_f, ok_f = _fwd_out(x, Wb, r, alpha, beta, act_bf16)
            pre_b, act_b, ok_b = _fwd_out(xb, Wb, r, alpha, beta, act_bf16)
            assert ok_f and ok_b, "guard overwritten"
            assert torch.equal(pre_f, pre_b) and torch.equal(act_f, act_b), (name, act_bf16)
        pre32, act32 = _fwd_f32(x, Wb, r, alpha, beta)             # and both equal the existing kernel
        assert torch.equal(pre_b, pre32.to(BF)) and torch.equal(act_b, act32), name


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_ssilu_backward_with_bf16_z(M, N, K):
    from nabladft_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(2)
    n = M * N
    zbuf = (3.0 * torch.randn(n + 1, generator=g)).to(_dev()).to(BF)
    gbuf = torch.randn(n + 1, generator=g).to(_dev())
    for shift in (0, 1):                                          # shift 1: unaligned pointers -> the one-element path
        z, gy = zbuf[shift:shift + n - shift], gbuf[shift:shift + n - shift]
        m = z.numel()
        ref = torch.empty(m, device=_dev())
        zf = z.float()
        _lib.check(lib.nq_gn_ssilu_backward(_lib.ptr(zf), _lib.ptr(gy.contiguous()), 0.7, m, _lib.ptr(ref), _lib.stream_ptr()))
        buf = torch.full((GUARD + shift + m + GUARD,), SENTINEL, device=_dev())
        out = buf[GUARD + shift:GUARD + shift + m]
        _lib.check(lib.nq_gn_ssilu_backward_bf16(_lib.ptr(z), _lib.ptr(gy), 0.7, m, _lib.ptr(out), _lib.stream_ptr()))
        assert torch.equal(out, ref), shift
        assert bool((buf[:GUARD + shift] == SENTINEL).all()) and bool((buf[GUARD + shift + m:] == SENTINEL).all()), "guard overwritten"


@pytest.mark.parametrize("M,N,K", SHAPES + [(5000, 64, 96)])          # the last one: more than one slab of the split over the rows
def test_weight_grad_with_bf16_x(M, N, K):
    from nabladft_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(3)
    gy, xb = torch.randn(M, N, generator=g).to(_dev()), torch.randn(M, K, generator=g).to(_dev()).to(BF)
    xf = xb.float()
    scr = torch.empty(int(lib.nq_weight_grad_bf16_scratch_bytes(M, N, K)), device=_dev(), dtype=torch.uint8)
    ref, a, b = (torch.empty(N, K, device=_dev()) for _ in range(3))
    _lib.check(lib.nq_linear_weight_grad_bf16(_lib.ptr(gy), _lib.ptr(xf), _lib.ptr(ref), M, N, K, _lib.ptr(scr), _lib.stream_ptr()))
    _lib.check(lib.nq_linear_weight_grad_bf16_x(_lib.ptr(gy), _lib.ptr(xb), _lib.ptr(a), M, N, K, _lib.ptr(scr), _lib.stream_ptr()))
    _lib.check(lib.nq_linear_weight_grad_bf16_x(_lib.ptr(gy), _lib.ptr(xb), _lib.ptr(b), M, N, K, _lib.ptr(scr), _lib.stream_ptr()))
    assert torch.equal(a, ref)
    assert torch.equal(a, b)                                        # fixed-order reduction
    exact = gy.to(BF).double().T @ xb.double()                      # and the reference kernel itself is sane at these (smaller) sizes
    assert (ref.double() - exact).abs().max() < 2e-6 * exact.abs().max() * (M ** 0.5)


def _saved_dtypes(fn, M, units):
    """dtypes of the [M, units] tensors the node saves for its backward pass."""
    seen = []

    def pack(t):
        if tuple(t.shape) == (M, units):
            seen.append(t.dtype)
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = fn()
    assert out.dtype == torch.float32 and tuple(out.shape) == (M, units)
    return sorted(seen, key=str)


def test_saved_tensors_are_bf16_only_where_the_shape_rule_holds():
    from nabladft_amd import gemnet_oc
    units = 64
    g = torch.Generator(device="cpu").manual_seed(4)
    W1, W2 = (torch.randn(units, units, generator=g).mul(units ** -0.5).to(_dev()).requires_grad_(True) for _ in range(2))
    gemnet_oc.set_gemm_precision("bf16_act")
    try:
        for M, n_bf in ((300, True), (100, False)):
            x = torch.randn(M, units, generator=g).to(_dev()).requires_grad_(True)
            res = _saved_dtypes(lambda: gemnet_oc._ResidualFn.apply(x, W1, W2), M, units)
            den = _saved_dtypes(lambda: gemnet_oc._DenseFn.apply(x, W1, True), M, units)
            if n_bf:
                assert res == [BF, BF, BF, torch.float32], res          # pre1, a1, pre2; x
                assert den == [BF, torch.float32], den                  # pre; x
            else:
                assert res == [torch.float32] * 4 and den == [torch.float32] * 2, (res, den)
        # the node's gradients follow the "bf16" mode's: same kernels on pre-activations that differ by one bf16 rounding (2^-9 relative, through silu' whose
        # slope is at most 1.1 / 0.6) -- far below the 5e-2 the mode documents for a whole model
        x = torch.randn(300, units, generator=g).to(_dev()).requires_grad_(True)
        grads = {}
        for mode in ("bf16", "bf16_act"):
            gemnet_oc.set_gemm_precision(mode)
            out = gemnet_oc._ResidualFn.apply(x, W1, W2)
            grads[mode] = (out.detach().clone(),) + torch.autograd.grad(out.square().sum(), (x, W1, W2))
        assert torch.equal(grads["bf16"][0], grads["bf16_act"][0])
        for a, b in zip(grads["bf16"][1:], grads["bf16_act"][1:]):
            assert float((a - b).norm() / a.norm()) < 5e-2
    finally:
        gemnet_oc.set_gemm_precision("f32")


class _Rep:
    pass


def _replicated(base, reps=8):
    """>= 256 rows per Dense product: copies of the small fixture's molecules, far apart (as test_bf16_weights_follow_in_place_optimizer_updates does)."""
    rep = _Rep()
    nmol = int(base.batch.max()) + 1
    rep.pos = torch.cat([base.pos + 50.0 * i for i in range(reps)])
    rep.z = base.z.repeat(reps)
    rep.batch = torch.cat([base.batch + nmol * i for i in range(reps)])
    cnt = torch.bincount(rep.batch)
    rep.ptr = torch.cat([cnt.new_zeros(1), cnt.cumsum(0)])
    rep.y = torch.zeros(nmol * reps, device=base.pos.device)
    rep.forces = torch.zeros_like(rep.pos)
    return rep


SMALL32 = dict(SMALL, emb_size_atom=64, emb_size_edge=64, emb_size_trip_in=32, emb_size_trip_out=32, emb_size_quad_in=32, emb_size_quad_out=32,
               emb_size_aint_in=32, emb_size_aint_out=32)          # contraction sizes that are multiples of 32 -> the bf16 kernels really run


def _three_modes(net, data, loss):
    """E, F and parameter gradients in "f32", "bf16" and "bf16_act"; in the new mode the backward pass runs twice over the same graph."""
    from nabladft_amd import gemnet_oc
    out = {}
    try:
        for mode in ("f32", "bf16", "bf16_act"):
            gemnet_oc.set_gemm_precision(mode)
            net.zero_grad(set_to_none=True)
            E, F = net(data)
            L = loss(E, F)
            L.backward(retain_graph=mode == "bf16_act")
            out[mode] = (E.detach().clone(), F.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
            if mode == "bf16_act":
                net.zero_grad(set_to_none=True)
                L.backward()
                out["again"] = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    finally:
        gemnet_oc.set_gemm_precision("f32")
        net.zero_grad(set_to_none=True)
    return out


@pytest.fixture(scope="module")
def model_runs():
    from nabladft_amd import gemnet_oc
    dev = _dev()
    runs = {}
    full = np.load(os.path.join(GOLD, "gemnet_full.npz"))
    data = Data(full, dev)
    runs["yaml"] = _three_modes(build(FULL, full, dev, False), data, lambda E, F: _loss(E, F, data))
    small = np.load(os.path.join(GOLD, "gemnet_small.npz"))
    rep = _replicated(Data(small, dev))
    torch.manual_seed(3)
    net = gemnet_oc.GemNetOC(**SMALL32).to(dev)
    runs["small_x8"] = _three_modes(net, rep, lambda E, F: ((E - 1.0) ** 2).mean().add((F ** 2).mean()))
    return runs


def _deviation(g, g0):
    num = sum(float(((g[k] - g0[k]) ** 2).sum()) for k in g0)
    den = sum(float((v ** 2).sum()) for v in g0.values())
    return (num / den) ** 0.5


@pytest.mark.parametrize("config", ["yaml", "small_x8"])
def test_model_forward_equals_bf16_and_gradients_stay_as_close_to_f32(model_runs, config):
    """Whole-gradient relative deviation from the "f32" gradients (that path is pinned to the reference's float64 run at 5e-5), measured on the MI355X:
        yaml (gemnet_full.npz):       d_bf16 = 1.201e-03, d_act = 1.210e-03
        small x 8 (gemnet_small.npz): d_bf16 = 6.506e-04, d_act = 6.537e-04
    Bound: d_act <= 2 d_bf16 -- the new mode adds one 2^-9-relative rounding per saved pre-activation and rounds the a1 operand of the small weight-gradient
    products, the same size as the two operand roundings every product already makes; independent errors of equal size add to sqrt(2), a wrong kernel is off by
    O(1) -- and d_act < 5e-2, the bound the "bf16" mode documents."""
    r = model_runs[config]
    E1, F1, g1 = r["bf16"]
    E2, F2, g2 = r["bf16_act"]
    assert torch.equal(E1, E2) and torch.equal(F1, F2)                  # the forward pass is bit-identical to "bf16"
    assert float((E1 - r["f32"][0]).abs().max()) > 0.0                  # ... and both really took the bf16 kernels
    assert set(g2) == set(r["again"]) == set(g1) == set(r["f32"][2])
    for k in g2:
        assert torch.equal(g2[k], r["again"][k]), k                     # fixed-order reductions, no atomics
    assert any(not torch.equal(g1[k], g2[k]) for k in g1)                # the backward pass really read rounded tensors
    d_bf16, d_act = _deviation(g1, r["f32"][2]), _deviation(g2, r["f32"][2])
    print(f"gemnet bf16_act [{config}]: d_bf16 = {d_bf16:.3e}  d_act = {d_act:.3e}")
    assert d_act <= 2.0 * d_bf16 and d_act < 5e-2, (d_bf16, d_act)


def test_bf16_act_weights_follow_in_place_optimizer_updates():
    """The assertions of test_bf16_weights_follow_in_place_optimizer_updates for the new mode: three AdamW steps through FlatParameters track the fp32 run."""
    from nabladft_amd import gemnet_oc
    from nabladft_amd.trainer import FlatParameters
    dev = _dev()
    rep = _replicated(Data(np.load(os.path.join(GOLD, "gemnet_small.npz")), dev))
    outs = {}
    for mode in ("f32", "bf16_act"):
        torch.manual_seed(3)
        net = gemnet_oc.GemNetOC(**SMALL32).to(dev)
        gemnet_oc.set_gemm_precision(mode)
        try:
            flat = FlatParameters(net.parameters())
            opt = torch.optim.AdamW([flat.flat], lr=1e-2, weight_decay=0)
            seq = []
            for _ in range(3):
                flat.zero_grad()
                E, F = net(rep)
                seq.append(E.detach().clone())
                ((E - 1.0) ** 2).mean().add((F ** 2).mean()).backward()
                opt.step()
            with torch.no_grad():
                seq.append(net(rep)[0].clone())
        finally:
            gemnet_oc.set_gemm_precision("f32")
        outs[mode] = seq
    f, b = outs["f32"], outs["bf16_act"]
    scale = float(f[0].abs().max()) + 1e-6
    assert float((b[0] - b[1]).abs().max()) > 1e-3 * scale and float((b[2] - b[3]).abs().max()) > 1e-4 * scale      # every step changed what the forward sees
    move = float((f[3] - f[0]).abs().max())
    assert move > 1e-2 * scale                                              # the three fp32 steps moved the energies visibly ...
    assert float((b[3] - f[3]).abs().max()) < 0.25 * move + 3e-2 * scale    # ... and the bf16_act run followed them (stale weights would stay at step 0)
