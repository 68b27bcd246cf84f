"""GPU: nabladft_amd.dense -- the shared autograd Functions are exactly the launcher sequence, for every combination of requested gradients.

Every comparison is bitwise (``bits``): ``dense.linear`` / ``dense.linear2`` / ``dense.Matmul`` against the launchers called directly through the C ABI into NaN-filled outputs, in
the order the Functions issue them (nq_linear_forward, nq_qh_act for SiLU', nq_linear_input_grad, nq_linear_weight_grad or nq_linear_weight_grad_bias).
Shapes: a single row, a row count that is no multiple of a tile, DimeNet++'s radial width (below one MFMA k-step) and a K / N pair that is no multiple of 64."""
import pytest
import torch

from tests.helpers import DEV, P, _release_copies, bits, check, lib, nan_dev, st  # noqa: F401  (_release_copies: autouse)

pytestmark = pytest.mark.gpu

ROWS = [1, 67, 272]
WIDTHS = [(6, 8), (96, 160)]


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def same(name, got, ref):
    assert got is not None, name
    assert got.shape == ref.shape and torch.equal(bits(got), bits(ref)), name


def scratch(M, N, K):
    return torch.empty(int(lib().nq_weight_grad_scratch_floats(M, N, K)) + 64, device=DEV, dtype=torch.float32)


def launch_linear(x, W, b, gy, silu):
    """-> (y, gx, gW, gb) of x W^T (+ b) (+ SiLU) from the launchers alone."""
    M, K = x.shape
    N = W.shape[0]
    pre, post = nan_dev(M, N), (nan_dev(M, N) if silu else None)
    check(lib().nq_linear_forward(P(x), P(W), P(b), P(pre), P(post), M, N, K, st()))
    gp = gy
    if silu:
        gp = nan_dev(M, N)
        check(lib().nq_qh_act(P(pre), P(gy), 0, 1.0, gy.numel(), P(gp), st()))
    gx, gW, gb, scr = nan_dev(M, K), nan_dev(N, K), None, scratch(M, N, K)
    check(lib().nq_linear_input_grad(P(gp), P(W), P(gx), M, N, K, 0, st()))
    if b is None:
        check(lib().nq_linear_weight_grad(P(gp), P(x), P(gW), M, N, K, P(scr), st()))
    else:
        gb = nan_dev(N)
        check(lib().nq_linear_weight_grad_bias(P(gp), P(x), P(gW), P(gb), M, N, K, P(scr), st()))
    torch.cuda.synchronize()
    return (post if silu else pre), gx, gW, gb


@pytest.mark.parametrize("K,N", WIDTHS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("fn", ["linear", "linear2"])
def test_linear_is_the_launcher_sequence(fn, bias, silu, M, K, N):
    """``dense.linear`` (one autograd node) and ``dense.linear2`` (the twice-differentiable pair): the same launches."""
    from nabladft_amd import dense
    x, W, gy = (rnd(s, *shape).to(DEV) for s, shape in ((1, (M, K)), (2, (N, K)), (4, (M, N))))
    b = rnd(3, N).to(DEV) if bias else None
    y_ref, gx_ref, gW_ref, gb_ref = launch_linear(x, W, b, gy, silu)

    def run(need_x, need_w, need_b=None):
        xs = x.clone().requires_grad_(need_x)
        Ws = W.clone().requires_grad_(need_w)
        bs = None if b is None else b.clone().requires_grad_(need_w if need_b is None else need_b)
        y = getattr(dense, fn)(xs, Ws, bs, silu)
        y.backward(gy)
        torch.cuda.synchronize()
        return y, xs.grad, Ws.grad, (None if bs is None else bs.grad)

    for need_x, need_w in ((True, True), (False, True), (True, False)):
        tag = f"bias={bias} silu={silu} M={M} K={K} N={N} need_x={need_x} need_w={need_w}"
        y, gx, gW, gb = run(need_x, need_w)
        same("y " + tag, y, y_ref)
        if need_x:
            same("gx " + tag, gx, gx_ref)
        else:
            assert gx is None, tag
        if need_w:
            same("gW " + tag, gW, gW_ref)
            if bias:
                same("gb " + tag, gb, gb_ref)
        else:
            assert gW is None and gb is None, tag
    if bias:                                               # a frozen weight under a trainable bias: the bias gradient of the same fused launch
        y, gx, gW, gb = run(True, False, True)
        assert gW is None
        same("y frozen W", y, y_ref), same("gx frozen W", gx, gx_ref), same("gb frozen W", gb, gb_ref)


@pytest.mark.parametrize("K,N", WIDTHS)
@pytest.mark.parametrize("M", ROWS)
def test_matmul_is_the_launcher_sequence_with_swapped_roles(M, K, N):
    """x [M, K] @ W [K, N]: forward through the input-gradient launcher, gx through the forward launcher, gW through the weight-gradient launcher on (x, g)."""
    from nabladft_amd import dense
    x, W, gy = (rnd(s, *shape).to(DEV) for s, shape in ((5, (M, K)), (6, (K, N)), (7, (M, N))))
    y_ref, gx_ref, gW_ref, scr = nan_dev(M, N), nan_dev(M, K), nan_dev(K, N), scratch(M, K, N)
    check(lib().nq_linear_input_grad(P(x), P(W), P(y_ref), M, K, N, 0, st()))
    check(lib().nq_linear_forward(P(gy), P(W), None, P(gx_ref), None, M, K, N, st()))
    check(lib().nq_linear_weight_grad(P(x), P(gy), P(gW_ref), M, K, N, P(scr), st()))
    xs, Ws = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    y = dense.Matmul.apply(xs, Ws)
    y.backward(gy)
    torch.cuda.synchronize()
    tag = f"M={M} K={K} N={N}"
    same("y " + tag, y, y_ref), same("gx " + tag, xs.grad, gx_ref), same("gW " + tag, Ws.grad, gW_ref)
