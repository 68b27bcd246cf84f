"""The f32 dense layer of the torch-side models on the fp32 MFMA GEMM launchers (nq_linear_*): the launch sequence, once.

  * raw helpers (``forward``, ``input_grad``, ``weight_grad``, ``silu_grad``, ``silu_grad2``): float32 contiguous tensors in, fresh tensors out, on the
    current stream.  Outside gemnet_oc.py's precision-aware helpers (bf16 by shape, bench hooks) nothing else calls these launchers;
  * ``Linear`` / ``linear``: x W^T (+ b) (+ SiLU in the GEMM epilogue), W [out, in] as torch.nn.Linear keeps it; ``Linear2`` / ``linear2``: the same on the
    same launches, differentiable twice (one more autograd node per backward);
  * ``Matmul``: x W with W [in, out] (e3nn's FullyConnectedNet layout).
"""
import torch

from . import _lib
from ._lib import _f32, _new, _st


# ---- the launches ---------------------------------------------------------------------------------------------------------------------------------------------
def forward(x, W, b=None, silu=False):
    """-> (pre, post): pre = x W^T (+ b), post = silu(pre) from the epilogue of the same launch (None unless ``silu``)."""
    M, K = x.shape
    N = W.shape[0]
    pre = _new(M, N, like=x)
    post = torch.empty_like(pre) if silu else None
    _lib.check(_lib.load().nq_linear_forward(_lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(pre), _lib.ptr(post), M, N, K, _st()))
    return pre, post


def input_grad(g, W):
    """g W."""
    M, N = g.shape
    K = W.shape[1]
    gx = _new(M, K, like=g)
    _lib.check(_lib.load().nq_linear_input_grad(_lib.ptr(g), _lib.ptr(W), _lib.ptr(gx), M, N, K, 0, _st()))
    return gx


def weight_grad(g, x, with_bias=False):
    """-> (g^T x, the column sums of g or None).  With the bias both come from one launch: the column sums are taken from the operand registers of the
    contraction (fixed order)."""
    lib = _lib.load()
    M, N = g.shape
    K = x.shape[1]
    gW = _new(N, K, like=g)
    scr = _new(int(lib.nq_weight_grad_scratch_floats(M, N, K)) + 64, like=g)
    if not with_bias:
        _lib.check(lib.nq_linear_weight_grad(_lib.ptr(g), _lib.ptr(x), _lib.ptr(gW), M, N, K, _lib.ptr(scr), _st()))
        return gW, None
    gb = _new(N, like=g)
    _lib.check(lib.nq_linear_weight_grad_bias(_lib.ptr(g), _lib.ptr(x), _lib.ptr(gW), _lib.ptr(gb), M, N, K, _lib.ptr(scr), _st()))
    return gW, gb


def silu_grad(pre, g):
    """g * silu'(pre)."""
    out = torch.empty_like(g)
    _lib.check(_lib.load().nq_qh_act(_lib.ptr(pre), _lib.ptr(g), 0, 1.0, g.numel(), _lib.ptr(out), _st()))
    return out


def silu_grad2(pre, g, a):
    """a = the adjoint of g * silu'(pre) -> (a * silu'(pre), a * g * silu''(pre))."""
    a_g, a_pre = torch.empty_like(pre), torch.empty_like(pre)
    _lib.check(_lib.load().nq_dnt_silu(_lib.ptr(pre), _lib.ptr(g), _lib.ptr(a), pre.numel(), _lib.ptr(a_g), _lib.ptr(a_pre), _st()))
    return a_g, a_pre


def only_tangents(what, *adjoints):
    """The second sweep of a backward Function builds the adjoints of its input gradients only."""
    if any(a is not None for a in adjoints):
        raise NotImplementedError(f"second sweep: an adjoint of {what} was asked for (a loss on parameter gradients); only losses on energies and forces are built")


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------------------------------
_FORCE_PASS = [False]      # set by DimeNetPlusPlusPotential.forward around its force call: that pass asks for the position gradient only, so the backward
#                            functions skip the parameter gradients (weight-gradient products, column sums) it would compute and drop


def _linear_forward(ctx, x, W, b, silu):
    x, W = _f32(x), _f32(W)
    b = None if b is None else _f32(b)
    pre, post = forward(x, W, b, silu)
    ctx.save_for_backward(x, W, pre if silu else x.new_zeros(0))
    ctx.silu, ctx.has_bias = silu, b is not None
    return pre, post


def _linear_backward(g, g_pre, x, W, pre, silu, has_bias, need_x, need_W):
    """(g, g_pre) -> (g, gp, gx, gW, gb) with gp = g silu'(pre) + g_pre: the launches of the first-order backward, for both Functions below."""
    g = None if g is None else _f32(g)
    gp = g
    if silu and x.shape[0] > 0 and g is not None:
        gp = silu_grad(pre, g)
    if g_pre is not None:
        gp = _f32(g_pre) if gp is None else gp + _f32(g_pre)
    gx = input_grad(gp, W) if need_x else None
    gW, gb = weight_grad(gp, x, has_bias) if need_W else (None, None)
    return g, gp, gx, gW, gb


class Linear(torch.autograd.Function):
    """torch.nn.Linear with or without bias, SiLU optionally fused into the GEMM epilogue; differentiable once.  One autograd node per layer: the models whose
    steps are bound by the host (PhiSNet: some hundred small layers per step) pay for every further node."""

    @staticmethod
    def forward(ctx, x, W, b, silu):
        pre, post = _linear_forward(ctx, x, W, b, silu)
        return post if silu else pre

    @staticmethod
    def backward(ctx, g):
        x, W, pre = ctx.saved_tensors
        need_x, need_W, need_b = ctx.needs_input_grad[:3]
        return (*_linear_backward(g, None, x, W, pre, ctx.silu, ctx.has_bias, need_x, need_W or need_b)[2:], None)


class Linear2(torch.autograd.Function):
    """The same layer, differentiable twice (DimeNet++'s force loss).  -> (y, pre): ``pre`` (None without SiLU) is an output only so that the second sweep can
    hand its adjoint back to this node; nothing else reads it.  The backward is a Function too (``_LinearBwd``) with the launches of ``Linear.backward``;
    under ``create_graph=False`` it records nothing."""

    @staticmethod
    def forward(ctx, x, W, b, silu):
        pre, post = _linear_forward(ctx, x, W, b, silu)
        ctx.set_materialize_grads(False)
        return (post, pre) if silu else (pre, None)

    @staticmethod
    def backward(ctx, g, g_pre):
        if g is None and g_pre is None:
            return None, None, None, None
        x, W, pre = ctx.saved_tensors
        need_x, need_W, need_b = ctx.needs_input_grad[:3]
        return (*_LinearBwd.apply(g, g_pre, x, W, pre, ctx.silu, ctx.has_bias, need_x, (need_W or need_b) and not _FORCE_PASS[0]), None)


class _LinearBwd(torch.autograd.Function):
    """(g, g_pre) -> (gx, gW, gb).  Second sweep, a_gx given: a_gp = a_gx W^T (the forward launcher), a_W = gp^T a_gx (the weight-gradient launcher), then
    a_g = a_gp silu'(pre) and a_pre = a_gp g silu''(pre), which returns to ``Linear2`` as the adjoint of its second output."""

    @staticmethod
    def forward(ctx, g, g_pre, x, W, pre, silu, has_bias, need_x, need_W):
        g, gp, gx, gW, gb = _linear_backward(g, g_pre, x, W, pre, silu, has_bias, need_x, need_W)
        ctx.save_for_backward(g if g is not None else x.new_zeros(0), gp, W, pre)
        ctx.silu, ctx.has = silu, (g is not None, g_pre is not None)
        ctx.set_materialize_grads(False)
        return gx, gW, gb

    @staticmethod
    def backward(ctx, a_gx, a_gW, a_gb):
        only_tangents("a weight gradient", a_gW, a_gb)
        out = [None] * 9
        if a_gx is None or a_gx.shape[0] == 0:
            return tuple(out)
        g, gp, W, pre = ctx.saved_tensors
        a_gx = _f32(a_gx)
        a_gp = forward(a_gx, W)[0]
        if ctx.needs_input_grad[3]:
            out[3] = weight_grad(gp, a_gx)[0]
        has_g, has_pre = ctx.has
        if has_pre:
            out[1] = a_gp
        if has_g:
            if ctx.silu:
                out[0], out[4] = silu_grad2(pre, g, a_gp)
            else:
                out[0] = a_gp
        return tuple(out)


def linear(x, W, b=None, silu=False):
    return Linear.apply(x, W, b, silu)


def linear2(x, W, b=None, silu=False):
    return Linear2.apply(x, W, b, silu)[0]


class Matmul(torch.autograd.Function):
    """y = x @ W, W [in, out]: the launchers with their roles swapped (the forward is the input-gradient product of W as a Linear weight)."""

    @staticmethod
    def forward(ctx, x, W):
        x, W = _f32(x), _f32(W)
        ctx.save_for_backward(x, W)
        return input_grad(x, W)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        g = _f32(g)
        return forward(g, W)[0], weight_grad(x, g)[0]
