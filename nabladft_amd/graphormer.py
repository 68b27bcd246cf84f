"""Graphormer3D on the HIP kernels of csrc/graphormer.hip, csrc/equiformer.hip (layer norm) and the fp32 MFMA GEMMs -- host-side mirror of the reference's
``nablaDFT.graphormer.Graphormer3D`` / ``Graphormer3DLightning`` (graphormer/graphormer_3d.py:227-321, :324-483; config/model/graphormer3d-small.yaml): same
constructor arguments, same module tree (``state_dict`` keys and shapes equal, so Graphormer3D-small checkpoints load), same initial distributions.

Ragged instead of padded: atoms [N] behind ``ptr``, all n_b^2 ordered pairs of molecule b behind ``pair_ptr``.  A padded key of the reference carries a -inf
bias, so real rows never read it, and padded query rows are masked out of the energy, the force loss and every gradient: on real atoms the reference IS this
function (tests/graphormer_ref.py pins that against the real class).  ``forward`` returns the reference's padded triple with ZEROS at padding (the reference
leaves unmasked values of padded rows there); ``forward_ragged`` returns ``(energy [B], forces [N, 3])``.

What runs where
  * pair featuriser (distances, unit vectors, Gaussian basis, its per-atom sum) forward and backward, the head-major bias layout, attention with the shared
    additive bias forward and backward, the rotational force head, exact GELU, the E -> 1 energy projection: csrc/graphormer.hip;
  * every nn.Linear: the GEMM launchers (dense.Linear); nn.LayerNorm: equiformer_v2._LayerNormFn; the atom embedding and the molecule sum:
    escn._EmbeddingFn / gemnet_oc._SegSumFn.
  * The attention bias is transposed once per forward into the head-major buffer all blocks x layers encoder applications and the force head read; its adjoint
    is accumulated IN PLACE by their backward kernels and transposed back once (``_BiasLayoutFn``).
  * Dropout: elementwise dropouts are torch.nn.functional.dropout between kernels; the attention-probability dropouts (``attention_dropout`` and the force
    head's fixed 0.1) are uint8 keep masks drawn by torch and handed to the kernels, so the kernels stay deterministic functions of their inputs.
    ``eval()`` is exactly dropout-free.  No CPU path.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, dense
from ._lib import _f32, _new, _st
from .equiformer_v2 import _LayerNormFn
from .escn import _EmbeddingFn, _inverse_lists
from .gemnet_oc import _SegSumFn
from .lightning import _HAVE_PL, _Task

ATOM_TYPES = 64
EDGE_TYPES = ATOM_TYPES * ATOM_TYPES
HEAD_DIMS = (16, 32)                       # built instances of the attention kernels
FORCE_HEAD_DROPOUT = 0.1                   # hard-coded in NodeTaskHead.forward (graphormer_3d.py:213)
ENERGY_DROPOUT = 0.1                       # graphormer_3d.py:311
_EMBED_CHUNK = 128


def max_molecule_atoms() -> int:
    return int(_lib.load().nq_g3d_max_mol_atoms())


# ---- the pair structure of a batch --------------------------------------------------------------------------------------------------------------------------
def check_atomic_numbers(z):
    """The reference indexes a 64-row embedding with z and a 4096-row one with 64 z_i + z_j; z = 0 is its padding value."""
    if z.numel() and (int(z.min()) <= 0 or int(z.max()) >= ATOM_TYPES):
        raise ValueError(f"Graphormer3D takes atomic numbers 1..{ATOM_TYPES - 1} (got {int(z.min())}..{int(z.max())})")


def build_plan(data):
    """ptr / pair_ptr / atom_mol, the edge types sorted once (for the 4096-bin gradients of gbf.mul / gbf.bias) and the inverse list of the atom embedding."""
    check_atomic_numbers(data.z)
    pos = data.pos
    if not pos.is_cuda:
        raise RuntimeError("nabladft_amd.Graphormer3D runs on MI355X only: tensors must be on a cuda (HIP) device")
    dev = pos.device
    ptr64 = getattr(data, "ptr", None)
    if ptr64 is None:
        counts = torch.bincount(data.batch)
        ptr64 = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    ptr64 = ptr64.to(dev).long()
    sizes = ptr64[1:] - ptr64[:-1]
    sizes_host = sizes.tolist()
    B, N = len(sizes_host), int(pos.shape[0])
    if B < 1 or min(sizes_host) < 1 or sum(sizes_host) != N:
        raise ValueError("Graphormer3D: every molecule needs at least one atom and ptr must cover all atoms")
    limit = max_molecule_atoms()
    if max(sizes_host) > limit:
        raise _lib.NablaqError(_lib.NQ_ERR_MOL_TOO_LARGE, f"a molecule of {max(sizes_host)} atoms exceeds the limit of {limit}")
    pair_ptr = torch.cat([sizes.new_zeros(1), (sizes * sizes).cumsum(0)])
    P = int(sum(n * n for n in sizes_host))
    mol = torch.arange(B, device=dev)
    atom_mol = torch.repeat_interleave(mol, sizes)
    pair_mol = torch.repeat_interleave(mol, sizes * sizes)
    local = torch.arange(P, device=dev) - pair_ptr[pair_mol]
    n_of = sizes[pair_mol]
    z = data.z.to(dev).long()
    et = z[ptr64[pair_mol] + local // n_of] * ATOM_TYPES + z[ptr64[pair_mol] + local % n_of]
    order = torch.sort(et, stable=True).indices.contiguous()
    type_ptr = torch.cat([et.new_zeros(1), torch.bincount(et, minlength=EDGE_TYPES).cumsum(0)]).contiguous()
    z32 = z.to(torch.int32).contiguous()
    # adjoint of the atom embedding in two fixed-order steps (atoms -> chunks of <= 128 atoms of one element -> the element): a one-step sum would leave one
    # thread per channel walking all atoms of an element
    z_order, z_ptr = _inverse_lists(z32, ATOM_TYPES)
    z_ptr64 = z_ptr.long()
    n_chunks = (z_ptr64[1:] - z_ptr64[:-1] + _EMBED_CHUNK - 1) // _EMBED_CHUNK
    chunk_ptr = torch.cat([n_chunks.new_zeros(1), n_chunks.cumsum(0)])
    chunk_z = torch.repeat_interleave(torch.arange(ATOM_TYPES, device=dev), n_chunks)
    total = int(chunk_z.numel())
    start = z_ptr64[chunk_z] + (torch.arange(total, device=dev) - chunk_ptr[chunk_z]) * _EMBED_CHUNK
    z_levels = [(z_order, torch.cat([start, start.new_full((1,), N)]).to(torch.int32).contiguous(), total), (None, chunk_ptr.to(torch.int32).contiguous(), ATOM_TYPES)]
    plan = SimpleNamespace(N=N, B=B, P=P, sizes=sizes_host, max_mol=max(sizes_host), ptr=ptr64.to(torch.int32).contiguous(), ptr64=ptr64,
                           pair_ptr=pair_ptr.contiguous(), atom_mol=atom_mol.to(torch.int32).contiguous(), atom_mol64=atom_mol, z=z32,
                           z_levels=z_levels, order=order, type_ptr=type_ptr, pos=_f32(pos))
    plan.geometry_key = _lib.geometry_key(data)
    return plan


def keep_mask(plan, H, p):
    """uint8 keep mask in the head-major bias layout and its scale 1 / (1 - p), drawn by torch (the current generator of the device)."""
    return (torch.rand(plan.P * H, device=plan.pos.device) >= p).to(torch.uint8), 1.0 / (1.0 - p)


# ---- autograd wrappers of csrc/graphormer.hip ------------------------------------------------------------------------------------------------------------------
class _PairFn(torch.autograd.Function):
    """(gbf [P, K], unit [P, 3], dist [P], efeat [N, K]) of the plan's positions; differentiable in the four GaussianLayer tensors only (nothing in this model
    differentiates with respect to positions)."""

    @staticmethod
    def forward(ctx, mul, bias, means, stds, plan):
        lib = _lib.load()
        mul, bias, means, stds = _f32(mul), _f32(bias), _f32(means), _f32(stds)
        K = means.numel()
        gbf, unit, dist, efeat = _new(plan.P, K, like=mul), _new(plan.P, 3, like=mul), _new(plan.P, like=mul), _new(plan.N, K, like=mul)
        _lib.check(lib.nq_g3d_pair_forward(_lib.ptr(plan.pos), _lib.ptr(plan.z), _lib.ptr(plan.ptr), _lib.ptr(plan.atom_mol), _lib.ptr(plan.pair_ptr), _lib.ptr(mul),
                                           _lib.ptr(bias), _lib.ptr(means), _lib.ptr(stds), plan.N, K, plan.max_mol, _lib.ptr(gbf), _lib.ptr(unit), _lib.ptr(dist),
                                           _lib.ptr(efeat), _st()))
        ctx.save_for_backward(mul, bias, means, stds, dist)
        ctx.plan = plan
        ctx.mark_non_differentiable(unit, dist)
        ctx.set_materialize_grads(False)
        return gbf, unit, dist, efeat

    @staticmethod
    def backward(ctx, g_gbf, _gu, _gd, g_efeat):
        lib = _lib.load()
        mul, bias, means, stds, dist = ctx.saved_tensors
        plan, K = ctx.plan, means.numel()
        if g_gbf is None and g_efeat is None:
            return None, None, None, None, None
        g_gbf = None if g_gbf is None else _f32(g_gbf)
        g_efeat = None if g_efeat is None else _f32(g_efeat)
        g_mul, g_bias, g_means, g_stds = torch.empty_like(mul), torch.empty_like(bias), torch.empty_like(means), torch.empty_like(stds)
        scr = _new(int(lib.nq_g3d_pair_scratch_floats(plan.N, plan.P, K)), like=mul)
        _lib.check(lib.nq_g3d_pair_backward(_lib.ptr(plan.pos), _lib.ptr(plan.z), _lib.ptr(plan.ptr), _lib.ptr(plan.atom_mol), _lib.ptr(plan.pair_ptr), _lib.ptr(mul),
                                            _lib.ptr(bias), _lib.ptr(means), _lib.ptr(stds), _lib.ptr(dist), _lib.ptr(plan.order), _lib.ptr(plan.type_ptr), plan.N, plan.P,
                                            K, _lib.ptr(g_gbf), _lib.ptr(g_efeat), _lib.ptr(g_means), _lib.ptr(g_stds), _lib.ptr(g_mul), _lib.ptr(g_bias), _lib.ptr(scr),
                                            _st()))
        return g_mul, g_bias, g_means, g_stds, None


class _BiasLayoutFn(torch.autograd.Function):
    """bias [P, H] -> (head-major buffer, token).  The buffer is not differentiable through autograd: its users add their adjoint IN PLACE into ``acc.grad`` (one
    buffer for all blocks x layers + 1 uses) and return a gradient for ``token`` instead, which makes this node wait for all of them; its backward then
    transposes the accumulated adjoint back once."""

    @staticmethod
    def forward(ctx, bias_pm, plan, acc):
        bias_pm = _f32(bias_pm)
        H = bias_pm.shape[1]
        hm = torch.empty(plan.P * H, device=bias_pm.device, dtype=torch.float32)
        _lib.check(_lib.load().nq_g3d_bias_to_heads(_lib.ptr(bias_pm), _lib.ptr(plan.ptr), _lib.ptr(plan.atom_mol), _lib.ptr(plan.pair_ptr), plan.N, H, _lib.ptr(hm),
                                                    _st()))
        ctx.meta = (plan, acc, H)
        ctx.mark_non_differentiable(hm)
        return hm, bias_pm.new_zeros(1)

    @staticmethod
    def backward(ctx, _ghm, _gtoken):
        plan, acc, H = ctx.meta
        if acc.grad is None:
            return None, None, None
        g = torch.empty(plan.P, H, device=acc.grad.device, dtype=torch.float32)
        _lib.check(_lib.load().nq_g3d_bias_from_heads(_lib.ptr(acc.grad), _lib.ptr(plan.ptr), _lib.ptr(plan.atom_mol), _lib.ptr(plan.pair_ptr), plan.N, H, _lib.ptr(g),
                                                      _st()))
        acc.grad = None
        return g, None, None


def _acc_buffer(acc, like):
    if acc.grad is None:
        acc.grad = torch.zeros_like(like)
    return acc.grad


class _AttentionFn(torch.autograd.Function):
    """graphormer_3d.py:40-59 between in_proj and out_proj: qkv [N, 3E] -> [N, E]."""

    @staticmethod
    def forward(ctx, qkv, token, bias_hm, acc, plan, H, scaling, mask, mask_scale):
        qkv = _f32(qkv)
        E = qkv.shape[1] // 3
        out, lse = _new(plan.N, E, like=qkv), _new(plan.N, H, like=qkv)
        _lib.check(_lib.load().nq_g3d_attention_forward(_lib.ptr(qkv), _lib.ptr(bias_hm), _lib.ptr(mask), mask_scale, _lib.ptr(plan.ptr), _lib.ptr(plan.pair_ptr), plan.B,
                                                        plan.N, H, E // H, plan.max_mol, scaling, _lib.ptr(out), _lib.ptr(lse), _st()))
        ctx.save_for_backward(qkv, out, lse)
        ctx.meta = (bias_hm, acc, plan, H, scaling, mask, mask_scale)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, out, lse = ctx.saved_tensors
        bias_hm, acc, plan, H, scaling, mask, mask_scale = ctx.meta
        E = out.shape[1]
        g = _f32(g)
        g_qkv, scr = torch.empty_like(qkv), _new(plan.N * H, like=qkv)
        _lib.check(_lib.load().nq_g3d_attention_backward(_lib.ptr(qkv), _lib.ptr(bias_hm), _lib.ptr(mask), mask_scale, _lib.ptr(plan.ptr), _lib.ptr(plan.pair_ptr), plan.B,
                                                         plan.N, H, E // H, plan.max_mol, scaling, _lib.ptr(out), _lib.ptr(lse), _lib.ptr(g), _lib.ptr(g_qkv),
                                                         _lib.ptr(_acc_buffer(acc, bias_hm)), _lib.ptr(scr), _st()))
        return g_qkv, g.new_zeros(1), None, None, None, None, None, None, None


class _ForceFn(torch.autograd.Function):
    """NodeTaskHead (graphormer_3d.py:202-224) after q_proj / k_proj / v_proj, the three E -> 1 projections folded in: qkv [N, 3E] -> forces [N, 3]."""

    @staticmethod
    def forward(ctx, qkv, W3, b3, token, bias_hm, acc, unit, plan, H, scaling, mask, mask_scale):
        qkv, W3, b3 = _f32(qkv), _f32(W3), _f32(b3)
        E = qkv.shape[1] // 3
        fh, lse, f = _new(plan.N, H, 3, like=qkv), _new(plan.N, H, like=qkv), _new(plan.N, 3, like=qkv)
        _lib.check(_lib.load().nq_g3d_force_forward(_lib.ptr(qkv), _lib.ptr(bias_hm), _lib.ptr(mask), mask_scale, _lib.ptr(unit), _lib.ptr(W3), _lib.ptr(b3),
                                                    _lib.ptr(plan.ptr), _lib.ptr(plan.pair_ptr), plan.B, plan.N, H, E // H, plan.max_mol, scaling, _lib.ptr(fh),
                                                    _lib.ptr(lse), _lib.ptr(f), _st()))
        ctx.save_for_backward(qkv, W3, fh, lse)
        ctx.meta = (bias_hm, acc, unit, plan, H, scaling, mask, mask_scale)
        return f

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        qkv, W3, fh, lse = ctx.saved_tensors
        bias_hm, acc, unit, plan, H, scaling, mask, mask_scale = ctx.meta
        E = W3.shape[1]
        g = _f32(g)
        g_qkv, g_W3, g_b3 = torch.empty_like(qkv), torch.empty_like(W3), _new(3, like=qkv)
        scr = _new(int(lib.nq_g3d_force_scratch_floats(plan.N, H, E // H)), like=qkv)
        _lib.check(lib.nq_g3d_force_backward(_lib.ptr(qkv), _lib.ptr(bias_hm), _lib.ptr(mask), mask_scale, _lib.ptr(unit), _lib.ptr(W3), _lib.ptr(plan.ptr),
                                             _lib.ptr(plan.pair_ptr), plan.B, plan.N, H, E // H, plan.max_mol, scaling, _lib.ptr(fh), _lib.ptr(lse), _lib.ptr(g),
                                             _lib.ptr(g_qkv), _lib.ptr(_acc_buffer(acc, bias_hm)), _lib.ptr(g_W3), _lib.ptr(g_b3), _lib.ptr(scr), _st()))
        return g_qkv, g_W3, g_b3, g.new_zeros(1), None, None, None, None, None, None, None, None


class _GeluFn(torch.autograd.Function):
    """F.gelu (exact, erf) of x [rows, C]."""

    @staticmethod
    def forward(ctx, x):
        x = _f32(x)
        y = torch.empty_like(x)
        _lib.check(_lib.load().nq_g3d_gelu_forward(_lib.ptr(x), None, x.shape[0], x.shape[1], _lib.ptr(y), _st()))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        _lib.check(_lib.load().nq_g3d_gelu_backward(_lib.ptr(x), None, _lib.ptr(_f32(g)), x.shape[0], x.shape[1], _lib.ptr(gx), _st()))
        return gx


class _RowDotFn(torch.autograd.Function):
    """nn.Linear(C, 1): x [rows, C], weight [1, C], bias [1] -> [rows, 1]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x, weight, bias = _f32(x), _f32(weight), _f32(bias)
        y = _new(x.shape[0], 1, like=x)
        _lib.check(_lib.load().nq_g3d_rowdot_forward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), x.shape[0], x.shape[1], _lib.ptr(y), _st()))
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, weight = ctx.saved_tensors
        rows, Cc = x.shape
        gx, gw, gb = torch.empty_like(x), torch.empty_like(weight), _new(1, like=x)
        scr = _new(int(lib.nq_g3d_rowdot_scratch_floats(rows, Cc)), like=x)
        _lib.check(lib.nq_g3d_rowdot_backward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(_f32(g)), rows, Cc, _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(scr), _st()))
        return gx, gw, gb


def _linear(mod, x):
    return dense.linear(x, mod.weight, mod.bias, False)


def _layer_norm(mod, x):
    return _LayerNormFn.apply(x, mod.weight, mod.bias, mod.eps)


# ---- the reference's module tree (parameter holders with its initialisation; the arithmetic is in Graphormer3D.forward_ragged) ------------------------------------
class SelfMultiheadAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.scaling = self.head_dim ** -0.5
        self.in_proj = nn.Linear(embed_dim, embed_dim * 3)
        self.out_proj = nn.Linear(embed_dim, embed_dim)


class Graphormer3DEncoderLayer(nn.Module):
    def __init__(self, embedding_dim, ffn_embedding_dim, num_attention_heads, dropout, attention_dropout, activation_dropout):
        super().__init__()
        self.dropout, self.attention_dropout, self.activation_dropout = dropout, attention_dropout, activation_dropout
        self.self_attn = SelfMultiheadAttention(embedding_dim, num_attention_heads, dropout=attention_dropout)
        self.self_attn_layer_norm = nn.LayerNorm(embedding_dim)
        self.fc1 = nn.Linear(embedding_dim, ffn_embedding_dim)
        self.fc2 = nn.Linear(ffn_embedding_dim, embedding_dim)
        self.final_layer_norm = nn.LayerNorm(embedding_dim)

    def forward(self, x, plan, bias):
        """graphormer_3d.py:95-116 on ragged rows x [N, E]; bias = (token, head-major buffer, accumulator)."""
        att, H = self.self_attn, self.self_attn.num_heads
        mask, scale = keep_mask(plan, H, self.attention_dropout) if self.training and self.attention_dropout > 0.0 else (None, 1.0)
        h = _AttentionFn.apply(_linear(att.in_proj, _layer_norm(self.self_attn_layer_norm, x)), bias[0], bias[1], bias[2], plan, H, att.scaling, mask, scale)
        x = x + F.dropout(_linear(att.out_proj, h), p=self.dropout, training=self.training)
        h = _GeluFn.apply(_linear(self.fc1, _layer_norm(self.final_layer_norm, x)))
        h = _linear(self.fc2, F.dropout(h, p=self.activation_dropout, training=self.training))
        return x + F.dropout(h, p=self.dropout, training=self.training)


class GaussianLayer(nn.Module):
    def __init__(self, K=128, edge_types=1024):
        super().__init__()
        self.K = K
        self.means, self.stds = nn.Embedding(1, K), nn.Embedding(1, K)
        self.mul, self.bias = nn.Embedding(edge_types, 1), nn.Embedding(edge_types, 1)
        nn.init.uniform_(self.means.weight, 0, 3)
        nn.init.uniform_(self.stds.weight, 0, 3)
        nn.init.constant_(self.bias.weight, 0)
        nn.init.constant_(self.mul.weight, 1)


class NonLinear(nn.Module):
    def __init__(self, input, output_size, hidden=None):
        super().__init__()
        hidden = input if hidden is None else hidden
        self.layer1 = nn.Linear(input, hidden)
        self.layer2 = nn.Linear(hidden, output_size)


class NodeTaskHead(nn.Module):
    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.q_proj, self.k_proj, self.v_proj = nn.Linear(embed_dim, embed_dim), nn.Linear(embed_dim, embed_dim), nn.Linear(embed_dim, embed_dim)
        self.scaling = (embed_dim // num_heads) ** -0.5
        self.force_proj1, self.force_proj2, self.force_proj3 = nn.Linear(embed_dim, 1), nn.Linear(embed_dim, 1), nn.Linear(embed_dim, 1)
        self.force_mask_p = FORCE_HEAD_DROPOUT            # tests set 0.0 to force an all-keep mask

    def forward(self, x, plan, bias, unit):
        qkv = dense.linear(x, torch.cat([self.q_proj.weight, self.k_proj.weight, self.v_proj.weight]),
                           torch.cat([self.q_proj.bias, self.k_proj.bias, self.v_proj.bias]), False)
        W3 = torch.cat([self.force_proj1.weight, self.force_proj2.weight, self.force_proj3.weight])
        b3 = torch.cat([self.force_proj1.bias, self.force_proj2.bias, self.force_proj3.bias])
        mask, scale = keep_mask(plan, self.num_heads, self.force_mask_p) if self.training and self.force_mask_p > 0.0 else (None, 1.0)
        return _ForceFn.apply(qkv, W3, b3, bias[0], bias[1], bias[2], unit, plan, self.num_heads, self.scaling, mask, scale)


class Graphormer3D(nn.Module):
    def __init__(self, blocks: int, layers: int, embed_dim: int, ffn_embed_dim: int, attention_heads: int, input_dropout: float, dropout: float,
                 attention_dropout: float, activation_dropout: float, num_kernel: int):
        super().__init__()
        if embed_dim % attention_heads or embed_dim // attention_heads not in HEAD_DIMS:
            raise NotImplementedError(f"head dimension embed_dim / attention_heads = {embed_dim / attention_heads:g}: the attention kernels are built for {HEAD_DIMS}")
        if not 1 <= num_kernel <= 256:
            raise NotImplementedError("num_kernel: 1..256 Gaussian kernels are built")
        self.blocks, self.atom_types, self.edge_types, self.K = blocks, ATOM_TYPES, EDGE_TYPES, num_kernel
        self.atom_encoder = nn.Embedding(self.atom_types, embed_dim, padding_idx=0)
        self.tag_encoder = nn.Embedding(3, embed_dim)
        self.input_dropout, self.energy_dropout = input_dropout, ENERGY_DROPOUT
        self.layers = nn.ModuleList([Graphormer3DEncoderLayer(embed_dim, ffn_embed_dim, attention_heads, dropout, attention_dropout, activation_dropout)
                                     for _ in range(layers)])
        self.final_ln = nn.LayerNorm(embed_dim)
        self.energy_proj = NonLinear(embed_dim, 1)
        self.energy_agg_factor = nn.Embedding(3, 1)
        nn.init.normal_(self.energy_agg_factor.weight, 0, 0.01)
        self.gbf = GaussianLayer(self.K, self.edge_types)
        self.bias_proj = NonLinear(self.K, attention_heads)
        self.edge_proj = nn.Linear(self.K, embed_dim)
        self.node_proj = NodeTaskHead(embed_dim, attention_heads)

    def prepare(self, data):
        """data.prepared = net.prepare(data): the pair structure and the edge-type sort, once per composition and geometry."""
        return build_plan(data)

    def _plan(self, data):
        plan = getattr(data, "prepared", None)
        if plan is None:
            return build_plan(data)
        if plan.N != int(data.pos.shape[0]):
            raise ValueError("data.prepared belongs to another batch")
        _lib.check_prepared(plan, data)
        return plan

    def forward_ragged(self, data, return_intermediates: bool = False):
        """-> (energy [B], forces [N, 3]) on real atoms."""
        plan = self._plan(data)
        g = self.gbf
        gbf, unit, _, efeat = _PairFn.apply(g.mul.weight, g.bias.weight, g.means.weight, g.stds.weight, plan)
        # tags are 1 on every real atom (graphormer_3d.py:277-280): row 1 of tag_encoder / energy_agg_factor
        x = _EmbeddingFn.apply(self.atom_encoder.weight, plan.z, plan.z_levels) + self.tag_encoder.weight[1] + _linear(self.edge_proj, efeat)
        x = F.dropout(x, p=self.input_dropout, training=self.training)
        bias_pm = _linear(self.bias_proj.layer2, _GeluFn.apply(_linear(self.bias_proj.layer1, gbf)))
        acc = SimpleNamespace(grad=None)
        hm, token = _BiasLayoutFn.apply(bias_pm, plan, acc)
        bias = (token, hm, acc)
        rec = dict(gbf=gbf, efeat=efeat, bias=bias_pm, layer_out=[]) if return_intermediates else None
        for _ in range(self.blocks):
            for layer in self.layers:
                x = layer(x, plan, bias)
                if rec is not None:
                    rec["layer_out"].append(x)
        out = _layer_norm(self.final_ln, x)
        h = F.dropout(out, p=self.energy_dropout, training=self.training)
        h = _GeluFn.apply(_linear(self.energy_proj.layer1, h))
        e_atom = _RowDotFn.apply(h, self.energy_proj.layer2.weight, self.energy_proj.layer2.bias) * self.energy_agg_factor.weight[1]
        energy = _SegSumFn.apply(e_atom, plan.ptr, plan.atom_mol, plan.B).reshape(plan.B)
        forces = self.node_proj(out, plan, bias, unit)
        self.last_plan = plan
        return (energy, forces, rec) if return_intermediates else (energy, forces)

    def forward(self, data):
        """The reference's triple: energy [B], node_output [B, n_max, 3] (zeros at padding), mask [B, n_max, 1]."""
        energy, forces = self.forward_ragged(data)
        dense, mask = to_dense(forces, self.last_plan)
        return energy, dense, mask.unsqueeze(-1)


def to_dense(x, plan):
    """Ragged rows [N, ...] -> ([B, n_max, ...] with zeros at padding, bool mask [B, n_max])."""
    local = torch.arange(plan.N, device=x.device) - plan.ptr64[plan.atom_mol64]
    dense = x.new_zeros((plan.B, plan.max_mol) + tuple(x.shape[1:]))
    mask = torch.zeros(plan.B, plan.max_mol, dtype=torch.bool, device=x.device)
    dense[plan.atom_mol64, local] = x
    mask[plan.atom_mol64, local] = True
    return dense, mask


class Graphormer3DLightning(_Task):
    """graphormer_3d.py:324-483.  The reference's force-loss semantics are kept: ``loss`` is applied to the PADDED dense [B, n_max, 3] tensors (:356-358), so a
    mean-reducing L1Loss divides by B * n_max * 3, padding zeros included.  ``forward`` / ``predict_step`` return ``(energy, forces [N, 3])``."""

    def __init__(self, model_name: str, net: nn.Module, optimizer, lr_scheduler, loss, metric, warmup_steps: int, energy_loss_coef: float,
                 forces_loss_coef: float) -> None:
        super().__init__()
        self.net, self.loss = net, loss
        self.loss_energy_coef, self.loss_forces_coef = energy_loss_coef, forces_loss_coef
        self._store_hparams(["net"], model_name=model_name, optimizer=optimizer, lr_scheduler=lr_scheduler, loss=loss, metric=metric, warmup_steps=warmup_steps,
                            energy_loss_coef=energy_loss_coef, forces_loss_coef=forces_loss_coef)

    def forward(self, data):
        return self.net.forward_ragged(data)

    def predict_step(self, data, **kwargs):
        return self(data)

    def step(self, batch, calculate_metrics: bool = False):
        energy, forces = self.net.forward_ragged(batch)
        plan = self.net.last_plan
        dense, _ = to_dense(forces, plan)
        target, _ = to_dense(batch.forces.to(forces.dtype), plan)
        loss = self.loss_forces_coef * self.loss(dense, target) + self.loss_energy_coef * self.loss(energy, batch.y)
        if calculate_metrics:
            return loss, self._calculate_metrics({"energy": energy, "forces": dense}, {"energy": batch.y, "forces": target})
        return loss

    def configure_optimizers(self):
        optimizer = self.hparams.optimizer(params=self.parameters())
        if self.hparams.lr_scheduler is None:
            return {"optimizer": optimizer}
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": self.hparams.lr_scheduler(optimizer=optimizer), "interval": "step", "frequency": 1}}

    def _log_current_lr(self):                  # LR is logged while global_step <= warmup_steps (:370-371)
        if _HAVE_PL and self.trainer.global_step <= self.hparams.warmup_steps:
            self.log("LR", self.optimizers().optimizer.param_groups[0]["lr"], logger=True)
