"""DimeNet++ on the HIP kernels of csrc/dimenet.hip and the fp32 MFMA GEMMs -- host-side mirror of the reference's ``DimeNetPlusPlusPotential`` /
``DimeNetPlusPlusLightning`` (dimenetplusplus/dimenetplusplus.py:22-113, :116-270; config/model/dimenetplusplus.yaml).

The wrapper (head, forces = -d prediction / d pos, post-processing, Lightning task) is pinned against the reference.  The core the reference imports from
torch-geometric (``torch_geometric.nn.models.DimeNetPlusPlus``, 2.4.0) is not part of the reference tree: it is RESTATED here and in tests/dimenet_ref.py
(DESIGN_details.md "DimeNet++"), with the same module tree, so ``state_dict`` keys and shapes are those of the reference class.

What runs where
  * edge geometry and its adjoint, the float64 radial basis / radial table of the spherical basis, the triplet product (no [T, .] array, no triplet index
    list), x * gate, the output block's gated in-edge sum, the embedding block's gather + SiLU: csrc/dimenet.hip (``nq_dn_*``);
  * every Linear (+ SiLU in the epilogue): dense.Linear2 on the GEMM launchers; the atom embedding: escn._EmbeddingFn; the molecule sum: gemnet_oc._SegSumFn;
  * forces: ONE ``torch.autograd.grad`` through the backward functions of these kernels.  Each of them is differentiable once more (the tangent kernels
    ``nq_dnt_*``), so with ``create_graph=True`` the forces carry the graph of the parameters and a loss on them trains: ``DimeNetPlusPlusForceLightning``.
    ``DimeNetPlusPlusLightning.training_step`` keeps refusing ``forces_loss_coef != 0``.  No CPU path.
"""
import math
from types import SimpleNamespace

import ctypes as C
import numpy as np
import torch
from torch import nn

from . import _lib, dense
from ._lib import _f32, _new, _st
from .escn import _EmbeddingFn, _inverse_lists
from .gemnet_oc import _SegSumFn
from .lightning import _Task

NUM_ELEMENTS = 95
INT_EMB_SIZES = (64, 128, 192, 256)        # one lane per channel of the triplet kernels, up to 4 registers per lane
MAX_SPHERICAL, MAX_RADIAL, MAX_BASIS_EMB = 8, 16, 8


# ---- float64 table of the spherical basis: roots z_ln of j_l and normalisers (0.5 j_{l+1}(z_ln)^2)^(-1/2) ----------------------------------------------------
def _sph_jn(l, x):
    """j_l(x), float64, upward recurrence (used at and between the roots only, where x > l)."""
    x = np.asarray(x, dtype=np.float64)
    jm = np.sin(x) / x
    if l == 0:
        return jm
    j = (np.sin(x) / x - np.cos(x)) / x
    for n in range(1, l):
        jm, j = j, (2 * n + 1) / x * j - jm
    return j


def bessel_table(num_spherical, num_radial):
    """(roots [S, R], norms [S, R]) float64.  The roots of j_l interlace those of j_{l-1}; each bracket is bisected down to neighbouring floats."""
    S, R = num_spherical, num_radial
    points = np.arange(1, R + S, dtype=np.float64) * np.pi
    roots = np.zeros((S, R))
    roots[0] = points[:R]
    for l in range(1, S):
        new = np.zeros(len(points) - 1)
        for q in range(len(points) - 1):
            a, b = points[q], points[q + 1]
            fa = _sph_jn(l, a)
            for _ in range(200):
                m = 0.5 * (a + b)
                if m == a or m == b:
                    break
                fm = _sph_jn(l, m)
                if (fm > 0) == (fa > 0):
                    a, fa = m, fm
                else:
                    b = m
            new[q] = 0.5 * (a + b)
        points = new
        roots[l] = points[:R]
    norms = np.stack([1.0 / np.sqrt(0.5 * _sph_jn(l + 1, roots[l]) ** 2) for l in range(S)])
    return roots, norms


# ---- the graph of a batch -----------------------------------------------------------------------------------------------------------------------------------
def build_plan(data, cutoff, max_num_neighbors):
    """radius_graph(pos, r=cutoff, batch, max_num_neighbors) as CSR by target (nq_es_graph_*), the edges sorted by source, d / u of every edge."""
    lib = _lib.load()
    pos = data.pos
    if not pos.is_cuda:
        raise RuntimeError("nabladft_amd.DimeNetPlusPlusPotential runs on MI355X only: tensors must be on a cuda (HIP) device")
    dev = pos.device
    pos = pos.detach().to(torch.float32).contiguous()
    N = int(pos.shape[0])
    z = data.z.to(dev).long()
    batch = data.batch.to(dev).long()
    lo, hi, B = (int(v) for v in torch.stack([z.min(), z.max(), batch[-1] + 1]).tolist())
    if lo < 0 or hi >= NUM_ELEMENTS:
        raise ValueError(f"DimeNet++ takes atomic numbers 0..{NUM_ELEMENTS - 1} (got {lo}..{hi})")
    counts = torch.bincount(batch, minlength=B)
    mol_ptr64 = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    mol_ptr, atom_mol = mol_ptr64.to(torch.int32).contiguous(), batch.to(torch.int32).contiguous()
    i32 = dict(device=dev, dtype=torch.int32)
    deg, row_ptr = torch.empty(N, **i32), torch.empty(N + 1, **i32)
    e_host = C.c_int32(0)
    _lib.check(lib.nq_es_graph_count(_lib.ptr(pos), _lib.ptr(mol_ptr), _lib.ptr(atom_mol), N, float(cutoff), int(max_num_neighbors), _lib.ptr(deg),
                                     _lib.ptr(row_ptr), C.byref(e_host), _st()))
    E = int(e_host.value)
    src, dst = torch.empty(E, **i32), torch.empty(E, **i32)
    geom = torch.empty(E, 4, device=dev, dtype=torch.float32)
    d, u = torch.empty(E, device=dev, dtype=torch.float32), torch.empty(E, 3, device=dev, dtype=torch.float32)
    if E:
        _lib.check(lib.nq_es_graph_fill(_lib.ptr(pos), _lib.ptr(mol_ptr), _lib.ptr(atom_mol), N, float(cutoff), int(max_num_neighbors), _lib.ptr(row_ptr),
                                        _lib.ptr(src), _lib.ptr(dst), _lib.ptr(geom), _st()))
        _lib.check(lib.nq_dn_geom_forward(_lib.ptr(geom), E, _lib.ptr(d), _lib.ptr(u), _st()))
    src_order, src_ptr = _inverse_lists(src, N)
    z32 = z.to(torch.int32).contiguous()
    z_order, z_ptr = _inverse_lists(z32, NUM_ELEMENTS)
    plan = SimpleNamespace(N=N, B=B, E=E, pos=pos, z=z32, z_levels=[(z_order, z_ptr, NUM_ELEMENTS)], mol_ptr=mol_ptr, atom_mol=atom_mol, row_ptr=row_ptr,
                           src=src, dst=dst, d=d, u=u, src_order=src_order.contiguous(), src_ptr=src_ptr.contiguous())
    plan.geometry_key = _lib.geometry_key(data)
    return plan


def _colsum(rows_t):
    """Column sums of [rows, C] in a fixed order."""
    lib = _lib.load()
    rows, Cc = rows_t.shape
    out = _new(Cc, like=rows_t)
    if rows == 0:
        return out.zero_()
    scr = _new(int(lib.nq_column_sum_scratch_floats(rows, Cc)) + 64, like=rows_t)
    _lib.check(lib.nq_column_sum(_lib.ptr(rows_t), rows, Cc, Cc, _lib.ptr(out), _lib.ptr(scr), _st()))
    return out


# ---- autograd wrappers ----------------------------------------------------------------------------------------------------------------------------------------
# Every ``backward`` below is itself a Function (``_*Bwd``) with the launches the first-order path always had, so it can be differentiated once more: a loss on the
# forces needs d/d parameters <v, dE/dpos>, v = d loss / d forces.  The adjoint that reaches a ``_*Bwd`` node is the tangent of the kernel along the position
# displacement; its ``backward`` returns that tangent pushed through the kernel (the adjoint of ``g``) and the reverse of the tangent with respect to the
# parameter-dependent inputs.  d, u and the positions get None there: the position gradient of a force loss is not provided.  Under ``create_graph=False`` the
# ``_*Bwd.apply`` calls run without recording anything: the same launches and the same bits as before.  The Linear layers are
# ``dense.Linear2``, built the same way; ``dense._FORCE_PASS`` is set around the force call of DimeNetPlusPlusPotential.forward: that pass asks for the position
# gradient only, so the backward functions skip the parameter gradients (weight-gradient products, W_sbf2 partials, column sums) it would compute and drop.


class _GeomFn(torch.autograd.Function):
    """pos -> (d [E], u [E, 3]) of the plan's graph (the values were written when the graph was built from the same positions)."""

    @staticmethod
    def forward(ctx, pos, plan):
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        return plan.d.clone(), plan.u.clone()

    @staticmethod
    def backward(ctx, gd, gu):
        plan = ctx.plan
        if gd is None and gu is None:
            return _new(plan.N, 3, like=plan.pos).zero_(), None
        return _GeomBwd.apply(gd, gu, plan), None


class _GeomBwd(torch.autograd.Function):
    """(gd, gu) -> gpos.  Second sweep: the adjoint of gpos is a displacement of the atoms; (a_gd, a_gu) = the tangent (td, tu) of (d, u) along it."""

    @staticmethod
    def forward(ctx, gd, gu, plan):
        gd = None if gd is None else _f32(gd)
        gu = None if gu is None else _f32(gu)
        gpos, gvec = _new(plan.N, 3, like=plan.pos), _new(plan.E, 3, like=plan.pos)
        _lib.check(_lib.load().nq_dn_geom_backward(_lib.ptr(plan.d), _lib.ptr(plan.u), _lib.ptr(gd), _lib.ptr(gu), _lib.ptr(plan.row_ptr), _lib.ptr(plan.src_order),
                                                   _lib.ptr(plan.src_ptr), plan.N, plan.E, _lib.ptr(gvec), _lib.ptr(gpos), _st()))
        ctx.plan, ctx.has = plan, (gd is not None, gu is not None)
        ctx.set_materialize_grads(False)
        return gpos

    @staticmethod
    def backward(ctx, a_gpos):
        if a_gpos is None:
            return None, None, None
        plan = ctx.plan
        a_gpos = _f32(a_gpos)
        td, tu = _new(plan.E, like=plan.pos), _new(plan.E, 3, like=plan.pos)
        _lib.check(_lib.load().nq_dnt_geom(_lib.ptr(plan.d), _lib.ptr(plan.u), _lib.ptr(a_gpos), _lib.ptr(plan.src), _lib.ptr(plan.dst), plan.E, _lib.ptr(td),
                                           _lib.ptr(tu), _st()))
        return (td if ctx.has[0] else None), (tu if ctx.has[1] else None), None


class _BasisFn(torch.autograd.Function):
    """(d [E], freq [R]) -> (rbf [E, R], rad [E, S * R]), float64 inside the kernel."""

    @staticmethod
    def forward(ctx, d, freq, roots, norms, S, R, cutoff, p):
        d, freq = _f32(d), _f32(freq)
        E = d.shape[0]
        rbf, rad = _new(E, R, like=d), _new(E, S * R, like=d)
        _lib.check(_lib.load().nq_dn_basis_forward(_lib.ptr(d), _lib.ptr(freq), _lib.ptr(roots), _lib.ptr(norms), E, S, R, float(cutoff), p, _lib.ptr(rbf),
                                                   _lib.ptr(rad), _st()))
        ctx.save_for_backward(d, freq)
        ctx.meta = (roots, norms, S, R, cutoff, p)
        ctx.set_materialize_grads(False)
        return rbf, rad

    @staticmethod
    def backward(ctx, g_rbf, g_rad):
        d, freq = ctx.saved_tensors
        return (*_BasisBwd.apply(g_rbf, g_rad, d, freq, ctx.meta, ctx.needs_input_grad[1] and not dense._FORCE_PASS[0]), None, None, None, None, None, None)


class _BasisBwd(torch.autograd.Function):
    """(g_rbf, g_rad) -> (gd, gfreq).  Second sweep, t = the adjoint of gd: a_g_rbf = t drbf/dd, a_g_rad = t dRad/dd, a_freq[n] = sum_e t g_rbf d2rbf/(dd dfreq_n)."""

    @staticmethod
    def forward(ctx, g_rbf, g_rad, d, freq, meta, need_freq):
        roots, norms, S, R, cutoff, p = meta
        E = d.shape[0]
        g_rbf = None if g_rbf is None else _f32(g_rbf)
        g_rad = None if g_rad is None else _f32(g_rad)
        gd, rows = _new(E, like=d), _new(E, R, like=d)
        _lib.check(_lib.load().nq_dn_basis_backward(_lib.ptr(d), _lib.ptr(freq), _lib.ptr(roots), _lib.ptr(norms), E, S, R, float(cutoff), p, _lib.ptr(g_rbf),
                                                    _lib.ptr(g_rad), _lib.ptr(gd), _lib.ptr(rows), _st()))
        gfreq = _colsum(rows) if need_freq else None
        ctx.save_for_backward(d, freq, g_rbf if g_rbf is not None else d.new_zeros(0))
        ctx.meta, ctx.has = meta, (g_rbf is not None, g_rad is not None)
        ctx.set_materialize_grads(False)
        return gd, gfreq

    @staticmethod
    def backward(ctx, t, a_gfreq):
        dense.only_tangents("the frequency gradient", a_gfreq)
        if t is None:
            return (None,) * 6
        d, freq, g_rbf = ctx.saved_tensors
        roots, norms, S, R, cutoff, p = ctx.meta
        E = d.shape[0]
        t = _f32(t)
        rbf_t, rad_t, rows = _new(E, R, like=d), _new(E, S * R, like=d), _new(E, R, like=d)
        _lib.check(_lib.load().nq_dnt_basis(_lib.ptr(d), _lib.ptr(freq), _lib.ptr(roots), _lib.ptr(norms), E, S, R, float(cutoff), p, _lib.ptr(t),
                                            _lib.ptr(g_rbf) if ctx.has[0] else None, _lib.ptr(rbf_t), _lib.ptr(rad_t), _lib.ptr(rows), _st()))
        a_freq = _colsum(rows) if ctx.needs_input_grad[3] and ctx.has[0] else None
        return (rbf_t if ctx.has[0] else None), (rad_t if ctx.has[1] else None), None, a_freq, None, None


class _TripletFn(torch.autograd.Function):
    """m[(j->i)] = sum_{(k->j), k != i} x_kj[(k->j)] * (W_sbf2 (sum_l Y_l(u_ji . u_kj) Q[(k->j)][l]))."""

    @staticmethod
    def forward(ctx, x, Q, u, W2, plan, S):
        x, Q, u, W2 = _f32(x), _f32(Q), _f32(u), _f32(W2)
        I, Bs = W2.shape
        m = _new(plan.E, I, like=x)
        _lib.check(_lib.load().nq_dn_triplet_forward(_lib.ptr(x), _lib.ptr(Q), _lib.ptr(u), _lib.ptr(W2), _lib.ptr(plan.row_ptr), _lib.ptr(plan.src),
                                                     _lib.ptr(plan.dst), plan.E, I, S, Bs, _lib.ptr(m), _st()))
        ctx.save_for_backward(x, Q, u, W2)
        ctx.meta = (plan, S)
        return m

    @staticmethod
    def backward(ctx, g):
        x, Q, u, W2 = ctx.saved_tensors
        plan, S = ctx.meta
        return (*_TripletBwd.apply(g, x, Q, u, W2, plan, S, ctx.needs_input_grad[3] and not dense._FORCE_PASS[0]), None, None)


class _TripletBwd(torch.autograd.Function):
    """g -> (gx, gQ, gu, gW2).  Second sweep: (a_gx, a_gQ, a_gu) are the tangents (tx, tQ, tu) of (x, Q, u); a_g = the tangent of m along them
    (nq_dnt_triplet_forward) and (a_x, a_Q, a_W2) = the reverse of <g, that tangent> (nq_dnt_triplet_backward).  u gets None."""

    @staticmethod
    def forward(ctx, g, x, Q, u, W2, plan, S, need_W2):
        lib = _lib.load()
        I, Bs = W2.shape
        g = _f32(g)
        gx, gQ, gu = torch.empty_like(x), torch.empty_like(Q), torch.empty_like(u)
        gW2 = scr = None
        if need_W2:
            gW2 = torch.empty_like(W2)
            scr = _new(int(lib.nq_dn_triplet_scratch_floats(plan.E, I, Bs)) + 64, like=x)
        _lib.check(lib.nq_dn_triplet_backward(_lib.ptr(x), _lib.ptr(Q), _lib.ptr(u), _lib.ptr(W2), _lib.ptr(plan.row_ptr), _lib.ptr(plan.src), _lib.ptr(plan.dst),
                                              _lib.ptr(plan.src_order), _lib.ptr(plan.src_ptr), plan.E, I, S, Bs, _lib.ptr(g), _lib.ptr(gx), _lib.ptr(gQ),
                                              _lib.ptr(gu), _lib.ptr(gW2), _lib.ptr(scr), _st()))
        ctx.save_for_backward(g, x, Q, u, W2)
        ctx.meta = (plan, S)
        ctx.set_materialize_grads(False)
        return gx, gQ, gu, gW2

    @staticmethod
    def backward(ctx, tx, tQ, tu, a_gW2):
        dense.only_tangents("the W_sbf2 gradient", a_gW2)
        out = [None] * 8
        if tx is None and tQ is None and tu is None:
            return tuple(out)
        lib = _lib.load()
        g, x, Q, u, W2 = ctx.saved_tensors
        plan, S = ctx.meta
        I, Bs = W2.shape
        tx, tQ, tu = (None if t is None else _f32(t) for t in (tx, tQ, tu))
        if ctx.needs_input_grad[0]:
            mt = _new(plan.E, I, like=x)
            _lib.check(lib.nq_dnt_triplet_forward(_lib.ptr(x), _lib.ptr(Q), _lib.ptr(u), _lib.ptr(W2), _lib.ptr(tx), _lib.ptr(tQ), _lib.ptr(tu), _lib.ptr(plan.row_ptr),
                                                  _lib.ptr(plan.src), _lib.ptr(plan.dst), plan.E, I, S, Bs, _lib.ptr(mt), _st()))
            out[0] = mt
        if any(ctx.needs_input_grad[k] for k in (1, 2, 4)):
            a_x, a_Q = torch.empty_like(x), torch.empty_like(Q)
            a_W2 = scr = None
            if ctx.needs_input_grad[4]:
                a_W2 = torch.empty_like(W2)
                scr = _new(int(lib.nq_dn_triplet_scratch_floats(plan.E, I, Bs)) + 64, like=x)
            _lib.check(lib.nq_dnt_triplet_backward(_lib.ptr(x), _lib.ptr(Q), _lib.ptr(u), _lib.ptr(W2), _lib.ptr(tx), _lib.ptr(tQ), _lib.ptr(tu), _lib.ptr(plan.row_ptr),
                                                   _lib.ptr(plan.src), _lib.ptr(plan.dst), _lib.ptr(plan.src_order), _lib.ptr(plan.src_ptr), plan.E, I, S, Bs,
                                                   _lib.ptr(g), _lib.ptr(a_x), _lib.ptr(a_Q), _lib.ptr(a_W2), _lib.ptr(scr), _st()))
            out[1], out[2], out[4] = a_x, a_Q, a_W2
        return tuple(out)


class _GateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gate):
        x, gate = _f32(x), _f32(gate)
        y = torch.empty_like(x)
        _lib.check(_lib.load().nq_dn_gate_forward(_lib.ptr(x), _lib.ptr(gate), x.numel(), _lib.ptr(y), _st()))
        ctx.save_for_backward(x, gate)
        return y

    @staticmethod
    def backward(ctx, g):
        return _GateBwd.apply(g, *ctx.saved_tensors)


class _GateBwd(torch.autograd.Function):
    """g -> (gx, gg) = (g gate, g x).  Second sweep (one small kernel, nq_dnt_gate): a_g = a_gx gate + a_gg x, a_x = a_gg g, a_gate = a_gx g."""

    @staticmethod
    def forward(ctx, g, x, gate):
        g = _f32(g)
        gx, gg = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().nq_dn_gate_backward(_lib.ptr(x), _lib.ptr(gate), _lib.ptr(g), x.numel(), _lib.ptr(gx), _lib.ptr(gg), _st()))
        ctx.save_for_backward(g, x, gate)
        ctx.set_materialize_grads(False)
        return gx, gg

    @staticmethod
    def backward(ctx, a_gx, a_gg):
        if a_gx is None and a_gg is None:
            return None, None, None
        g, x, gate = ctx.saved_tensors
        a_gx, a_gg = (None if t is None else _f32(t) for t in (a_gx, a_gg))
        a_g, a_x, a_gate = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().nq_dnt_gate(_lib.ptr(x), _lib.ptr(gate), _lib.ptr(g), _lib.ptr(a_gx), _lib.ptr(a_gg), x.numel(), _lib.ptr(a_g), _lib.ptr(a_x),
                                           _lib.ptr(a_gate), _st()))
        return a_g, a_x, a_gate


class _GateSumFn(torch.autograd.Function):
    """out[i] = sum over the in-edges e of atom i of x[e] * gate[e]."""

    @staticmethod
    def forward(ctx, x, gate, plan):
        x, gate = _f32(x), _f32(gate)
        H = x.shape[1]
        out = _new(plan.N, H, like=x)
        _lib.check(_lib.load().nq_dn_gatesum_forward(_lib.ptr(x), _lib.ptr(gate), _lib.ptr(plan.row_ptr), plan.N, H, _lib.ptr(out), _st()))
        ctx.save_for_backward(x, gate)
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, g):
        x, gate = ctx.saved_tensors
        return (*_GateSumBwd.apply(g, x, gate, ctx.plan), None)


class _GateSumBwd(torch.autograd.Function):
    """g [N, H] -> (gx, gg) = (g[dst] gate, g[dst] x).  Second sweep, composed from the existing calls (the [N, H] results are small): a_g = gatesum(a_gx, gate) +
    gatesum(a_gg, x); (a_x, a_gate) = nq_dn_gatesum_backward with (a_gx, a_gg) in the places of (x, gate)."""

    @staticmethod
    def forward(ctx, g, x, gate, plan):
        g = _f32(g)
        gx, gg = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().nq_dn_gatesum_backward(_lib.ptr(x), _lib.ptr(gate), _lib.ptr(g), _lib.ptr(plan.dst), plan.E, x.shape[1], _lib.ptr(gx), _lib.ptr(gg),
                                                      _st()))
        ctx.save_for_backward(g, x, gate)
        ctx.plan = plan
        return gx, gg

    @staticmethod
    def backward(ctx, a_gx, a_gg):
        lib = _lib.load()
        g, x, gate = ctx.saved_tensors
        plan = ctx.plan
        H = x.shape[1]
        a_gx, a_gg = _f32(a_gx), _f32(a_gg)
        p, q = _new(plan.N, H, like=x), _new(plan.N, H, like=x)
        _lib.check(lib.nq_dn_gatesum_forward(_lib.ptr(a_gx), _lib.ptr(gate), _lib.ptr(plan.row_ptr), plan.N, H, _lib.ptr(p), _st()))
        _lib.check(lib.nq_dn_gatesum_forward(_lib.ptr(a_gg), _lib.ptr(x), _lib.ptr(plan.row_ptr), plan.N, H, _lib.ptr(q), _st()))
        a_x, a_gate = torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.nq_dn_gatesum_backward(_lib.ptr(a_gx), _lib.ptr(a_gg), _lib.ptr(g), _lib.ptr(plan.dst), plan.E, H, _lib.ptr(a_x), _lib.ptr(a_gate), _st()))
        return p + q, a_x, a_gate, None


class _EmbedFn(torch.autograd.Function):
    """silu(AB[dst][:H] + AB[src][H:] + Cr + bias): the embedding block's Linear(3H, H) after its products over N and E rows.  -> (y, pre), ``pre`` as in ``dense.Linear2``."""

    @staticmethod
    def forward(ctx, AB, Cr, bias, plan):
        AB, Cr, bias = _f32(AB), _f32(Cr), _f32(bias)
        H = Cr.shape[1]
        pre, y = torch.empty_like(Cr), torch.empty_like(Cr)
        _lib.check(_lib.load().nq_dn_embed_forward(_lib.ptr(AB), _lib.ptr(Cr), _lib.ptr(bias), _lib.ptr(plan.src), _lib.ptr(plan.dst), plan.E, H, _lib.ptr(pre),
                                                   _lib.ptr(y), _st()))
        ctx.save_for_backward(pre)
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        return y, pre

    @staticmethod
    def backward(ctx, g, g_pre):
        if g is None and g_pre is None:
            return None, None, None, None
        (pre,) = ctx.saved_tensors
        return (*_EmbedBwd.apply(g, g_pre, pre, ctx.plan, ctx.needs_input_grad[2] and not dense._FORCE_PASS[0]), None)


class _EmbedBwd(torch.autograd.Function):
    """(g, g_pre) -> (gAB, gpre, gbias), gpre = g silu'(pre) + g_pre.  Second sweep: a = the adjoint of gpre (the one output the positions reach, through Cr):
    a_g = a silu'(pre), a_pre = a g silu''(pre)."""

    @staticmethod
    def forward(ctx, g, g_pre, pre, plan, need_bias):
        lib = _lib.load()
        H = pre.shape[1]
        g = None if g is None else _f32(g)
        gAB = _new(plan.N, 2 * H, like=pre)
        if g_pre is None:
            gpre = torch.empty_like(pre)
            _lib.check(lib.nq_dn_embed_backward(_lib.ptr(pre), _lib.ptr(g), _lib.ptr(plan.row_ptr), _lib.ptr(plan.src_order), _lib.ptr(plan.src_ptr), plan.N, plan.E,
                                                H, _lib.ptr(gpre), _lib.ptr(gAB), _st()))
        else:
            gpre = _f32(g_pre)
            if g is not None and plan.E:
                gpre = dense.silu_grad(pre, g) + gpre
            _lib.check(lib.nq_dnt_embed_scatter(_lib.ptr(gpre), _lib.ptr(plan.row_ptr), _lib.ptr(plan.src_order), _lib.ptr(plan.src_ptr), plan.N, plan.E, H,
                                                _lib.ptr(gAB), _st()))
        ctx.save_for_backward(pre, g if g is not None else pre.new_zeros(0))
        ctx.has = (g is not None, g_pre is not None)
        ctx.set_materialize_grads(False)
        return gAB, gpre, (_colsum(gpre) if need_bias else None)

    @staticmethod
    def backward(ctx, a_gAB, a, a_gbias):
        dense.only_tangents("the embedding's atom-side gradients", a_gAB, a_gbias)
        if a is None:
            return (None,) * 5
        pre, g = ctx.saved_tensors
        a = _f32(a)
        a_g = a_pre = None
        if ctx.has[0]:
            a_g, a_pre = dense.silu_grad2(pre, g, a)
        return a_g, (a if ctx.has[1] else None), a_pre, None, None


# ---- the core's module tree (parameter holders with torch-geometric's initialisation; the arithmetic is in DimeNetPlusPlus.forward) ---------------------------
def glorot_orthogonal(tensor, scale):
    nn.init.orthogonal_(tensor.data)
    tensor.data *= (scale / ((tensor.size(-2) + tensor.size(-1)) * tensor.var())).sqrt()


def _lin(n_in, n_out, bias=True):
    lin = nn.Linear(n_in, n_out, bias=bias)
    glorot_orthogonal(lin.weight, 2.0)
    if bias:
        lin.bias.data.fill_(0)
    return lin


class BesselBasisLayer(nn.Module):
    def __init__(self, num_radial, cutoff, envelope_exponent):
        super().__init__()
        self.cutoff, self.p = cutoff, envelope_exponent + 1
        self.freq = nn.Parameter(torch.arange(1, num_radial + 1, dtype=torch.float32) * math.pi)


class EmbeddingBlock(nn.Module):
    def __init__(self, num_radial, hidden_channels):
        super().__init__()
        self.emb = nn.Embedding(NUM_ELEMENTS, hidden_channels)
        self.emb.weight.data.uniform_(-math.sqrt(3), math.sqrt(3))
        self.lin_rbf = nn.Linear(num_radial, hidden_channels)
        self.lin = nn.Linear(3 * hidden_channels, hidden_channels)


class ResidualLayer(nn.Module):
    def __init__(self, hidden_channels):
        super().__init__()
        self.lin1, self.lin2 = _lin(hidden_channels, hidden_channels), _lin(hidden_channels, hidden_channels)


class InteractionPPBlock(nn.Module):
    def __init__(self, hidden_channels, int_emb_size, basis_emb_size, num_spherical, num_radial, num_before_skip, num_after_skip):
        super().__init__()
        self.lin_rbf1 = _lin(num_radial, basis_emb_size, bias=False)
        self.lin_rbf2 = _lin(basis_emb_size, hidden_channels, bias=False)
        self.lin_sbf1 = _lin(num_spherical * num_radial, basis_emb_size, bias=False)
        self.lin_sbf2 = _lin(basis_emb_size, int_emb_size, bias=False)
        self.lin_kj, self.lin_ji = _lin(hidden_channels, hidden_channels), _lin(hidden_channels, hidden_channels)
        self.lin_down = _lin(hidden_channels, int_emb_size, bias=False)
        self.lin_up = _lin(int_emb_size, hidden_channels, bias=False)
        self.layers_before_skip = nn.ModuleList([ResidualLayer(hidden_channels) for _ in range(num_before_skip)])
        self.lin = _lin(hidden_channels, hidden_channels)
        self.layers_after_skip = nn.ModuleList([ResidualLayer(hidden_channels) for _ in range(num_after_skip)])


class OutputPPBlock(nn.Module):
    def __init__(self, num_radial, hidden_channels, out_emb_channels, out_channels, num_layers):
        super().__init__()
        self.lin_rbf = _lin(num_radial, hidden_channels, bias=False)
        self.lin_up = _lin(hidden_channels, out_emb_channels, bias=False)
        self.lins = nn.ModuleList([_lin(out_emb_channels, out_emb_channels) for _ in range(num_layers)])
        self.lin = nn.Linear(out_emb_channels, out_channels, bias=False)
        self.lin.weight.data.fill_(0)


class DimeNetPlusPlus(nn.Module):
    """torch_geometric.nn.models.DimeNetPlusPlus (2.4.0) restated: (pos, z, batch) -> [B, out_channels]."""

    def __init__(self, hidden_channels, out_channels, num_blocks, int_emb_size, basis_emb_size, out_emb_channels, num_spherical, num_radial, cutoff=5.0,
                 max_num_neighbors=32, envelope_exponent=5, num_before_skip=1, num_after_skip=2, num_output_layers=3):
        super().__init__()
        problems = []
        if int_emb_size not in INT_EMB_SIZES:
            problems.append(f"int_emb_size {int_emb_size} (built: {INT_EMB_SIZES})")
        if not 1 <= basis_emb_size <= MAX_BASIS_EMB:
            problems.append(f"basis_emb_size {basis_emb_size} (1..{MAX_BASIS_EMB})")
        if not 2 <= num_spherical <= MAX_SPHERICAL:
            problems.append(f"num_spherical {num_spherical} (2..{MAX_SPHERICAL})")
        if not 1 <= num_radial <= MAX_RADIAL:
            problems.append(f"num_radial {num_radial} (1..{MAX_RADIAL})")
        if hidden_channels < 32 or hidden_channels % 32 or out_emb_channels < 32 or out_emb_channels % 32:
            problems.append(f"hidden_channels {hidden_channels} / out_emb_channels {out_emb_channels} (multiples of 32)")
        if not 1 <= envelope_exponent <= 15:
            problems.append(f"envelope_exponent {envelope_exponent} (1..15)")
        if num_blocks < 1 or out_channels < 1 or max_num_neighbors < 1 or not cutoff > 0 or min(num_before_skip, num_after_skip, num_output_layers) < 0:
            problems.append("num_blocks / out_channels / max_num_neighbors / cutoff must be positive")
        if problems:
            raise NotImplementedError("DimeNet++ kernels are not built for " + "; ".join(problems))
        self.cutoff, self.max_num_neighbors, self.num_blocks = cutoff, max_num_neighbors, num_blocks
        self.num_spherical, self.num_radial, self.out_channels = num_spherical, num_radial, out_channels
        self.rbf = BesselBasisLayer(num_radial, cutoff, envelope_exponent)
        self.emb = EmbeddingBlock(num_radial, hidden_channels)
        self.output_blocks = nn.ModuleList([OutputPPBlock(num_radial, hidden_channels, out_emb_channels, out_channels, num_output_layers)
                                            for _ in range(num_blocks + 1)])
        self.interaction_blocks = nn.ModuleList([InteractionPPBlock(hidden_channels, int_emb_size, basis_emb_size, num_spherical, num_radial, num_before_skip,
                                                                    num_after_skip) for _ in range(num_blocks)])
        self.bessel_roots, self.bessel_norms = bessel_table(num_spherical, num_radial)        # float64 numpy; not part of the state_dict
        self._table = {}
        self._frozen = False

    def _tables(self, dev):
        if dev not in self._table:
            self._table[dev] = (torch.from_numpy(self.bessel_roots).to(dev).contiguous(), torch.from_numpy(self.bessel_norms).to(dev).contiguous())
        return self._table[dev]

    def prepare(self, data):
        return build_plan(data, self.cutoff, self.max_num_neighbors)

    def _w(self, p):
        return p.detach() if self._frozen else p

    def _dense(self, lin, x, silu=False):
        return dense.linear2(x, self._w(lin.weight), None if lin.bias is None else self._w(lin.bias), silu)

    def _residual(self, layer, h):
        return h + self._dense(layer.lin2, self._dense(layer.lin1, h, True), True)

    def _output(self, blk, x, rbf, plan):
        h = _GateSumFn.apply(x, self._dense(blk.lin_rbf, rbf), plan)
        h = self._dense(blk.lin_up, h)
        for lin in blk.lins:
            h = self._dense(lin, h, True)
        return self._dense(blk.lin, h)

    def _interaction(self, blk, x, rbf, rad, u, plan):
        S, R = self.num_spherical, self.num_radial
        x_ji, x_kj = self._dense(blk.lin_ji, x, True), self._dense(blk.lin_kj, x, True)
        x_kj = _GateFn.apply(x_kj, self._dense(blk.lin_rbf2, self._dense(blk.lin_rbf1, rbf)))
        x_kj = self._dense(blk.lin_down, x_kj, True)
        W1 = self._w(blk.lin_sbf1.weight)
        Bs = W1.shape[0]
        W1v = W1.view(Bs, S, R)
        Q = dense.linear2(rad, torch.block_diag(*[W1v[:, l, :] for l in range(S)]), None)         # Q[e][l][b] = sum_n rad[e][l][n] W1[b][l R + n]
        m = _TripletFn.apply(x_kj, Q, u, self._w(blk.lin_sbf2.weight), plan, S)
        h = x_ji + self._dense(blk.lin_up, m, True)
        for layer in blk.layers_before_skip:
            h = self._residual(layer, h)
        h = self._dense(blk.lin, h, True) + x
        for layer in blk.layers_after_skip:
            h = self._residual(layer, h)
        return h

    def forward_plan(self, pos, plan, record=None):
        """pos: the float32 leaf the plan was built from.  -> [B, out_channels]."""
        H = self.emb.emb.weight.shape[1]
        d, u = _GeomFn.apply(pos, plan)
        roots, norms = self._tables(pos.device)
        rbf, rad = _BasisFn.apply(d, self._w(self.rbf.freq), roots, norms, self.num_spherical, self.num_radial, self.cutoff, self.rbf.p)
        W = self._w(self.emb.lin.weight)
        hz = _EmbeddingFn.apply(self._w(self.emb.emb.weight), plan.z, plan.z_levels)
        AB = dense.linear2(hz, torch.cat([W[:, :H], W[:, H:2 * H]], 0), None)
        Cr = dense.linear2(self._dense(self.emb.lin_rbf, rbf, True), W[:, 2 * H:].contiguous(), None)
        x = _EmbedFn.apply(AB, Cr, self._w(self.emb.lin.bias), plan)[0]
        P = self._output(self.output_blocks[0], x, rbf, plan)
        if record is not None:
            record.update(rbf=rbf, rad=rad, block_out=[x])
        for blk, out in zip(self.interaction_blocks, self.output_blocks[1:]):
            x = self._interaction(blk, x, rbf, rad, u, plan)
            P = P + self._output(out, x, rbf, plan)
            if record is not None:
                record["block_out"].append(x)
        return _SegSumFn.apply(P, plan.mol_ptr, plan.atom_mol, plan.B)


class Swish(nn.Module):
    def forward(self, x):
        return x * x.sigmoid()


class DimeNetPlusPlusPotential(nn.Module):
    def __init__(self, node_latent_dim: int, scaler=None, dimenet_hidden_channels=128, dimenet_num_blocks=4, dimenet_int_emb_size=64, dimenet_basis_emb_size=8,
                 dimenet_out_emb_channels=256, dimenet_num_spherical=7, dimenet_num_radial=6, dimenet_max_num_neighbors=32, dimenet_envelope_exponent=5,
                 dimenet_num_before_skip=1, dimenet_num_after_skip=2, dimenet_num_output_layers=3, cutoff=5.0, do_postprocessing=False):
        super().__init__()
        if node_latent_dim < 2:
            raise NotImplementedError("node_latent_dim must be at least 2 (the head halves it)")
        self.node_latent_dim = node_latent_dim
        self.dimenet_hidden_channels, self.dimenet_num_blocks, self.dimenet_int_emb_size = dimenet_hidden_channels, dimenet_num_blocks, dimenet_int_emb_size
        self.dimenet_basis_emb_size, self.dimenet_out_emb_channels = dimenet_basis_emb_size, dimenet_out_emb_channels
        self.dimenet_num_spherical, self.dimenet_num_radial, self.dimenet_max_num_neighbors = dimenet_num_spherical, dimenet_num_radial, dimenet_max_num_neighbors
        self.dimenet_envelope_exponent, self.dimenet_num_before_skip, self.dimenet_num_after_skip = dimenet_envelope_exponent, dimenet_num_before_skip, dimenet_num_after_skip
        self.dimenet_num_output_layers, self.cutoff = dimenet_num_output_layers, cutoff
        self.linear_output_size = 1
        self.scaler, self.do_postprocessing = scaler, do_postprocessing
        self.net = DimeNetPlusPlus(hidden_channels=dimenet_hidden_channels, out_channels=node_latent_dim, num_blocks=dimenet_num_blocks,
                                   int_emb_size=dimenet_int_emb_size, basis_emb_size=dimenet_basis_emb_size, out_emb_channels=dimenet_out_emb_channels,
                                   num_spherical=dimenet_num_spherical, num_radial=dimenet_num_radial, cutoff=cutoff, max_num_neighbors=dimenet_max_num_neighbors,
                                   envelope_exponent=dimenet_envelope_exponent, num_before_skip=dimenet_num_before_skip, num_after_skip=dimenet_num_after_skip,
                                   num_output_layers=dimenet_num_output_layers)
        n = node_latent_dim
        self.regr_or_cls_nn = nn.Sequential(nn.Linear(n, n), Swish(), nn.Linear(n, n // 2), Swish(), nn.Linear(n // 2, n // 2), Swish(),
                                            nn.Linear(n // 2, self.linear_output_size))

    def _plan(self, data):
        plan = getattr(data, "prepared", None)
        if plan is None:
            return self.net.prepare(data)
        if plan.N != int(data.pos.shape[0]):
            raise ValueError("data.prepared belongs to another batch")
        _lib.check_prepared(plan, data)
        return plan

    def forward(self, data, return_intermediates: bool = False, create_graph: bool = False):
        """-> (energies [B], forces [N, 3]); the energies carry the graph of the parameters when gradients are enabled.  The forces carry no autograd graph unless
        ``create_graph`` is set (and gradients are enabled): then the force call is ``torch.autograd.grad(..., create_graph=True)`` and the forces, bitwise those of
        the default path, carry the graph of the parameters (the second sweep of the wrappers above), so a loss on them trains.  That graph reaches the
        parameters only: the second sweep forms no adjoint of the distances, the directions or the positions, so the position gradient of a force loss is not
        provided (the internal position leaf is never handed out)."""
        plan = self._plan(data)
        with_graph = torch.is_grad_enabled()
        second = bool(create_graph) and with_graph
        net = self.net
        net._frozen = not with_graph
        rec = {} if return_intermediates else None
        try:
            with torch.enable_grad():
                pos = plan.pos.detach().requires_grad_(True)
                P = net.forward_plan(pos, plan, rec)
                h = P
                for k in (0, 2, 4):
                    h = net._dense(self.regr_or_cls_nn[k], h, True)
                pred = net._dense(self.regr_or_cls_nn[6], h).reshape(-1)
                if plan.E:
                    dense._FORCE_PASS[0] = True
                    (gpos,) = torch.autograd.grad(pred.sum(), pos, retain_graph=with_graph, create_graph=second)
                else:
                    gpos = torch.zeros_like(pos)
        finally:
            net._frozen = False
            dense._FORCE_PASS[0] = False
        forces = -gpos if second and gpos.requires_grad else -gpos.detach()
        if not with_graph:
            pred = pred.detach()
        if rec is not None:
            rec["P"], rec["unscaled"] = P.detach(), pred.detach()
        if self.scaler and self.do_postprocessing:
            pred = self.scaler["scale_"] * pred + self.scaler["mean_"]
        self.last_plan = plan
        return (pred, forces, rec) if return_intermediates else (pred, forces)


class DimeNetPlusPlusLightning(_Task):
    """dimenetplusplus.py:116-270.  ``step`` is the reference's; ``training_step`` refuses a force loss (the second-order sweep is ``DimeNetPlusPlusForceLightning``)."""

    def __init__(self, net: nn.Module, loss, metric, energy_loss_coef: float, forces_loss_coef: float, monitor_loss: str = "val/loss", model_name: str = None,
                 lr_scheduler=None, scheduler_args=None, optimizer=None):
        super().__init__()
        self.net, self.loss = net, loss
        self.scheduler_args, self.monitor_loss = scheduler_args, monitor_loss
        self.loss_energy_coef, self.loss_forces_coef = energy_loss_coef, forces_loss_coef
        self._store_hparams(["net", "loss"], metric=metric, energy_loss_coef=energy_loss_coef, forces_loss_coef=forces_loss_coef, monitor_loss=monitor_loss,
                            model_name=model_name, lr_scheduler=lr_scheduler, scheduler_args=scheduler_args, optimizer=optimizer)

    def forward(self, data):
        return self.net(data)

    def predict_step(self, batch, *args, **kwargs):
        return self(batch)

    def step(self, batch, calculate_metrics: bool = False):
        energy, forces = self.forward(batch)
        target_f = batch.forces.to(forces.dtype)
        loss = self.loss_forces_coef * self.loss(forces, target_f) + self.loss_energy_coef * self.loss(energy, batch.y)
        if calculate_metrics:
            return loss, self._calculate_metrics({"energy": energy, "forces": forces}, {"energy": batch.y, "forces": target_f})
        return loss

    def training_step(self, batch, batch_idx):
        if self.loss_forces_coef != 0:
            raise NotImplementedError("DimeNet++ training with forces_loss_coef != 0 differentiates the forces with respect to the parameters: the second-order "
                                      "sweep is not part of this class; use DimeNetPlusPlusForceLightning (same constructor, same state_dict) or train with "
                                      "forces_loss_coef = 0 (validation, test and predict work with any coefficient)")
        return super().training_step(batch, batch_idx)

    def configure_optimizers(self):
        opt = self.hparams.optimizer(self.parameters())
        scheduler = None
        if self.hparams.lr_scheduler is not None:
            scheduler = self.hparams.lr_scheduler(optimizer=opt, **(self.scheduler_args or {}))
        return {"optimizer": opt, "monitor": self.monitor_loss, "lr_scheduler": scheduler}


class DimeNetPlusPlusForceLightning(DimeNetPlusPlusLightning):
    """The same task with the reference's ``create_graph=self.training`` (dimenetplusplus.py:99-109): in training the forces carry the graph of the parameters, so
    ``training_step`` takes any ``forces_loss_coef`` (config/model/dimenetplusplus.yaml: 1 and 1).  Constructor, ``state_dict`` keys, validation, test and predict
    are the parent's.  The gradient of the force loss reaches the parameters, not the positions."""

    def forward(self, data):
        return self.net(data, create_graph=self.net.training)

    def training_step(self, batch, batch_idx):
        return _Task.training_step(self, batch, batch_idx)
