"""The force-loss training step of DimeNet++ on tests/dimenet_ref.py: the wrapper's arithmetic (dimenetplusplus.py:93-113 with ``create_graph=True``, :144-148)
around the restated core.  scripts/make_golden_dimenet_force.py asserts that it reproduces the real wrapper; the tests re-run it without the reference tree."""
import math
from collections import OrderedDict

import torch

from tests import dimenet_ref as D

PAIRS = ((1.0, 1.0), (0.0, 1.0))                # (energy_loss_coef, forces_loss_coef)


def tag(pair):
    return f"{pair[0]:g}_{pair[1]:g}"


def force_loss(cfg, params, b, pair, dtype=torch.float64, exact_basis=False):
    """-> (loss, {parameter name: gradient}, energies, forces) of loss = c_F L1(F, forces) + c_E L1(E, y), F = -dE/dpos with the graph of the parameters."""
    model = D.build(cfg, params, dtype, exact_basis)
    pos = b["pos"].to(dtype).clone().requires_grad_(True)
    pred = torch.flatten(model.regr_or_cls_nn(model.net(b["z"], pos, b["batch"])))
    forces = -torch.autograd.grad(pred, pos, grad_outputs=torch.ones_like(pred), create_graph=True)[0]
    l1 = torch.nn.L1Loss()
    loss = pair[1] * l1(forces, b["forces"].to(dtype)) + pair[0] * l1(pred, b["y"].to(dtype))
    gs = torch.autograd.grad(loss, list(model.parameters()), allow_unused=True)
    grads = OrderedDict((k, (torch.zeros_like(p) if g is None else g).detach()) for (k, p), g in zip(model.named_parameters(), gs))
    return loss.detach(), grads, pred.detach(), forces.detach()


# ---- the second sweep of one operation --------------------------------------------------------------------------------------------------------------------------
def second_sweep(fn, inputs, tangent_of, tangents, g, adjoint_of):
    """torch.autograd's own double backward of ``fn(*inputs) -> out`` (a tensor or a tuple): with first = d<g, out>/d inputs[tangent_of] kept in the graph and
    phi = <first, tangents>, returns d phi / d (g..., inputs[adjoint_of]...): the tangent of ``out`` along ``tangents`` followed by the adjoints of <g, that
    tangent> with respect to the chosen inputs.  float64 in, float64 out; ``g`` matches ``out``."""
    ins = [t.detach().double().clone().requires_grad_(True) for t in inputs]
    gs = [t.detach().double().clone().requires_grad_(True) for t in (g if isinstance(g, (tuple, list)) else (g,))]
    out = fn(*ins)
    outs = out if isinstance(out, (tuple, list)) else (out,)
    first = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, gs)), [ins[k] for k in tangent_of], create_graph=True)
    phi = sum((f * t.double()).sum() for f, t in zip(first, tangents))
    res = torch.autograd.grad(phi, gs + [ins[k] for k in adjoint_of], allow_unused=True)
    return [torch.zeros_like(w) if r is None else r for r, w in zip(res, gs + [ins[k] for k in adjoint_of])]


# ---- the formulas the kernels implement, stated in torch (any dtype) ---------------------------------------------------------------------------------------------
def legendre_dy(c, S):
    """dY_l0 / dc, l < S -> [..., S] (P'_{l+1} = ((2l + 1)(P_l + c P'_l) - l P'_{l-1}) / (l + 1))."""
    P, Q = [torch.ones_like(c), c], [torch.zeros_like(c), torch.ones_like(c)]
    for l in range(1, S - 1):
        P.append(((2 * l + 1) * c * P[l] - l * P[l - 1]) / (l + 1))
        Q.append(((2 * l + 1) * (P[l] + c * Q[l]) - l * Q[l - 1]) / (l + 1))
    return torch.stack([math.sqrt((2 * l + 1) / (4 * math.pi)) * Q[l] for l in range(S)], -1)


def triplet_tangent(kj, ji, E, x, Q, u, W2, tx, tQ, tu, g, S, Bs):
    """-> (mt, a_x, a_Q, a_W2): the tangent of the triplet product along (tx, tQ, tu) and the adjoints of <g, mt> with respect to x, Q and W2."""
    c = (u[ji] * u[kj]).sum(-1)
    cd = (tu[ji] * u[kj]).sum(-1) + (u[ji] * tu[kj]).sum(-1)
    Y, dYc = D.legendre_y(c, S), legendre_dy(c, S) * cd.unsqueeze(-1)
    Qk, tQk = Q[kj].view(-1, S, Bs), tQ[kj].view(-1, S, Bs)
    s = (Y.unsqueeze(-1) * Qk).sum(1)
    sd = (Y.unsqueeze(-1) * tQk + dYc.unsqueeze(-1) * Qk).sum(1)
    zero = lambda *shape: torch.zeros(*shape, dtype=x.dtype)                                            # noqa: E731
    mt = zero(E, W2.shape[0]).index_add_(0, ji, tx[kj] * (s @ W2.t()) + x[kj] * (sd @ W2.t()))
    a_x = zero(E, W2.shape[0]).index_add_(0, kj, g[ji] * (sd @ W2.t()))
    G1, G2 = (g[ji] * tx[kj]) @ W2, (g[ji] * x[kj]) @ W2
    a_Q = zero(E, S, Bs).index_add_(0, kj, Y.unsqueeze(-1) * G1.unsqueeze(1) + dYc.unsqueeze(-1) * G2.unsqueeze(1)).view(E, S * Bs)
    a_W2 = (g[ji] * tx[kj]).t() @ s + (g[ji] * x[kj]).t() @ sd
    return mt, a_x, a_Q, a_W2


def geometry(pos, src, dst):
    v = pos[dst] - pos[src]
    d = v.norm(dim=-1)
    return d, v / d[:, None]


def geometry_tangent(d, u, tpos, src, dst):
    w = tpos[dst] - tpos[src]
    td = (w * u).sum(-1)
    return td, (w - td[:, None] * u) / d[:, None]


def basis_tangent(d, freq, t, g_rbf, cutoff, exponent, S, R, table):
    """-> (rbf_t [E, R], rad_t [E, S R], a_freq [R]) with x = d / cutoff."""
    p = exponent + 1
    a, b, c = -(p + 1) * (p + 2) / 2, p * (p + 2), -p * (p + 1) / 2
    x = (d / cutoff).unsqueeze(-1)
    env = 1.0 / x + a * x.pow(p - 1) + b * x.pow(p) + c * x.pow(p + 1)
    denv = -1.0 / (x * x) + a * (p - 1) * x.pow(p - 2) + b * p * x.pow(p - 1) + c * (p + 1) * x.pow(p)
    te = (t / cutoff).unsqueeze(-1)
    sn, cs = torch.sin(freq * x), torch.cos(freq * x)
    rbf_t = te * (denv * sn + env * freq * cs)
    a_freq = (te * g_rbf * (denv * x * cs + env * cs - env * freq * x * sn)).sum(0)
    roots, norms = (torch.as_tensor(tb, dtype=d.dtype) for tb in table)
    cols = []
    for l in range(S):
        for n in range(R):
            z = roots[l, n] * x[:, 0]
            j = D._jl_stable(l, z)
            dj = -D._jl_stable(1, z) if l == 0 else D._jl_stable(l - 1, z) - (l + 1) / z * j
            cols.append(norms[l, n] * (denv[:, 0] * j + env[:, 0] * roots[l, n] * dj))
    return rbf_t, te * torch.stack(cols, 1), a_freq


def silu(x):
    return x * torch.sigmoid(x)


def silu_reverse2(pre, g, a):
    s = torch.sigmoid(pre)
    return a * s * (1 + pre * (1 - s)), a * g * s * (1 - s) * (2 + pre * (1 - 2 * s))
