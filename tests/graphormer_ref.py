"""Ragged restatement of Graphormer3D (reference nablaDFT/graphormer/graphormer_3d.py) in plain torch, written for float64: the operator references of
tests/test_graphormer_ops_gpu.py and the model reference that tests/test_graphormer_cpu.py pins to the real reference's recorded run
(tests/golden/graphormer_small*.npz, written by scripts/make_golden_graphormer.py).

Layout (the one of csrc/graphormer.hip): atoms [N] behind ptr [B + 1]; molecule b owns the n_b^2 ordered pairs (i, j), i = j included, row-major behind
pair_ptr [B + 1].  There are no padded rows and no -inf: a padded key of the reference carries a -inf bias, so real rows never read it, and padded query
rows are masked out of the energy, the forces and the loss -- the reference on real atoms IS this function (the generator asserts it to the last bit).
Per-pair tensors are pair-major here ([P, H] bias, [P, H] keep masks); ``to_heads`` / ``from_heads`` give the kernels' per-molecule [H][n][n] layout.

Every operator has its forward and an analytic backward (checked against float64 autograd of the forward in the CPU tests).  ``make_params`` is the
deterministic weight generator keyed by parameter name that the fixtures were made with, so no weights are stored.
"""
import math
import zlib
from collections import OrderedDict

import numpy as np
import torch

ATOM_TYPES = 64
EDGE_TYPES = 64 * 64
ELEMENTS = (1, 6, 7, 8, 9, 16, 17, 35)
SMALL = dict(blocks=2, layers=2, embed_dim=64, ffn_embed_dim=96, attention_heads=4, num_kernel=32)
SMALL_D32 = dict(blocks=2, layers=2, embed_dim=64, ffn_embed_dim=96, attention_heads=2, num_kernel=32)
YAML = dict(blocks=4, layers=6, embed_dim=512, ffn_embed_dim=512, attention_heads=32, num_kernel=128)
SMALL_SIZES = (1, 2, 17, 42, 63, 64, 65, 70)
YAML_SIZES = (29, 54)
DROPOUTS = dict(input_dropout=0.1, dropout=0.1, attention_dropout=0.0, activation_dropout=0.1)


# ---- batch structure and inputs ---------------------------------------------------------------------------------------------------------------------------
def structure(sizes):
    """ptr int64 [B + 1], pair_ptr int64 [B + 1], atom_mol int64 [N]."""
    sizes = np.asarray(sizes, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    pair_ptr = np.concatenate([[0], np.cumsum(sizes * sizes)])
    return torch.from_numpy(ptr), torch.from_numpy(pair_ptr), torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes))


def make_batch(sizes, seed):
    """Random compact conformers: z from ELEMENTS, positions in a box whose side grows with the cube root of the atom count (nearest distances ~1 A), and
    targets y [B], forces [N, 3].  float64."""
    rng = np.random.default_rng(seed)
    zs, ps = [], []
    for n in sizes:
        zs.append(rng.choice(ELEMENTS, size=n))
        side = 1.6 * max(n, 1) ** (1.0 / 3.0)
        ps.append(rng.uniform(0.0, side, size=(n, 3)) + rng.normal(size=3) * 3.0)
    N = int(sum(sizes))
    return dict(z=torch.from_numpy(np.concatenate(zs).astype(np.int64)), pos=torch.from_numpy(np.concatenate(ps)),
                y=torch.from_numpy(rng.normal(size=len(sizes))), forces=torch.from_numpy(rng.normal(size=(N, 3)) * 0.5), sizes=tuple(int(n) for n in sizes))


def to_heads(x_pm, sizes):
    """pair-major [P, H] -> the kernels' flat head-major buffer (per molecule [H][n][n])."""
    out, off = [], 0
    for n in sizes:
        out.append(x_pm[off:off + n * n].reshape(n, n, -1).permute(2, 0, 1).reshape(-1))
        off += n * n
    return torch.cat(out)


def from_heads(x_hm, sizes, H):
    out, off = [], 0
    for n in sizes:
        out.append(x_hm[off:off + H * n * n].reshape(H, n, n).permute(1, 2, 0).reshape(n * n, H))
        off += H * n * n
    return torch.cat(out)


# ---- parameters -------------------------------------------------------------------------------------------------------------------------------------------
def param_shapes(cfg):
    """[(name, shape)] in the reference's state_dict order."""
    E, Fd, H, K = cfg["embed_dim"], cfg["ffn_embed_dim"], cfg["attention_heads"], cfg["num_kernel"]
    out = [("atom_encoder.weight", (ATOM_TYPES, E)), ("tag_encoder.weight", (3, E))]
    for l in range(cfg["layers"]):
        p = f"layers.{l}."
        out += [(p + "self_attn.in_proj.weight", (3 * E, E)), (p + "self_attn.in_proj.bias", (3 * E,)), (p + "self_attn.out_proj.weight", (E, E)),
                (p + "self_attn.out_proj.bias", (E,)), (p + "self_attn_layer_norm.weight", (E,)), (p + "self_attn_layer_norm.bias", (E,)),
                (p + "fc1.weight", (Fd, E)), (p + "fc1.bias", (Fd,)), (p + "fc2.weight", (E, Fd)), (p + "fc2.bias", (E,)),
                (p + "final_layer_norm.weight", (E,)), (p + "final_layer_norm.bias", (E,))]
    out += [("final_ln.weight", (E,)), ("final_ln.bias", (E,)),
            ("energy_proj.layer1.weight", (E, E)), ("energy_proj.layer1.bias", (E,)), ("energy_proj.layer2.weight", (1, E)), ("energy_proj.layer2.bias", (1,)),
            ("energy_agg_factor.weight", (3, 1)),
            ("gbf.means.weight", (1, K)), ("gbf.stds.weight", (1, K)), ("gbf.mul.weight", (EDGE_TYPES, 1)), ("gbf.bias.weight", (EDGE_TYPES, 1)),
            ("bias_proj.layer1.weight", (K, K)), ("bias_proj.layer1.bias", (K,)), ("bias_proj.layer2.weight", (H, K)), ("bias_proj.layer2.bias", (H,)),
            ("edge_proj.weight", (E, K)), ("edge_proj.bias", (E,))]
    for n in ("q_proj", "k_proj", "v_proj"):
        out += [(f"node_proj.{n}.weight", (E, E)), (f"node_proj.{n}.bias", (E,))]
    for n in ("force_proj1", "force_proj2", "force_proj3"):
        out += [(f"node_proj.{n}.weight", (1, E)), (f"node_proj.{n}.bias", (1,))]
    return out


def _rng(name, seed):
    return np.random.default_rng([zlib.crc32(name.encode()), seed])


def make_params(cfg, seed=0):
    """Deterministic float64 weights keyed by parameter name.  Scaled so that the energies are O(1) instead of the 1e-3 of the default initialisation:
    unit-variance embeddings, energy_agg_factor of order 1, a spread of mul / bias over the edge types; |stds| in [0.3, 3] with both signs."""
    out = OrderedDict()
    for name, shape in param_shapes(cfg):
        g = _rng(name, seed)
        if name in ("gbf.means.weight",):
            w = g.uniform(0.0, 3.0, size=shape)
        elif name == "gbf.stds.weight":
            w = g.uniform(0.3, 3.0, size=shape) * np.where(g.uniform(size=shape) < 0.25, -1.0, 1.0)
        elif name == "gbf.mul.weight":
            w = 1.0 + 0.2 * g.normal(size=shape)
        elif name == "gbf.bias.weight":
            w = 0.2 * g.normal(size=shape)
        elif name in ("atom_encoder.weight", "tag_encoder.weight", "energy_agg_factor.weight"):
            w = g.normal(size=shape)
            if name == "atom_encoder.weight":
                w[0] = 0.0                                  # padding_idx = 0
        elif "layer_norm" in name or name.startswith("final_ln"):
            w = (1.0 if name.endswith("weight") else 0.0) + 0.1 * g.normal(size=shape)
        elif name.endswith(".bias"):
            w = 0.1 * g.normal(size=shape)
        else:
            w = g.normal(size=shape) / math.sqrt(shape[-1])
        out[name] = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64))
    return out


def probe_direction(name, shape):
    """Seeded unit direction of a gradient tensor (the yaml fixture stores norm and projection instead of the tensor)."""
    d = _rng("probe:" + name, 0).normal(size=shape)
    return torch.from_numpy(d / np.linalg.norm(d))


# ---- operators --------------------------------------------------------------------------------------------------------------------------------------------
GAUSS_A = (2 * 3.14159) ** 0.5          # the reference's truncated pi (:121-122)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_backward(x, g):
    return g * (0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def pair_geometry(pos, z, ptr):
    """dist [P], unit [P, 3], edge type [P], row atom [P] of all ordered pairs."""
    dist, unit, et, row = [], [], [], []
    for b in range(len(ptr) - 1):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        p = pos[a0:a1]
        delta = p.unsqueeze(0) - p.unsqueeze(1)                      # [i, j] = pos_j - pos_i  (:283)
        d = delta.norm(dim=-1)
        dist.append(d.reshape(-1))
        unit.append((delta / (d.unsqueeze(-1) + 1e-5)).reshape(-1, 3))
        zz = z[a0:a1]
        et.append((zz.view(-1, 1) * ATOM_TYPES + zz.view(1, -1)).reshape(-1))
        row.append(torch.arange(a0, a1).view(-1, 1).expand(-1, a1 - a0).reshape(-1))
    return torch.cat(dist), torch.cat(unit), torch.cat(et), torch.cat(row)


def gaussian_basis(dist, et, mul, bias, means, stds):
    x = mul.reshape(-1)[et] * dist + bias.reshape(-1)[et]
    std = stds.reshape(-1).abs() + 1e-5
    u = (x.unsqueeze(-1) - means.reshape(-1)) / std
    return torch.exp(-0.5 * u * u) / (GAUSS_A * std)


def pair_features(pos, z, ptr, mul, bias, means, stds):
    """-> gbf [P, K], unit [P, 3], dist [P], efeat [N, K] (= sum over j of gbf[(i, j)])."""
    dist, unit, et, row = pair_geometry(pos, z, ptr)
    gbf = gaussian_basis(dist, et, mul, bias, means, stds)
    efeat = torch.zeros(pos.shape[0], gbf.shape[1], dtype=gbf.dtype).index_add_(0, row, gbf)
    return gbf, unit, dist, efeat


def pair_features_backward(pos, z, ptr, mul, bias, means, stds, g_gbf, g_efeat):
    """Analytic adjoints (g_means [K], g_stds [K], g_mul [4096], g_bias [4096]) of pair_features; g_gbf [P, K] and g_efeat [N, K], either may be None."""
    dist, _, et, row = pair_geometry(pos, z, ptr)
    x = mul.reshape(-1)[et] * dist + bias.reshape(-1)[et]
    s_raw = stds.reshape(-1)
    s = s_raw.abs() + 1e-5
    u = (x.unsqueeze(-1) - means.reshape(-1)) / s
    gbf = torch.exp(-0.5 * u * u) / (GAUSS_A * s)
    G = torch.zeros_like(gbf)
    if g_gbf is not None:
        G = G + g_gbf
    if g_efeat is not None:
        G = G + g_efeat[row]
    w = G * gbf / s
    g_means = (w * u).sum(0)
    g_stds = (w * (u * u - 1.0)).sum(0) * torch.sign(s_raw)
    gx = -(w * u).sum(-1)
    g_mul = torch.zeros(EDGE_TYPES, dtype=gbf.dtype).index_add_(0, et, gx * dist)
    g_bias = torch.zeros(EDGE_TYPES, dtype=gbf.dtype).index_add_(0, et, gx)
    return g_means, g_stds, g_mul, g_bias


def _probs(qkv, bias_pm, a0, a1, p0, H, scaling):
    n, E = a1 - a0, qkv.shape[1] // 3
    d = E // H
    q = qkv[a0:a1, :E].reshape(n, H, d).transpose(0, 1) * scaling
    k = qkv[a0:a1, E:2 * E].reshape(n, H, d).transpose(0, 1)
    v = qkv[a0:a1, 2 * E:].reshape(n, H, d).transpose(0, 1)
    S = q @ k.transpose(1, 2) + bias_pm[p0:p0 + n * n].reshape(n, n, H).permute(2, 0, 1)
    return q, k, v, torch.softmax(S, dim=-1)


def _keep(keep_pm, mask_scale, p0, n, H, dtype):
    if keep_pm is None:
        return None
    return keep_pm[p0:p0 + n * n].reshape(n, n, H).permute(2, 0, 1).to(dtype) * mask_scale


def attention(qkv, bias_pm, ptr, pair_ptr, H, scaling, keep_pm=None, mask_scale=1.0):
    """:40-59 between in_proj and out_proj.  qkv [N, 3E]; bias_pm [P, H]; keep_pm [P, H] (0 / 1) or None.  -> [N, E]."""
    out = []
    for b in range(len(ptr) - 1):
        a0, a1, p0 = int(ptr[b]), int(ptr[b + 1]), int(pair_ptr[b])
        n = a1 - a0
        q, k, v, P = _probs(qkv, bias_pm, a0, a1, p0, H, scaling)
        m = _keep(keep_pm, mask_scale, p0, n, H, P.dtype)
        if m is not None:
            P = P * m
        out.append((P @ v).transpose(0, 1).reshape(n, -1))
    return torch.cat(out)


def _softmax_backward(P, gPm, m):
    gP = gPm if m is None else gPm * m
    return P * (gP - (P * gP).sum(-1, keepdim=True))


def attention_backward(qkv, bias_pm, ptr, pair_ptr, H, scaling, g_out, keep_pm=None, mask_scale=1.0):
    """-> g_qkv [N, 3E], g_bias_pm [P, H]."""
    E = qkv.shape[1] // 3
    g_qkv, g_bias = [], []
    for b in range(len(ptr) - 1):
        a0, a1, p0 = int(ptr[b]), int(ptr[b + 1]), int(pair_ptr[b])
        n = a1 - a0
        q, k, v, P = _probs(qkv, bias_pm, a0, a1, p0, H, scaling)
        m = _keep(keep_pm, mask_scale, p0, n, H, P.dtype)
        go = g_out[a0:a1].reshape(n, H, -1).transpose(0, 1)
        gS = _softmax_backward(P, go @ v.transpose(1, 2), m)
        Pm = P if m is None else P * m
        gq, gk, gv = gS @ k * scaling, gS.transpose(1, 2) @ q, Pm.transpose(1, 2) @ go
        g_qkv.append(torch.cat([t.transpose(0, 1).reshape(n, E) for t in (gq, gk, gv)], dim=1))
        g_bias.append(gS.permute(1, 2, 0).reshape(n * n, H))
    return torch.cat(g_qkv), torch.cat(g_bias)


def force_head(qkv, bias_pm, unit, W3, b3, ptr, pair_ptr, H, scaling, keep_pm=None, mask_scale=1.0):
    """:202-224 after q_proj / k_proj / v_proj: x[i, c, h, :] = sum_j P_hij unit[(i, j), c] v_jh; f[i, c] = W3[c] . x[i, c] + b3[c].  -> [N, 3]."""
    out = []
    for b in range(len(ptr) - 1):
        a0, a1, p0 = int(ptr[b]), int(ptr[b + 1]), int(pair_ptr[b])
        n = a1 - a0
        q, k, v, P = _probs(qkv, bias_pm, a0, a1, p0, H, scaling)
        m = _keep(keep_pm, mask_scale, p0, n, H, P.dtype)
        if m is not None:
            P = P * m
        u = unit[p0:p0 + n * n].reshape(n, n, 3)
        x = torch.einsum("hij,ijc,hjd->ichd", P, u, v).reshape(n, 3, -1)
        out.append((x * W3.unsqueeze(0)).sum(-1) + b3)
    return torch.cat(out)


def force_head_backward(qkv, bias_pm, unit, W3, ptr, pair_ptr, H, scaling, g_f, keep_pm=None, mask_scale=1.0):
    """-> g_qkv [N, 3E], g_bias_pm [P, H], g_W3 [3, E], g_b3 [3]."""
    E = qkv.shape[1] // 3
    g_qkv, g_bias, g_W3 = [], [], torch.zeros_like(W3)
    for b in range(len(ptr) - 1):
        a0, a1, p0 = int(ptr[b]), int(ptr[b + 1]), int(pair_ptr[b])
        n = a1 - a0
        q, k, v, P = _probs(qkv, bias_pm, a0, a1, p0, H, scaling)
        m = _keep(keep_pm, mask_scale, p0, n, H, P.dtype)
        Pm = P if m is None else P * m
        u = unit[p0:p0 + n * n].reshape(n, n, 3)
        gf = g_f[a0:a1]
        x = torch.einsum("hij,ijc,hjd->ichd", Pm, u, v).reshape(n, 3, -1)
        g_W3 = g_W3 + (gf.unsqueeze(-1) * x).sum(0)
        gx = (gf.unsqueeze(-1) * W3.unsqueeze(0)).reshape(n, 3, H, -1)                    # [i, c, h, d]
        gPm = torch.einsum("ichd,ijc,hjd->hij", gx, u, v)
        gv = torch.einsum("hij,ijc,ichd->hjd", Pm, u, gx)
        gS = _softmax_backward(P, gPm, m)
        gq, gk = gS @ k * scaling, gS.transpose(1, 2) @ q
        g_qkv.append(torch.cat([t.transpose(0, 1).reshape(n, E) for t in (gq, gk, gv)], dim=1))
        g_bias.append(gS.permute(1, 2, 0).reshape(n * n, H))
    return torch.cat(g_qkv), torch.cat(g_bias), g_W3, g_f.sum(0)


# ---- the model --------------------------------------------------------------------------------------------------------------------------------------------
def _lin(p, name, x):
    return x @ p[name + ".weight"].t() + p[name + ".bias"]


def _ln(p, name, x):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), p[name + ".weight"], p[name + ".bias"], 1e-5)


def forward(p, cfg, z, pos, sizes):
    """eval()-mode forward on real atoms.  -> dict(energy [B], forces [N, 3], gbf, efeat, bias [P, H], layer_out [blocks * layers, N, E])."""
    ptr, pair_ptr, atom_mol = structure(sizes)
    H, E = cfg["attention_heads"], cfg["embed_dim"]
    scaling = (E // H) ** -0.5
    gbf, unit, _, efeat = pair_features(pos, z, ptr, p["gbf.mul.weight"], p["gbf.bias.weight"], p["gbf.means.weight"], p["gbf.stds.weight"])
    x = p["tag_encoder.weight"][1] + p["atom_encoder.weight"][z] + _lin(p, "edge_proj", efeat)
    bias = _lin(p, "bias_proj.layer2", gelu(_lin(p, "bias_proj.layer1", gbf)))
    layer_out = []
    for _ in range(cfg["blocks"]):
        for l in range(cfg["layers"]):
            pre = f"layers.{l}."
            r = x
            a = attention(_lin(p, pre + "self_attn.in_proj", _ln(p, pre + "self_attn_layer_norm", x)), bias, ptr, pair_ptr, H, scaling)
            x = r + _lin(p, pre + "self_attn.out_proj", a)
            r = x
            x = r + _lin(p, pre + "fc2", gelu(_lin(p, pre + "fc1", _ln(p, pre + "final_layer_norm", x))))
            layer_out.append(x)
    out = _ln(p, "final_ln", x)
    e_atom = _lin(p, "energy_proj.layer2", gelu(_lin(p, "energy_proj.layer1", out))) * p["energy_agg_factor.weight"][1]
    energy = torch.zeros(len(sizes), dtype=out.dtype).index_add_(0, atom_mol, e_atom.reshape(-1))
    qkv = torch.cat([_lin(p, "node_proj." + n, out) for n in ("q_proj", "k_proj", "v_proj")], dim=1)
    W3 = torch.cat([p[f"node_proj.force_proj{c}.weight"] for c in (1, 2, 3)])
    b3 = torch.cat([p[f"node_proj.force_proj{c}.bias"] for c in (1, 2, 3)])
    forces = force_head(qkv, bias, unit, W3, b3, ptr, pair_ptr, H, scaling)
    return dict(energy=energy, forces=forces, gbf=gbf, efeat=efeat, bias=bias, layer_out=torch.stack(layer_out))


def lightning_loss(energy, forces, y, forces_target, sizes, energy_coef=1.0, forces_coef=1.0):
    """Graphormer3DLightning.step with torch.nn.L1Loss (:351-359): the force loss is a mean over the PADDED dense [B, n_max, 3] tensors, zeros included."""
    loss_e = (energy - y).abs().mean()
    loss_f = (forces - forces_target).abs().sum() / (len(sizes) * max(sizes) * 3)
    return forces_coef * loss_f + energy_coef * loss_e


def loss_and_grads(p, cfg, batch):
    """-> (forward dict, loss, {name: gradient}) by float64 autograd through the restatement."""
    q = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in p.items())
    out = forward(q, cfg, batch["z"], batch["pos"], batch["sizes"])
    loss = lightning_loss(out["energy"], out["forces"], batch["y"], batch["forces"], batch["sizes"])
    grads = torch.autograd.grad(loss, list(q.values()), allow_unused=True)
    return out, loss, OrderedDict((k, torch.zeros_like(v) if g is None else g) for (k, v), g in zip(q.items(), grads))
