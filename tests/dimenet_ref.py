"""Torch restatement of the DimeNet++ core (torch_geometric.nn.models.DimeNetPlusPlus, 2.4.0, as DESIGN_details.md "DimeNet++" states it), materialised the way
torch-geometric does it: an edge index list, triplet index lists and a [T, S * R] spherical basis.  float64 or float32; ``exact_basis`` evaluates the bases in
float64 and rounds them once (the yardstick of the GPU tests).  scripts/make_golden_dimenet.py installs ``DimeNetPlusPlus`` as the class the reference's
wrapper imports.  RESTATED, UNPINNED: torch-geometric is not available to check it against; the wrapper around it is the reference's own."""
import math
import zlib
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

ELEMENTS = np.array([1, 6, 7, 8, 9, 16, 17, 35])
SMALL = dict(node_latent_dim=50, dimenet_hidden_channels=128, dimenet_num_blocks=2, dimenet_int_emb_size=64, dimenet_basis_emb_size=8,
             dimenet_out_emb_channels=256, dimenet_num_spherical=7, dimenet_num_radial=6, dimenet_max_num_neighbors=8, cutoff=5.0)
YAML = dict(node_latent_dim=50, dimenet_hidden_channels=256, dimenet_num_blocks=6, dimenet_int_emb_size=64, dimenet_basis_emb_size=8,
            dimenet_out_emb_channels=256, dimenet_num_spherical=7, dimenet_num_radial=6, dimenet_max_num_neighbors=32, cutoff=5.0)
SMALL_SIZES, YAML_SIZES = (1, 2, 3, 9, 24), (1, 2, 3, 17, 42)
SCALER = {"scale_": 3.5, "mean_": -7.25}


def core_kwargs(cfg):
    return dict(hidden_channels=cfg["dimenet_hidden_channels"], out_channels=cfg["node_latent_dim"], num_blocks=cfg["dimenet_num_blocks"],
                int_emb_size=cfg["dimenet_int_emb_size"], basis_emb_size=cfg["dimenet_basis_emb_size"], out_emb_channels=cfg["dimenet_out_emb_channels"],
                num_spherical=cfg["dimenet_num_spherical"], num_radial=cfg["dimenet_num_radial"], cutoff=cfg["cutoff"],
                max_num_neighbors=cfg["dimenet_max_num_neighbors"])


def _rng(name, seed):
    return np.random.default_rng([zlib.crc32(name.encode()), seed])


def make_batch(sizes, seed):
    """Random compact conformers, every distance >= 1 A (random sequential placement); targets y [B], forces [N, 3].  float64."""
    rng = np.random.default_rng(seed)
    zs, ps, bs = [], [], []
    for b, n in enumerate(sizes):
        side = 1.7 * max(n, 1) ** (1.0 / 3.0)
        pts = []
        while len(pts) < n:
            p = rng.uniform(0.0, side, size=3)
            if all(np.linalg.norm(p - q) >= 1.0 for q in pts):
                pts.append(p)
        ps.append(np.array(pts).reshape(n, 3) + rng.normal(size=3) * 3.0)
        zs.append(rng.choice(ELEMENTS, size=n))
        bs.append(np.full(n, b))
    N = int(sum(sizes))
    return dict(z=torch.from_numpy(np.concatenate(zs).astype(np.int64)), pos=torch.from_numpy(np.concatenate(ps)), batch=torch.from_numpy(np.concatenate(bs)),
                y=torch.from_numpy(rng.normal(size=len(sizes))), forces=torch.from_numpy(rng.normal(size=(N, 3)) * 0.5), sizes=tuple(int(n) for n in sizes))


def probe_direction(name, shape):
    d = _rng("probe:" + name, 0).normal(size=shape)
    return torch.from_numpy(d / np.linalg.norm(d))


# ---- graph and triplets ---------------------------------------------------------------------------------------------------------------------------------------
def radius_graph(pos, batch, cutoff, K):
    """Directed edges (j -> i): per target i the first K atoms of its molecule, in index order, with |pos_i - pos_j| < cutoff.  -> (src j [E], dst i [E]),
    sorted by target, sources ascending."""
    pos, batch = np.asarray(pos, dtype=np.float64), np.asarray(batch)
    src, dst = [], []
    for i in range(len(pos)):
        kept = 0
        for j in np.nonzero(batch == batch[i])[0]:
            if j != i and kept < K and np.linalg.norm(pos[i] - pos[j]) < cutoff:
                src.append(j), dst.append(i)
                kept += 1
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)


def triplets(src, dst, N):
    """(idx_kj, idx_ji, idx_i, idx_j, idx_k): for every edge e = (j -> i), every edge (k -> j) with k != i."""
    into = [[] for _ in range(N)]
    for e, i in enumerate(dst):
        into[i].append(e)
    kj, ji = [], []
    for e, (j, i) in enumerate(zip(src, dst)):
        for e2 in into[j]:
            if src[e2] != i:
                kj.append(e2), ji.append(e)
    kj, ji = np.array(kj, dtype=np.int64), np.array(ji, dtype=np.int64)
    return kj, ji, dst[ji], src[ji], src[kj]


# ---- bases ----------------------------------------------------------------------------------------------------------------------------------------------------
def _jl_np(l, x):
    x = np.asarray(x, dtype=np.float64)
    jm = np.sin(x) / x
    if l == 0:
        return jm
    j = (np.sin(x) / x - np.cos(x)) / x
    for n in range(1, l):
        jm, j = j, (2 * n + 1) / x * j - jm
    return j


def bessel_table(S, R):
    """Roots of j_l (l < S, the first R of each) by Newton iterations from interlacing brackets, and the normalisers (0.5 j_{l+1}(z)^2)^(-1/2).  float64."""
    points = np.arange(1, R + S, dtype=np.float64) * np.pi
    roots = np.zeros((S, R))
    roots[0] = points[:R]
    for l in range(1, S):
        new = []
        for a, b in zip(points[:-1], points[1:]):
            fa = _jl_np(l, a)
            for _ in range(60):                                 # bisection to ~1e-12, then Newton with j_l' = j_{l-1} - (l + 1) / x j_l
                m = 0.5 * (a + b)
                if (_jl_np(l, m) > 0) == (fa > 0):
                    a = m
                else:
                    b = m
            x = 0.5 * (a + b)
            for _ in range(3):
                f = _jl_np(l, x)
                x = x - f / (_jl_np(l - 1, x) - (l + 1) / x * f)
            new.append(float(x))
        points = np.array(new)
        roots[l] = points[:R]
    norms = np.stack([1.0 / np.sqrt(0.5 * _jl_np(l + 1, roots[l]) ** 2) for l in range(S)])
    return roots, norms


def _jl(l, x):
    """Closed form by the upward recurrence, in the dtype of x (what the generated closed forms do: it cancels like 1 / x^(l+1) for small x)."""
    jm = torch.sin(x) / x
    if l == 0:
        return jm
    j = (torch.sin(x) / x - torch.cos(x)) / x
    for n in range(1, l):
        jm, j = j, (2 * n + 1) / x * j - jm
    return j


def _jl_stable(l, x):
    """float64 j_l that is accurate for every x > 0: the power series where x < l, the recurrence elsewhere."""
    small = x < l
    xs = torch.where(small, x, torch.ones_like(x))
    pre = torch.ones_like(xs)
    for k in range(1, l + 1):
        pre = pre * xs / (2 * k + 1)
    a, s = torch.ones_like(xs), torch.ones_like(xs)
    for k in range(1, 40):
        a = a * (-0.5 * xs * xs) / (k * (2 * l + 2 * k + 1))
        s = s + a
    xl = torch.where(small, torch.full_like(x, float(max(l, 1))), x)
    return torch.where(small, pre * s, _jl(l, xl))


def envelope(x, exponent):
    p = exponent + 1
    a, b, c = -(p + 1) * (p + 2) / 2, p * (p + 2), -p * (p + 1) / 2
    xp0 = x.pow(p - 1)
    xp1 = xp0 * x
    return (1.0 / x + a * xp0 + b * xp1 + c * xp1 * x) * (x < 1.0).to(x.dtype)


def legendre_y(c, S):
    """Y_l0 = sqrt((2l + 1) / 4 pi) P_l(c), l < S -> [..., S]."""
    P = [torch.ones_like(c), c]
    for l in range(1, S - 1):
        P.append(((2 * l + 1) * c * P[l] - l * P[l - 1]) / (l + 1))
    return torch.stack([math.sqrt((2 * l + 1) / (4 * math.pi)) * P[l] for l in range(S)], -1)


def radial_bases(dist, freq, cutoff, exponent, S, R, table, stable=False):
    """(rbf [E, R], rad [E, S * R]) in the dtype of dist."""
    x = dist / cutoff
    env = envelope(x, exponent)
    rbf = env.unsqueeze(-1) * torch.sin(freq * x.unsqueeze(-1))
    roots, norms = (torch.as_tensor(t, dtype=dist.dtype) for t in table)
    fn = _jl_stable if stable else _jl
    rad = torch.stack([norms[l, n] * fn(l, roots[l, n] * x) for l in range(S) for n in range(R)], 1)
    return rbf, env.unsqueeze(-1) * rad


# ---- the module tree of torch_geometric.nn.models.DimeNetPlusPlus ---------------------------------------------------------------------------------------------
def swish(x):
    return x * x.sigmoid()


class _Holder(nn.Module):
    pass


def _linear(i, o, bias=True):
    return nn.Linear(i, o, bias=bias)


class DimeNetPlusPlus(nn.Module):
    def __init__(self, hidden_channels, out_channels, num_blocks, int_emb_size, basis_emb_size, out_emb_channels, num_spherical, num_radial, cutoff=5.0,
                 max_num_neighbors=32, envelope_exponent=5, num_before_skip=1, num_after_skip=2, num_output_layers=3):
        super().__init__()
        H, I, Bs, O, S, R = hidden_channels, int_emb_size, basis_emb_size, out_emb_channels, num_spherical, num_radial
        self.cfg = dict(H=H, I=I, Bs=Bs, O=O, S=S, R=R, cutoff=cutoff, K=max_num_neighbors, exponent=envelope_exponent)
        self.exact_basis = False
        self.record = None
        self.table = bessel_table(S, R)
        self.rbf = _Holder()
        self.rbf.freq = nn.Parameter(torch.arange(1, R + 1, dtype=torch.get_default_dtype()) * math.pi)
        self.emb = _Holder()
        self.emb.emb, self.emb.lin_rbf, self.emb.lin = nn.Embedding(95, H), _linear(R, H), _linear(3 * H, H)
        self.emb.emb.weight.data.uniform_(-math.sqrt(3), math.sqrt(3))
        self.output_blocks, self.interaction_blocks = nn.ModuleList(), nn.ModuleList()
        for _ in range(num_blocks + 1):
            o = _Holder()
            o.lin_rbf, o.lin_up = _linear(R, H, False), _linear(H, O, False)
            o.lins = nn.ModuleList([_linear(O, O) for _ in range(num_output_layers)])
            o.lin = _linear(O, out_channels, False)
            o.lin.weight.data.fill_(0)
            self.output_blocks.append(o)
        for _ in range(num_blocks):
            b = _Holder()
            b.lin_rbf1, b.lin_rbf2 = _linear(R, Bs, False), _linear(Bs, H, False)
            b.lin_sbf1, b.lin_sbf2 = _linear(S * R, Bs, False), _linear(Bs, I, False)
            b.lin_kj, b.lin_ji = _linear(H, H), _linear(H, H)
            b.lin_down, b.lin_up = _linear(H, I, False), _linear(I, H, False)
            b.layers_before_skip = nn.ModuleList([self._res(H) for _ in range(num_before_skip)])
            b.lin = _linear(H, H)
            b.layers_after_skip = nn.ModuleList([self._res(H) for _ in range(num_after_skip)])
            self.interaction_blocks.append(b)

    @staticmethod
    def _res(H):
        r = _Holder()
        r.lin1, r.lin2 = _linear(H, H), _linear(H, H)
        return r

    @staticmethod
    def _residual(r, h):
        return h + swish(r.lin2(swish(r.lin1(h))))

    def _output(self, o, x, rbf, i, N):
        h = torch.zeros(N, x.shape[1], dtype=x.dtype).index_add_(0, i, o.lin_rbf(rbf) * x)
        h = o.lin_up(h)
        for lin in o.lins:
            h = swish(lin(h))
        return o.lin(h)

    def forward(self, z, pos, batch=None):
        c = self.cfg
        S, R = c["S"], c["R"]
        N = pos.shape[0]
        batch = torch.zeros(N, dtype=torch.long) if batch is None else batch
        src, dst = radius_graph(pos.detach().numpy(), batch.numpy(), c["cutoff"], c["K"])
        kj, ji, ti, tj, tk = (torch.from_numpy(a) for a in triplets(src, dst, N))
        j, i = torch.from_numpy(src), torch.from_numpy(dst)
        dist = (pos[i] - pos[j]).pow(2).sum(-1).sqrt()
        pos_jk, pos_ij = pos[tj] - pos[tk], pos[ti] - pos[tj]
        a = (pos_ij * pos_jk).sum(-1)
        b = torch.linalg.cross(pos_ij, pos_jk).norm(dim=-1)
        angle = torch.atan2(b, a)
        freq = self.rbf.freq
        if self.exact_basis:
            rbf, rad = (t.to(pos.dtype) for t in radial_bases(dist.double(), freq.double(), c["cutoff"], c["exponent"], S, R, self.table, stable=True))
            cbf = legendre_y(torch.cos(angle.double()), S).to(pos.dtype)
        else:
            rbf, rad = radial_bases(dist, freq, c["cutoff"], c["exponent"], S, R, self.table, stable=pos.dtype == torch.float64)
            cbf = legendre_y(torch.cos(angle), S)
        sbf = (rad[kj].view(-1, S, R) * cbf.view(-1, S, 1)).view(-1, S * R)
        e = self.emb
        x = swish(e.lin(torch.cat([e.emb(z)[i], e.emb(z)[j], swish(e.lin_rbf(rbf))], -1)))
        P = self._output(self.output_blocks[0], x, rbf, i, N)
        rec = dict(src=src, dst=dst, n_triplets=np.bincount(ji.numpy(), minlength=len(src)), rbf=rbf, rad=rad, sin_min=float(torch.sin(angle.detach()).abs().min()) if len(kj) else 1.0,
                   dist_min=float(dist.detach().min()) if len(src) else 9.0, block_out=[x])
        for blk, out in zip(self.interaction_blocks, self.output_blocks[1:]):
            x_ji, x_kj = swish(blk.lin_ji(x)), swish(blk.lin_kj(x))
            x_kj = x_kj * blk.lin_rbf2(blk.lin_rbf1(rbf))
            x_kj = swish(blk.lin_down(x_kj))
            t = x_kj[kj] * blk.lin_sbf2(blk.lin_sbf1(sbf))
            m = torch.zeros(len(src), t.shape[1], dtype=t.dtype).index_add_(0, ji, t)
            h = x_ji + swish(blk.lin_up(m))
            for r in blk.layers_before_skip:
                h = self._residual(r, h)
            h = swish(blk.lin(h)) + x
            for r in blk.layers_after_skip:
                h = self._residual(r, h)
            x = h
            P = P + self._output(out, x, rbf, i, N)
            rec["block_out"].append(x)
        B = int(batch.max()) + 1
        out = torch.zeros(B, P.shape[1], dtype=P.dtype).index_add_(0, batch, P)
        rec["P"] = out
        self.record = rec
        return out


# ---- parameters -------------------------------------------------------------------------------------------------------------------------------------------------
class Potential(nn.Module):
    """The wrapper's arithmetic (dimenetplusplus.py:22-113) around the restated core; the fixtures are produced by the REAL wrapper class, this one only lets the
    tests re-run the function without the reference tree."""

    def __init__(self, cfg, scaler=None, do_postprocessing=False):
        super().__init__()
        self.net = DimeNetPlusPlus(**core_kwargs(cfg))
        n = cfg["node_latent_dim"]
        self.regr_or_cls_nn = nn.Sequential(nn.Linear(n, n), nn.SiLU(), nn.Linear(n, n // 2), nn.SiLU(), nn.Linear(n // 2, n // 2), nn.SiLU(), nn.Linear(n // 2, 1))
        self.scaler, self.do_postprocessing = scaler, do_postprocessing

    def forward(self, z, pos, batch):
        with torch.enable_grad():
            pos = pos.detach().requires_grad_(True)
            pred = torch.flatten(self.regr_or_cls_nn(self.net(z, pos, batch)))
            forces = -torch.autograd.grad(pred.sum(), pos, create_graph=False, retain_graph=True)[0]
        unscaled = pred
        if self.scaler and self.do_postprocessing:
            pred = self.scaler["scale_"] * pred + self.scaler["mean_"]
        return pred, forces, unscaled


def param_shapes(cfg):
    """[(name, shape)] in state_dict order."""
    return [(k, tuple(v.shape)) for k, v in Potential(cfg).state_dict().items()]


def make_params(cfg, seed=0):
    """Deterministic float64 weights keyed by parameter name.  EVERY parameter is random, the zero-initialised output_blocks.*.lin.weight included (with the
    default initialisation the energy does not depend on the positions).  Scales keep the activations O(1) through the blocks."""
    out = OrderedDict()
    R = cfg["dimenet_num_radial"]
    for name, shape in param_shapes(cfg):
        g = _rng(name, seed)
        if name == "net.rbf.freq":
            w = np.arange(1, R + 1) * np.pi + 0.1 * g.normal(size=shape)
        elif name == "net.emb.emb.weight":
            w = g.uniform(-math.sqrt(3), math.sqrt(3), size=shape)
        elif name.endswith(".bias"):
            w = 0.1 * g.normal(size=shape)
        else:
            fan_in = shape[-1]
            gain = 1.0
            if "lin_rbf" in name or "lin_sbf1" in name:
                gain = 0.5                      # the bases reach ~10 at short distances
            w = gain * g.normal(size=shape) / math.sqrt(fan_in)
        out[name] = torch.from_numpy(np.asarray(w, dtype=np.float64))
    return out


def build(cfg, params, dtype=torch.float64, exact_basis=False, scaler=None, do_postprocessing=False):
    model = Potential(cfg, scaler, do_postprocessing).to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in params.items()})
    model.net.exact_basis = exact_basis
    return model


def run(cfg, params, b, dtype=torch.float64, exact_basis=False, grads=True):
    """-> dict: energy, forces, rbf, rad, block_out, P, loss (mean |E - y|) and its gradients by parameter name."""
    model = build(cfg, params, dtype, exact_basis)
    E, F, _ = model(b["z"], b["pos"].to(dtype), b["batch"])
    rec = model.net.record
    out = dict(energy=E.detach(), forces=F.detach(), rbf=rec["rbf"].detach(), rad=rec["rad"].detach(), block_out=[x.detach() for x in rec["block_out"]],
               P=rec["P"].detach(), src=rec["src"], dst=rec["dst"], n_triplets=rec["n_triplets"], sin_min=rec["sin_min"], dist_min=rec["dist_min"])
    if grads:
        loss = (E - b["y"].to(dtype)).abs().mean()
        gs = torch.autograd.grad(loss, list(model.parameters()), allow_unused=True)
        out["loss"] = loss.detach()
        out["grads"] = OrderedDict((k, (torch.zeros_like(p) if g is None else g).detach()) for (k, p), g in zip(model.named_parameters(), gs))
    return out
