"""The DimeNet++ kernels of csrc/dimenet.hip one by one through the C ABI against float64 torch (tests/dimenet_ref.py), built from the kernel's own float32
inputs promoted to float64 (``Dv``: a device copy kept alive until the test ends).  Every output buffer starts as NaN, so an element a kernel never writes fails the comparison.

Bounds: the bases must stay, element by element, within 4 x the error ONE float32 rounding of the distance can cause, |f(d (1 + 2^-23)) - f(d)| + 2^-23 |f|
(computed from the restatement; the 4 is for the float32 distance arithmetic); the other forward kernels within 2e-6 of the output's maximum; the reverse
kernels within 5e-6 of each adjoint's norm.  The triplet kernels run twice and must agree bitwise.

Inputs: the small batch (molecules of 1, 2, 3, 9 and 24 atoms, at most 8 neighbours: E = 272, T = 1974; it holds edges without a triplet, edges without a
reverse edge, and rows where the excluded neighbour k = i is the first, the last and the only one -- asserted below) at the widths (I 64, S 7, R 6, Bs 8) and
(I 128, S 5, R 4, Bs 4).  No lane is mapped to a neighbour or a triplet, so there is no neighbour-cap case."""
import os

import numpy as np
import pytest
import torch

from tests import dimenet_ref as D
from tests.helpers import D as Dv, DEV, P, _release_copies, _report, bits, check, lib, nan_dev, st, twice  # noqa: F401  (_release_copies: autouse)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [dict(I=64, S=7, R=6, Bs=8), dict(I=128, S=5, R=4, Bs=4)]
CUTOFF, EXPONENT, K = 5.0, 5, 8
_G = {}


def _record(line):
    _report(line)                     # the suite's parity report (tests/helpers.py); a copy of these lines is kept as profiles/dimenet_parity.txt
    print(line)


def graph(sizes=D.SMALL_SIZES, seed=1, K_=K):
    """The batch's graph as the kernels take it (host tensors + device copies), built once."""
    key = (sizes, seed, K_)
    if key in _G:
        return _G[key]
    b = D.make_batch(sizes, seed)
    pos = b["pos"].float()
    src, dst = D.radius_graph(pos.double().numpy(), b["batch"].numpy(), CUTOFF, K_)
    N, E = len(pos), len(src)
    kj, ji, _, _, _ = D.triplets(src, dst, N)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))])
    order = np.argsort(src, kind="stable")
    src_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))])
    vec = pos.double()[dst] - pos.double()[src]
    d64 = vec.norm(dim=-1)
    g = dict(N=N, E=E, T=len(kj), pos=pos, src=src, dst=dst, kj=torch.from_numpy(kj), ji=torch.from_numpy(ji), d=d64.float(), u=(vec / d64[:, None]).float(),
             n_trip=np.bincount(ji, minlength=E))
    for k, a in (("row_ptr", row_ptr), ("src", src), ("dst", dst), ("src_order", order), ("src_ptr", src_ptr)):
        g["d_" + k] = torch.as_tensor(a, dtype=torch.int32).to(DEV)
    g["d_d"], g["d_u"] = g["d"].to(DEV), g["u"].to(DEV).contiguous()
    _G[key] = g
    return g


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def fwd_ok(name, got, ref64):
    g = got.detach().cpu().double()
    assert not torch.isnan(g).any(), f"{name}: elements never written"
    err = float((g - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30))
    _record(f"ops {name:34s} forward  err / max {err:.2e} (<= 2e-6)")
    assert err <= 2e-6, (name, err)


def rev_ok(name, got, ref64):
    g = got.detach().cpu().double()
    assert not torch.isnan(g).any(), f"{name}: elements never written"
    err = float((g - ref64).norm() / ref64.norm().clamp_min(1e-30))
    _record(f"ops {name:34s} reverse  err / norm {err:.2e} (<= 5e-6)")
    assert err <= 5e-6, (name, err)


def test_the_graph_holds_the_cases_the_triplet_kernels_must_pass():
    g = graph()
    src, dst = g["src"], g["dst"]
    assert g["E"] >= 200 and g["T"] >= 1000
    assert (g["n_trip"] == 0).any()
    pairs = set(zip(src.tolist(), dst.tolist()))
    assert any((i, j) not in pairs for j, i in pairs)                       # the neighbour cap bites: (k -> j) without (j -> k)
    first = last = only = False
    rows = {i: src[dst == i] for i in range(g["N"])}
    for j, i in zip(src, dst):
        r = rows[j]                                                          # the in-row of j, which the triplets of (j -> i) walk without k = i
        if i in r:
            only |= len(r) == 1
            first |= len(r) > 1 and r[0] == i
            last |= len(r) > 1 and r[-1] == i
    assert first and last and only


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_geometry_forward_and_backward():
    g = graph()
    E, N = g["E"], g["N"]
    vec32 = g["pos"][g["src"]] - g["pos"][g["dst"]]
    geom = torch.cat([vec32, vec32.double().norm(dim=-1, keepdim=True).float()], 1).contiguous()
    d, u = nan_dev(E), nan_dev(E, 3)
    check(lib().nq_dn_geom_forward(Dv(geom), E, P(d), P(u), st()))
    fwd_ok("geom d", d, geom[:, 3].double())
    fwd_ok("geom u", u, -geom[:, :3].double() / geom[:, 3:].double())
    gd, gu = rnd(1, E), rnd(2, E, 3)
    pos = g["pos"].double().requires_grad_(True)
    v = pos[g["dst"]] - pos[g["src"]]
    dd = v.norm(dim=-1)
    (ref,) = torch.autograd.grad((dd * gd.double()).sum() + ((v / dd[:, None]) * gu.double()).sum(), pos)

    def call():
        gvec, gpos = nan_dev(E, 3), nan_dev(N, 3)
        check(lib().nq_dn_geom_backward(P(g["d_d"]), P(g["d_u"]), Dv(gd), Dv(gu), P(g["d_row_ptr"]), P(g["d_src_order"]), P(g["d_src_ptr"]), N, E,
                                        P(gvec), P(gpos), st()))
        return (gpos,)
    (gpos,) = twice(call)
    rev_ok("geom grad_pos", gpos, ref)
    assert float(gpos[0].abs().max()) == 0.0                                # the lone atom


# ---- bases --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS, ids=lambda w: f"S{w['S']}R{w['R']}")
def test_basis_forward_within_one_rounding_of_the_distance(w):
    g = graph()
    S, R = w["S"], w["R"]
    d = torch.cat([g["d"], torch.linspace(0.7, 4.99, 64)])                  # the batch's distances (>= 1 A) and short ones, where float32 closed forms cancel
    E = d.numel()
    freq = (torch.arange(1, R + 1) * torch.pi + 0.1 * rnd(3, R)).float()
    table = D.bessel_table(S, R)
    f = lambda x: torch.cat(D.radial_bases(x, freq.double(), CUTOFF, EXPONENT, S, R, table, stable=True), 1)      # noqa: E731
    ref = f(d.double())
    bound = (f(d.double() * (1 + 2.0 ** -23)) - ref).abs() + 2.0 ** -23 * ref.abs()
    roots, norms = (torch.from_numpy(t).to(DEV).contiguous() for t in table)
    rbf, rad = nan_dev(E, R), nan_dev(E, S * R)
    check(lib().nq_dn_basis_forward(Dv(d), Dv(freq), P(roots), P(norms), E, S, R, CUTOFF, EXPONENT + 1, P(rbf), P(rad), st()))
    got = torch.cat([rbf, rad], 1).cpu().double()
    assert not torch.isnan(got).any()
    ratio = ((got - ref).abs() / bound.clamp_min(1e-300)).max()
    _record(f"ops basis S={S} R={R}: worst |kernel - float64| / (error of one float32 rounding of d) = {float(ratio):.3f} (<= 4)")
    assert float(ratio) <= 4.0


@pytest.mark.parametrize("w", WIDTHS, ids=lambda w: f"S{w['S']}R{w['R']}")
def test_basis_backward(w):
    g = graph()
    S, R, E = w["S"], w["R"], g["E"]
    freq = (torch.arange(1, R + 1) * torch.pi + 0.1 * rnd(3, R)).float()
    table = D.bessel_table(S, R)
    g_rbf, g_rad = rnd(4, E, R), rnd(5, E, S * R)
    d64, f64 = g["d"].double().requires_grad_(True), freq.double().requires_grad_(True)
    rbf, rad = D.radial_bases(d64, f64, CUTOFF, EXPONENT, S, R, table, stable=True)
    ref_d, ref_f = torch.autograd.grad((rbf * g_rbf.double()).sum() + (rad * g_rad.double()).sum(), [d64, f64])
    roots, norms = (torch.from_numpy(t).to(DEV).contiguous() for t in table)
    gd, rows = nan_dev(E), nan_dev(E, R)
    check(lib().nq_dn_basis_backward(P(g["d_d"]), Dv(freq), P(roots), P(norms), E, S, R, CUTOFF, EXPONENT + 1, Dv(g_rbf), Dv(g_rad), P(gd),
                                     P(rows), st()))
    rev_ok(f"basis S={S} grad_d", gd, ref_d)
    rev_ok(f"basis S={S} grad_freq", rows.cpu().double().sum(0), ref_f)


# ---- triplet product ----------------------------------------------------------------------------------------------------------------------------------------------
def _triplet_ref(g, x, Q, u, W2, S, Bs):
    kj, ji = g["kj"], g["ji"]
    c = (u[ji] * u[kj]).sum(-1)
    s = (D.legendre_y(c, S).unsqueeze(-1) * Q[kj].view(-1, S, Bs)).sum(1)
    return torch.zeros(g["E"], W2.shape[0], dtype=x.dtype).index_add_(0, ji, x[kj] * (s @ W2.t()))


def _triplet_inputs(g, w):
    E = g["E"]
    return rnd(10, E, w["I"]), rnd(11, E, w["S"] * w["Bs"]), g["u"], rnd(12, w["I"], w["Bs"]) / w["Bs"] ** 0.5


@pytest.mark.parametrize("w", WIDTHS, ids=lambda w: f"I{w['I']}S{w['S']}")
def test_triplet_forward(w):
    g = graph()
    E, I, S, Bs = g["E"], w["I"], w["S"], w["Bs"]
    x, Q, u, W2 = _triplet_inputs(g, w)
    dx, dQ, dW = x.to(DEV), Q.to(DEV), W2.to(DEV)

    def call():
        m = nan_dev(E, I)
        check(lib().nq_dn_triplet_forward(P(dx), P(dQ), P(g["d_u"]), P(dW), P(g["d_row_ptr"]), P(g["d_src"]), P(g["d_dst"]), E, I, S, Bs, P(m), st()))
        return (m,)
    (m,) = twice(call)
    fwd_ok(f"triplet I={I} S={S}", m, _triplet_ref(g, x.double(), Q.double(), u.double(), W2.double(), S, Bs))
    assert float(m.cpu()[torch.from_numpy(g["n_trip"] == 0)].abs().max()) == 0.0            # edges without a triplet


@pytest.mark.parametrize("w", WIDTHS, ids=lambda w: f"I{w['I']}S{w['S']}")
def test_triplet_backward(w):
    g = graph()
    E, I, S, Bs = g["E"], w["I"], w["S"], w["Bs"]
    x, Q, u, W2 = _triplet_inputs(g, w)
    gm = rnd(13, E, I)
    leaves = [t.double().requires_grad_(True) for t in (x, Q, u, W2)]
    refs = torch.autograd.grad((_triplet_ref(g, *leaves, S, Bs) * gm.double()).sum(), leaves)
    dx, dQ, dW, dgm = x.to(DEV), Q.to(DEV), W2.to(DEV), gm.to(DEV)
    scr = torch.empty(int(lib().nq_dn_triplet_scratch_floats(E, I, Bs)) + 64, device=DEV)

    def call(with_w=True):
        gx, gQ, gu, gW = nan_dev(E, I), nan_dev(E, S * Bs), nan_dev(E, 3), nan_dev(I, Bs)
        check(lib().nq_dn_triplet_backward(P(dx), P(dQ), P(g["d_u"]), P(dW), P(g["d_row_ptr"]), P(g["d_src"]), P(g["d_dst"]), P(g["d_src_order"]), P(g["d_src_ptr"]),
                                           E, I, S, Bs, P(dgm), P(gx), P(gQ), P(gu), P(gW) if with_w else None, P(scr) if with_w else None, st()))
        return gx, gQ, gu, gW
    got = twice(call)
    for name, a, r in zip(("grad_x", "grad_Q", "grad_u", "grad_W_sbf2"), got, refs):
        rev_ok(f"triplet I={I} {name}", a, r)
    lean = call(with_w=False)                                                # without the weight gradient: the same adjoints, the weight buffer untouched
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got[:3], lean[:3])) and torch.isnan(lean[3]).all()


def test_triplet_forward_allocates_nothing_of_the_size_of_the_triplets():
    from nabladft_amd.dimenetplusplus import _TripletFn
    from types import SimpleNamespace
    g = graph(sizes=(45, 45, 45), seed=7, K_=32)
    assert g["T"] >= 100000
    E, I, S, Bs = g["E"], 64, 7, 8
    x, Q, W2 = rnd(20, E, I).to(DEV), rnd(21, E, S * Bs).to(DEV), rnd(22, I, Bs).to(DEV)
    plan = SimpleNamespace(E=E, row_ptr=g["d_row_ptr"], src=g["d_src"], dst=g["d_dst"])
    with torch.no_grad():
        _TripletFn.apply(x, Q, g["d_u"], W2, plan, S)                     # loads the kernel's code object, which is not what is measured
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        m = _TripletFn.apply(x, Q, g["d_u"], W2, plan, S)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - m.numel() * 4
    _record(f"ops triplet forward at T = {g['T']}: peak device memory beyond inputs and output {extra} bytes (< 1 MiB; a [T, 64] array would be {g['T'] * 256})")
    assert extra < 1 << 20
    assert free0 - torch.cuda.mem_get_info()[0] < m.numel() * 4 + (4 << 20)           # nothing allocated behind torch's back either
    ref = _triplet_ref(g, x.cpu().double(), Q.cpu().double(), g["u"].double(), W2.cpu().double(), S, Bs)
    fwd_ok("triplet T=1e5", m, ref)


# ---- edge helpers -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [128, 96])
def test_gate_and_gated_sum(H):
    g = graph()
    E, N = g["E"], g["N"]
    x, gate, gy, go = rnd(30, E, H), rnd(31, E, H), rnd(32, E, H), rnd(33, N, H)
    dx, dg = x.to(DEV), gate.to(DEV)
    y, gx, gg = nan_dev(E, H), nan_dev(E, H), nan_dev(E, H)
    check(lib().nq_dn_gate_forward(P(dx), P(dg), E * H, P(y), st()))
    check(lib().nq_dn_gate_backward(P(dx), P(dg), Dv(gy), E * H, P(gx), P(gg), st()))
    fwd_ok("gate", y, x.double() * gate.double())
    rev_ok("gate grad_x", gx, gy.double() * gate.double()), rev_ok("gate grad_gate", gg, gy.double() * x.double())
    dst = torch.from_numpy(g["dst"])
    out, gx, gg = nan_dev(N, H), nan_dev(E, H), nan_dev(E, H)
    check(lib().nq_dn_gatesum_forward(P(dx), P(dg), P(g["d_row_ptr"]), N, H, P(out), st()))
    check(lib().nq_dn_gatesum_backward(P(dx), P(dg), Dv(go), P(g["d_dst"]), E, H, P(gx), P(gg), st()))
    fwd_ok("gated sum", out, torch.zeros(N, H, dtype=torch.float64).index_add_(0, dst, x.double() * gate.double()))
    rev_ok("gated sum grad_x", gx, go.double()[dst] * gate.double()), rev_ok("gated sum grad_gate", gg, go.double()[dst] * x.double())
    assert float(out[0].abs().max()) == 0.0                                 # the lone atom has no in-edge


@pytest.mark.parametrize("H", [128, 96])
def test_embedding_block(H):
    g = graph()
    E, N = g["E"], g["N"]
    AB, Cr, bias, gy = rnd(40, N, 2 * H), rnd(41, E, H), rnd(42, H), rnd(43, E, H)
    src, dst = torch.from_numpy(g["src"]), torch.from_numpy(g["dst"])
    leaves = [t.double().requires_grad_(True) for t in (AB, Cr, bias)]
    pre64 = leaves[0][dst, :H] + leaves[0][src, H:] + leaves[1] + leaves[2]
    y64 = pre64 * torch.sigmoid(pre64)
    refs = torch.autograd.grad((y64 * gy.double()).sum(), leaves)
    pre, y, gpre, gAB = nan_dev(E, H), nan_dev(E, H), nan_dev(E, H), nan_dev(N, 2 * H)
    check(lib().nq_dn_embed_forward(Dv(AB), Dv(Cr), Dv(bias), P(g["d_src"]), P(g["d_dst"]), E, H, P(pre), P(y), st()))
    check(lib().nq_dn_embed_backward(P(pre), Dv(gy), P(g["d_row_ptr"]), P(g["d_src_order"]), P(g["d_src_ptr"]), N, E, H, P(gpre), P(gAB), st()))
    fwd_ok("embed pre", pre, pre64.detach()), fwd_ok("embed y", y, y64.detach())
    rev_ok("embed grad_AB", gAB, refs[0]), rev_ok("embed grad_Cr", gpre, refs[1]), rev_ok("embed grad_bias", gpre.cpu().double().sum(0), refs[2])
