"""The second-sweep kernels of csrc/dimenet.hip (``nq_dnt_*``: what a loss on the forces needs) one by one through the C ABI, and every autograd wrapper of
nabladft_amd.dimenetplusplus by double backward, against float64 torch: torch.autograd's own double backward (tests/dimenet_force_ref.second_sweep) of the
restated operations of tests/test_dimenet_ops_gpu.py (``_triplet_ref``, ``D.radial_bases(stable=True)``, the geometry), built from the kernel's own float32
inputs promoted to float64.  Every output buffer starts as NaN.

Bounds (the project's own, tests/test_dimenet_ops_gpu.py): forward-type outputs (the tangents mt, td, tu and a_g) within 2e-6 of the output's maximum, adjoints
within 5e-6 of the adjoint's norm; the basis tangent by the rule of the basis-backward test (5e-6 of the norm).  The triplet calls run twice and must agree
bitwise; each tangent argument is tested alone with the others NULL; a NULL tangent equals a zero tangent bitwise.

Inputs: the small graph of tests/test_dimenet_ops_gpu.py (E = 272, T = 1974: edges without a triplet, edges without a reverse edge, the excluded neighbour
first, last and only) at that file's two width sets and at I = 256 (four registers per lane)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import dimenet_force_ref as FR
from tests import dimenet_ref as D
from tests import test_dimenet_ops_gpu as O
from tests.helpers import D as Dv, DEV, P, _release_copies, bits, check, lib, nan_dev, st, twice  # noqa: F401  (_release_copies: autouse)

pytestmark = pytest.mark.gpu

WIDTHS = O.WIDTHS + [dict(I=256, S=7, R=6, Bs=8)]
rnd, fwd_ok, rev_ok = O.rnd, O.fwd_ok, O.rev_ok


def _same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_geometry_tangent():
    g = O.graph()
    E, N = g["E"], g["N"]
    tpos, gd, gu = rnd(50, N, 3), rnd(51, E), rnd(52, E, 3)
    src, dst = torch.from_numpy(g["src"]), torch.from_numpy(g["dst"])
    ref = FR.second_sweep(lambda pos: FR.geometry(pos, src, dst), (g["pos"],), (0,), (tpos,), (gd, gu), ())
    td, tu = nan_dev(E), nan_dev(E, 3)
    check(lib().nq_dnt_geom(P(g["d_d"]), P(g["d_u"]), Dv(tpos), P(g["d_src"]), P(g["d_dst"]), E, P(td), P(tu), st()))
    fwd_ok("tangent geom td", td, ref[0]), fwd_ok("tangent geom tu", tu, ref[1])


@pytest.mark.parametrize("w", O.WIDTHS, ids=lambda w: f"S{w['S']}R{w['R']}")
def test_basis_tangent(w):
    g = O.graph()
    S, R, E = w["S"], w["R"], g["E"]
    freq = (torch.arange(1, R + 1) * torch.pi + 0.1 * rnd(3, R)).float()
    table = D.bessel_table(S, R)
    t, g_rbf, g_rad = rnd(53, E), rnd(54, E, R), rnd(55, E, S * R)
    ref = FR.second_sweep(lambda d, f: D.radial_bases(d, f, O.CUTOFF, O.EXPONENT, S, R, table, stable=True), (g["d"], freq), (0,), (t,), (g_rbf, g_rad), (1,))
    roots, norms = (torch.from_numpy(a).to(DEV).contiguous() for a in table)
    dfreq, dt = freq.to(DEV), t.to(DEV)

    def call(grad_rbf):
        rbf_t, rad_t, rows = nan_dev(E, R), nan_dev(E, S * R), nan_dev(E, R)
        check(lib().nq_dnt_basis(P(g["d_d"]), P(dfreq), P(roots), P(norms), E, S, R, O.CUTOFF, O.EXPONENT + 1, P(dt), grad_rbf, P(rbf_t), P(rad_t), P(rows), st()))
        return rbf_t, rad_t, rows
    rbf_t, rad_t, rows = call(Dv(g_rbf))
    rev_ok(f"tangent basis S={S} rbf_t", rbf_t, ref[0]), rev_ok(f"tangent basis S={S} rad_t", rad_t, ref[1])
    rev_ok(f"tangent basis S={S} adjoint of freq", rows.cpu().double().sum(0), ref[2])
    lean = call(None)                                                        # no adjoint of rbf: zero rows, the tangents unchanged
    assert _same(lean[:2], (rbf_t, rad_t)) and float(lean[2].abs().max()) == 0.0


def _triplet_case(w):
    g = O.graph()
    E, I, S, Bs = g["E"], w["I"], w["S"], w["Bs"]
    x, Q, u, W2 = O._triplet_inputs(g, w)
    tx, tQ, tu, gm = rnd(60, E, I), rnd(61, E, S * Bs), rnd(62, E, 3), rnd(63, E, I)
    dev = SimpleNamespace(x=x.to(DEV), Q=Q.to(DEV), W2=W2.to(DEV), tx=tx.to(DEV), tQ=tQ.to(DEV), tu=tu.to(DEV), gm=gm.to(DEV))
    fn = lambda x, Q, u, W2: O._triplet_ref(g, x, Q, u, W2, S, Bs)            # noqa: E731

    def ref(which):
        return FR.second_sweep(fn, (x, Q, u, W2), which, [(tx, tQ, tu)[k] for k in which], gm, (0, 1, 3))
    return g, E, I, S, Bs, dev, ref


SETS = [((0, 1, 2), "all"), ((0,), "tx"), ((1,), "tQ"), ((2,), "tu")]


@pytest.mark.parametrize("w", WIDTHS, ids=lambda w: f"I{w['I']}S{w['S']}")
def test_triplet_tangent_forward(w):
    g, E, I, S, Bs, dev, ref = _triplet_case(w)
    zeros = [torch.zeros_like(t) for t in (dev.tx, dev.tQ, dev.tu)]

    def call(tans):
        def run():
            mt = nan_dev(E, I)
            check(lib().nq_dnt_triplet_forward(P(dev.x), P(dev.Q), P(g["d_u"]), P(dev.W2), P(tans[0]), P(tans[1]), P(tans[2]), P(g["d_row_ptr"]), P(g["d_src"]),
                                               P(g["d_dst"]), E, I, S, Bs, P(mt), st()))
            return (mt,)
        return run
    full = (dev.tx, dev.tQ, dev.tu)
    for which, name in SETS:
        (mt,) = twice(call([full[k] if k in which else None for k in range(3)]))
        fwd_ok(f"tangent triplet I={I} mt ({name})", mt, ref(which)[0])
        (mz,) = call([full[k] if k in which else zeros[k] for k in range(3)])()
        assert _same((mt,), (mz,)), name                                       # NULL == a zero tangent, bit for bit
        assert float(mt.cpu()[torch.from_numpy(g["n_trip"] == 0)].abs().max()) == 0.0            # edges without a triplet


@pytest.mark.parametrize("w", WIDTHS, ids=lambda w: f"I{w['I']}S{w['S']}")
def test_triplet_tangent_backward(w):
    g, E, I, S, Bs, dev, ref = _triplet_case(w)
    zeros = [torch.zeros_like(t) for t in (dev.tx, dev.tQ, dev.tu)]
    scr = torch.empty(int(lib().nq_dn_triplet_scratch_floats(E, I, Bs)) + 64, device=DEV)

    def call(tans, with_w=True):
        def run():
            a_x, a_Q, a_W = nan_dev(E, I), nan_dev(E, S * Bs), nan_dev(I, Bs)
            check(lib().nq_dnt_triplet_backward(P(dev.x), P(dev.Q), P(g["d_u"]), P(dev.W2), P(tans[0]), P(tans[1]), P(tans[2]), P(g["d_row_ptr"]), P(g["d_src"]),
                                                P(g["d_dst"]), P(g["d_src_order"]), P(g["d_src_ptr"]), E, I, S, Bs, P(dev.gm), P(a_x), P(a_Q),
                                                P(a_W) if with_w else None, P(scr) if with_w else None, st()))
            return a_x, a_Q, a_W
        return run
    full = (dev.tx, dev.tQ, dev.tu)
    for which, name in SETS:
        got = twice(call([full[k] if k in which else None for k in range(3)]))
        for label, a, r in zip(("a_x", "a_Q", "a_W_sbf2"), got, ref(which)[1:]):
            rev_ok(f"tangent triplet I={I} {label} ({name})", a, r)
        assert _same(got, call([full[k] if k in which else zeros[k] for k in range(3)])()), name
    both, lean = call(full)(), call(full, with_w=False)()                    # without the weight adjoint: the same adjoints, the weight buffer untouched
    torch.cuda.synchronize()
    assert _same(both[:2], lean[:2]) and torch.isnan(lean[2]).all()


def test_silu_second_order():
    grid = torch.cat([torch.tensor([0.0, 20.0, -20.0, 100.0, -100.0, 1e-3, -1e-3]), torch.linspace(-12, 12, 481), rnd(70, 1500) * 3]).float()
    n = grid.numel()
    g, a = rnd(71, n), rnd(72, n)
    ref_g, ref_pre = FR.silu_reverse2(grid.double(), g.double(), a.double())
    a_g, a_pre = nan_dev(n), nan_dev(n)
    check(lib().nq_dnt_silu(Dv(grid), Dv(g), Dv(a), n, P(a_g), P(a_pre), st()))
    assert bool(torch.isfinite(a_g).all() and torch.isfinite(a_pre).all())
    fwd_ok("silu second order a_g", a_g, ref_g), rev_ok("silu second order a_pre", a_pre, ref_pre)
    assert float(a_pre[3:5].abs().max().cpu()) == 0.0                       # silu''(+-100) = 0, not inf * 0


@pytest.mark.parametrize("H", [128, 96])
def test_gate_second_order_and_embedding_scatter(H):
    g = O.graph()
    E, N = g["E"], g["N"]
    x, gate, gy, a_gx, a_gg = (rnd(80 + k, E, H) for k in range(5))
    x64, gate64, gy64, p64, q64 = (t.double() for t in (x, gate, gy, a_gx, a_gg))
    dx, dgate, dgy, dp, dq = (t.to(DEV) for t in (x, gate, gy, a_gx, a_gg))

    def call(p, q):
        a_g, a_x, a_gate = nan_dev(E, H), nan_dev(E, H), nan_dev(E, H)
        check(lib().nq_dnt_gate(P(dx), P(dgate), P(dgy), P(p), P(q), E * H, P(a_g), P(a_x), P(a_gate), st()))
        return a_g, a_x, a_gate
    a_g, a_x, a_gate = call(dp, dq)
    fwd_ok("gate second order a_g", a_g, p64 * gate64 + q64 * x64)
    rev_ok("gate second order a_x", a_x, q64 * gy64), rev_ok("gate second order a_gate", a_gate, p64 * gy64)
    assert _same(call(dp, None), call(dp, torch.zeros_like(dq))) and _same(call(None, dq), call(torch.zeros_like(dp), dq))
    rows = rnd(86, E, H)
    src, dst = torch.from_numpy(g["src"]), torch.from_numpy(g["dst"])
    ref = torch.cat([torch.zeros(N, H, dtype=torch.float64).index_add_(0, dst, rows.double()), torch.zeros(N, H, dtype=torch.float64).index_add_(0, src, rows.double())], 1)
    out = nan_dev(N, 2 * H)
    check(lib().nq_dnt_embed_scatter(Dv(rows), P(g["d_row_ptr"]), P(g["d_src_order"]), P(g["d_src_ptr"]), N, E, H, P(out), st()))
    rev_ok("embedding scatter", out, ref)
    assert float(out[0].abs().max()) == 0.0                                 # the lone atom


# ---- the wrappers: double backward of every Function against float64 torch ----------------------------------------------------------------------------------------
def _plan(g):
    return SimpleNamespace(N=g["N"], E=g["E"], pos=g["pos"].to(DEV), d=g["d_d"], u=g["d_u"], row_ptr=g["d_row_ptr"], src=g["d_src"], dst=g["d_dst"],
                           src_order=g["d_src_order"], src_ptr=g["d_src_ptr"])


def _wrapper(name, fn_dev, fn_ref, inputs, tangent_of, tangents, gs, adjoint_of):
    """The device Function (float32) by torch.autograd's double backward against the same double backward of the float64 restatement."""
    ref = FR.second_sweep(fn_ref, inputs, tangent_of, tangents, gs, adjoint_of)
    ins = [t.to(DEV).requires_grad_(True) for t in inputs]
    ws = [t.to(DEV).requires_grad_(True) for t in (gs if isinstance(gs, (tuple, list)) else (gs,))]
    out = fn_dev(*ins)
    outs = out if isinstance(out, (tuple, list)) else (out,)
    first = torch.autograd.grad(sum((o * v).sum() for o, v in zip(outs, ws)), [ins[k] for k in tangent_of], create_graph=True)
    assert all(f.grad_fn is not None for f in first), name
    res = torch.autograd.grad(first, ws + [ins[k] for k in adjoint_of], grad_outputs=[t.to(DEV) for t in tangents], allow_unused=True)
    for k, (a, r) in enumerate(zip(res, ref)):
        a = torch.zeros(r.shape) if a is None else a
        (fwd_ok if k < len(ws) else rev_ok)(f"wrapper {name} [{k}]", a, r)


@pytest.mark.parametrize("bias,silu", [(True, True), (True, False), (False, True), (False, False)])
def test_linear_wrapper_double_backward(bias, silu):
    from nabladft_amd.dense import linear2 as _linear
    E = O.graph()["E"]
    x, W, b, gy, a_gx = rnd(90, E, 6), rnd(91, 8, 6), rnd(92, 8), rnd(93, E, 8), rnd(94, E, 6)
    act = FR.silu if silu else (lambda z: z)
    if bias:
        _wrapper(f"linear bias silu={silu}", lambda x, W, b: _linear(x, W, b, silu), lambda x, W, b: act(x @ W.t() + b), (x, W, b), (0,), (a_gx,), gy, (0, 1, 2))
    else:
        _wrapper(f"linear silu={silu}", lambda x, W: _linear(x, W, None, silu), lambda x, W: act(x @ W.t()), (x, W), (0,), (a_gx,), gy, (0, 1))


@pytest.mark.parametrize("H", [128, 96])
def test_gate_gated_sum_and_embedding_wrappers_double_backward(H):
    from nabladft_amd.dimenetplusplus import _EmbedFn, _GateFn, _GateSumFn
    g = O.graph()
    E, N = g["E"], g["N"]
    plan = _plan(g)
    src, dst = torch.from_numpy(g["src"]), torch.from_numpy(g["dst"])
    x, gate, gy, a_gx, a_gg, go = rnd(100, E, H), rnd(101, E, H), rnd(102, E, H), rnd(103, E, H), rnd(104, E, H), rnd(105, N, H)
    _wrapper("gate", _GateFn.apply, lambda x, gate: x * gate, (x, gate), (0, 1), (a_gx, a_gg), gy, (0, 1))
    _wrapper("gated sum", lambda x, gate: _GateSumFn.apply(x, gate, plan), lambda x, gate: torch.zeros(N, H, dtype=torch.float64).index_add_(0, dst, x * gate),
             (x, gate), (0, 1), (a_gx, a_gg), go, (0, 1))
    AB, Cr, bias = rnd(106, N, 2 * H), rnd(107, E, H), rnd(108, H)
    _wrapper("embedding", lambda AB, Cr, bias: _EmbedFn.apply(AB, Cr, bias, plan)[0], lambda AB, Cr, bias: FR.silu(AB[dst, :H] + AB[src, H:] + Cr + bias),
             (AB, Cr, bias), (1,), (a_gx,), gy, (0, 1, 2))


def test_geometry_basis_triplet_and_molecule_sum_wrappers_double_backward():
    from nabladft_amd.dimenetplusplus import _BasisFn, _GeomFn, _TripletFn
    from nabladft_amd.gemnet_oc import _SegSumFn
    g = O.graph()
    E, N = g["E"], g["N"]
    plan = _plan(g)
    src, dst = torch.from_numpy(g["src"]), torch.from_numpy(g["dst"])
    _wrapper("geometry", lambda pos: _GeomFn.apply(pos, plan), lambda pos: FR.geometry(pos, src, dst), (g["pos"],), (0,), (rnd(110, N, 3),), (rnd(111, E), rnd(112, E, 3)), ())
    w = O.WIDTHS[0]
    I, S, R, Bs = w["I"], w["S"], w["R"], w["Bs"]
    table = D.bessel_table(S, R)
    roots, norms = (torch.from_numpy(a).to(DEV).contiguous() for a in table)
    freq = (torch.arange(1, R + 1) * torch.pi + 0.1 * rnd(3, R)).float()
    _wrapper("basis", lambda d, f: _BasisFn.apply(d, f, roots, norms, S, R, O.CUTOFF, O.EXPONENT + 1),
             lambda d, f: D.radial_bases(d, f, O.CUTOFF, O.EXPONENT, S, R, table, stable=True), (g["d"], freq), (0,), (rnd(113, E),), (rnd(114, E, R), rnd(115, E, S * R)), (1,))
    x, Q, u, W2 = O._triplet_inputs(g, w)
    _wrapper("triplet", lambda x, Q, u, W2: _TripletFn.apply(x, Q, u, W2, plan, S), lambda x, Q, u, W2: O._triplet_ref(g, x, Q, u, W2, S, Bs), (x, Q, u, W2), (0, 1, 2),
             (rnd(116, E, I), rnd(117, E, S * Bs), rnd(118, E, 3)), rnd(119, E, I), (0, 1, 3))
    sizes = np.array([1, 2, 3, 9, 24])
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    owner = torch.tensor(np.repeat(np.arange(5), sizes), dtype=torch.int32, device=DEV)
    own64 = owner.cpu().long()
    _wrapper("molecule sum", lambda rows, s: _SegSumFn.apply(rows * s, ptr, owner, 5), lambda rows, s: torch.zeros(5, 50, dtype=torch.float64).index_add_(0, own64, rows * s),
             (rnd(120, N, 50), rnd(121, N, 50)), (0,), (rnd(122, N, 50),), rnd(123, 5, 50), (1,))


def test_triplet_double_backward_allocates_nothing_of_the_size_of_the_triplets():
    from nabladft_amd.dimenetplusplus import _TripletFn
    g = O.graph(sizes=(45, 45, 45), seed=7, K_=32)
    assert g["T"] >= 100000
    E, I, S, Bs = g["E"], 64, 7, 8
    plan = _plan(g)
    x, Q, W2, gm = (t.to(DEV).requires_grad_(True) for t in (rnd(20, E, I), rnd(21, E, S * Bs), rnd(22, I, Bs), rnd(23, E, I)))
    u = g["d_u"].clone().requires_grad_(True)
    tans = [t.to(DEV) for t in (rnd(24, E, I), rnd(25, E, S * Bs), rnd(26, E, 3))]

    def sweep():
        m = _TripletFn.apply(x, Q, u, W2, plan, S)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        first = torch.autograd.grad(m, (x, Q, u), grad_outputs=gm, create_graph=True)
        second = torch.autograd.grad(first, (gm, x, Q, W2), grad_outputs=tans)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base - sum(t.numel() * 4 for t in first + second), second
    sweep()                                                                   # loads the code objects, which is not what is measured
    extra, second = sweep()
    O._record(f"ops triplet double backward at T = {g['T']}: peak device memory beyond its outputs {extra} bytes (< 1 MiB; a [T, 64] array would be {g['T'] * 256})")
    assert extra < 1 << 20
    assert all(bool(torch.isfinite(t).all()) for t in second)
