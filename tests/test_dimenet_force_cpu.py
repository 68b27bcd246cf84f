"""CPU: the force-loss task of DimeNet++ (nabladft_amd.DimeNetPlusPlusForceLightning) as far as it goes without a device, the recorded force-loss training step
of the real reference wrapper (tests/golden/dimenet_force_*.npz, scripts/make_golden_dimenet_force.py) against the float64 restatement, and the formulas the
second-sweep kernels of csrc/dimenet.hip implement (tests/dimenet_force_ref.py) against torch.autograd's own double backward of the restated operations, in
float64 at 1e-10: this pins the formulas before any kernel runs."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import dimenet_force_ref as FR
from tests import dimenet_ref as D
from tests.test_dimenet_ops_gpu import _triplet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fx(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(name, got, ref, tol=1e-10):
    err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
    assert err <= tol, (name, err)


@pytest.fixture(scope="module")
def graph():
    b = D.make_batch((1, 2, 3, 9), 1)
    src, dst = D.radius_graph(b["pos"].numpy(), b["batch"].numpy(), 5.0, 4)
    kj, ji, _, _, _ = D.triplets(src, dst, len(b["pos"]))
    assert len(kj) > 50 and (np.bincount(ji, minlength=len(src)) == 0).any()
    d, u = FR.geometry(b["pos"], torch.from_numpy(src), torch.from_numpy(dst))
    return dict(pos=b["pos"], src=torch.from_numpy(src), dst=torch.from_numpy(dst), kj=torch.from_numpy(kj), ji=torch.from_numpy(ji), E=len(src), N=len(b["pos"]),
                d=d, u=u)


def test_the_force_task_has_the_surface_of_the_reference_class_and_does_not_refuse():
    import nabladft_amd as nq
    assert "DimeNetPlusPlusForceLightning" in nq.__all__ and issubclass(nq.DimeNetPlusPlusForceLightning, nq.DimeNetPlusPlusLightning)
    fx = _fx("dimenet_force_small")
    assert list(inspect.signature(nq.DimeNetPlusPlusForceLightning.__init__).parameters)[1:] == [str(k) for k in fx["lightning_kwargs"]]
    net = nq.DimeNetPlusPlusPotential(**D.SMALL)
    kw = dict(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=1.0)
    task = nq.DimeNetPlusPlusForceLightning(**kw)
    assert list(task.state_dict().keys()) == [str(k) for k in fx["keys"]] == list(nq.DimeNetPlusPlusLightning(**kw).state_dict().keys())
    assert list(inspect.signature(net.forward).parameters) == ["data", "return_intermediates", "create_graph"]
    assert inspect.signature(net.forward).parameters["create_graph"].default is False
    for name in ("validation_step", "test_step", "predict_step", "step", "configure_optimizers"):
        assert getattr(nq.DimeNetPlusPlusForceLightning, name) is getattr(nq.DimeNetPlusPlusLightning, name)
    batch = nq.Batch(torch.zeros(3, 3), torch.tensor([1, 6, 8]), torch.zeros(3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="MI355X only"):             # passes into the model (which has no CPU path) with a force loss
        task.train().training_step(batch, 0)
    with pytest.raises(NotImplementedError, match="second-order.*DimeNetPlusPlusForceLightning"):
        nq.DimeNetPlusPlusLightning(**kw).training_step(batch, 0)


@pytest.mark.parametrize("pair", FR.PAIRS, ids=FR.tag)
def test_force_loss_fixture_reproduces_from_the_restatement(pair):
    fx, t = _fx("dimenet_force_small"), FR.tag(pair)
    b = D.make_batch(D.SMALL_SIZES, int(fx["seed"]) + 1)
    loss, grads, _, _ = FR.force_loss(D.SMALL, D.make_params(D.SMALL, int(fx["seed"])), b, pair)
    assert abs(float(loss) - float(fx["loss:" + t])) <= 1e-9 * abs(float(fx["loss:" + t]))
    for k, g in grads.items():
        nrm = float(fx[f"gnorm:{t}:{k}"])
        assert (nrm > 0) == (not (pair == (0.0, 1.0) and k == "regr_or_cls_nn.6.bias")), k
        assert abs(float((g * D.probe_direction(k, tuple(g.shape))).sum()) - float(fx[f"gprobe:{t}:{k}"])) <= 1e-9 * max(nrm, 1e-300), k
        assert abs(float(g.norm()) - nrm) <= 1e-9 * nrm, k
    for name in ("dimenet_force_small", "dimenet_force_yaml"):
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20


def test_triplet_tangent_formulas(graph):
    g_ = graph
    E, I, S, Bs = g_["E"], 8, 5, 3
    x, Q, W2, tx, tQ, tu, g = _rnd(1, E, I), _rnd(2, E, S * Bs), _rnd(3, I, Bs), _rnd(4, E, I), _rnd(5, E, S * Bs), _rnd(6, E, 3), _rnd(7, E, I)
    fn = lambda x, Q, u, W2: _triplet_ref(g_, x, Q, u, W2, S, Bs)            # noqa: E731  (the restatement the GPU tests use)
    ref = FR.second_sweep(fn, (x, Q, g_["u"], W2), (0, 1, 2), (tx, tQ, tu), g, (0, 1, 3))
    got = FR.triplet_tangent(g_["kj"], g_["ji"], E, x, Q, g_["u"], W2, tx, tQ, tu, g, S, Bs)
    for name, a, r in zip(("mt", "a_x", "a_Q", "a_W2"), got, ref):
        _close("triplet " + name, a, r)
    zero = torch.zeros_like
    for k, only in enumerate(((tx, zero(tQ), zero(tu)), (zero(tx), tQ, zero(tu)), (zero(tx), zero(tQ), tu))):       # each tangent alone
        ref = FR.second_sweep(fn, (x, Q, g_["u"], W2), (k,), (only[k],), g, (0, 1, 3))
        for name, a, r in zip(("mt", "a_x", "a_Q", "a_W2"), FR.triplet_tangent(g_["kj"], g_["ji"], E, x, Q, g_["u"], W2, *only, g, S, Bs), ref):
            _close(f"triplet tangent {k} alone {name}", a, r)


def test_geometry_and_basis_tangent_formulas(graph):
    g_ = graph
    E, N, S, R = g_["E"], g_["N"], 5, 4
    tpos, gd, gu = _rnd(10, N, 3), _rnd(11, E), _rnd(12, E, 3)
    ref = FR.second_sweep(lambda pos: FR.geometry(pos, g_["src"], g_["dst"]), (g_["pos"],), (0,), (tpos,), (gd, gu), ())
    td, tu = FR.geometry_tangent(g_["d"], g_["u"], tpos, g_["src"], g_["dst"])
    _close("geometry td", td, ref[0]), _close("geometry tu", tu, ref[1])
    table = D.bessel_table(S, R)
    freq = torch.arange(1, R + 1, dtype=torch.float64) * torch.pi + 0.1 * _rnd(13, R)
    t, g_rbf, g_rad = _rnd(14, E), _rnd(15, E, R), _rnd(16, E, S * R)
    ref = FR.second_sweep(lambda d, f: D.radial_bases(d, f, 5.0, 5, S, R, table, stable=True), (g_["d"], freq), (0,), (t,), (g_rbf, g_rad), (1,))
    rbf_t, rad_t, a_freq = FR.basis_tangent(g_["d"], freq, t, g_rbf, 5.0, 5, S, R, table)
    _close("basis rbf_t", rbf_t, ref[0]), _close("basis rad_t", rad_t, ref[1]), _close("basis a_freq", a_freq, ref[2])


def test_silu_gate_and_linear_second_order_formulas(graph):
    g_ = graph
    E, N, H = g_["E"], g_["N"], 6
    pre = torch.cat([_rnd(20, 50) * 3, torch.tensor([0.0, 20.0, -20.0, 100.0, -100.0], dtype=torch.float64)])
    g, a = _rnd(21, pre.numel()), _rnd(22, pre.numel())
    ref = FR.second_sweep(FR.silu, (pre,), (0,), (a,), g, (0,))
    a_g, a_pre = FR.silu_reverse2(pre, g, a)
    assert bool(torch.isfinite(a_g).all() and torch.isfinite(a_pre).all())
    _close("silu a_g", a_g, ref[0]), _close("silu a_pre", a_pre, ref[1])
    x, gate, gy, a_gx, a_gg = (_rnd(30 + k, E, H) for k in range(5))
    ref = FR.second_sweep(lambda x, gate: x * gate, (x, gate), (0, 1), (a_gx, a_gg), gy, (0, 1))
    _close("gate a_g", a_gx * gate + a_gg * x, ref[0]), _close("gate a_x", a_gg * gy, ref[1]), _close("gate a_gate", a_gx * gy, ref[2])
    dst, go = g_["dst"], _rnd(36, N, H)
    gsum = lambda p, q: torch.zeros(N, H, dtype=torch.float64).index_add_(0, dst, p * q)            # noqa: E731
    ref = FR.second_sweep(gsum, (x, gate), (0, 1), (a_gx, a_gg), go, (0, 1))
    _close("gated sum a_g", gsum(a_gx, gate) + gsum(a_gg, x), ref[0]), _close("gated sum a_x", go[dst] * a_gg, ref[1]), _close("gated sum a_gate", go[dst] * a_gx, ref[2])
    xin, W, bias, gy, a_gx = _rnd(40, E, 6), _rnd(41, 8, 6), _rnd(42, 8), _rnd(43, E, 8), _rnd(44, E, 6)
    ref = FR.second_sweep(lambda x, W, b: FR.silu(x @ W.t() + b), (xin, W, bias), (0,), (a_gx,), gy, (0, 1, 2))
    z = xin @ W.t() + bias
    a_gp = a_gx @ W.t()                                    # what the forward launcher computes from (a_gx [M, K], W [N, K])
    a_g, a_pre = FR.silu_reverse2(z, gy, a_gp)
    gp = gy * torch.autograd.functional.jvp(FR.silu, z, torch.ones_like(z))[1]
    _close("linear a_g", a_g, ref[0]), _close("linear a_x", a_pre @ W, ref[1]), _close("linear a_W", gp.t() @ a_gx + a_pre.t() @ xin, ref[2])
    _close("linear a_b", a_pre.sum(0), ref[3])
