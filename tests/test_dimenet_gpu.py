"""nabladft_amd.DimeNetPlusPlusPotential / DimeNetPlusPlusLightning on the GPU against the recorded float64 run of the real reference wrapper
(tests/golden/dimenet_*.npz, scripts/make_golden_dimenet.py; the torch-geometric core behind the wrapper is restated, unpinned).

Bound of every compared quantity: max(4 x own32x, 2e-6), own32x = the error of the reference's float32 run with the bases evaluated in float64 and rounded
once, in the same measure (arrays: max |a - b| / max |b|; gradient tensors: |g - g64| / |g64|).  The closest ratio per quantity goes to
the suite's parity report (tests/helpers.py; these lines are kept as profiles/dimenet_parity.txt)."""
import os

import numpy as np
import pytest
import torch

from tests import dimenet_ref as D
from tests.helpers import DEV, _report, bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {"dimenet_small": (D.SMALL, D.SMALL_SIZES), "dimenet_yaml": (D.YAML, D.YAML_SIZES)}
_CACHE = {}


def _record(line):
    _report(line)                     # the suite's parity report (tests/helpers.py); a copy of these lines is kept as profiles/dimenet_parity.txt
    print(line)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _np(t):
    return t.detach().cpu().double().numpy()


def setup(name, **kw):
    """(fixture, net on the device with the fixture's weights, batch on the device); built once per configuration."""
    import nabladft_amd as nq
    key = (name, repr(sorted(kw.items())))
    if key not in _CACHE:
        cfg, sizes = CASES[name]
        fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        net = nq.DimeNetPlusPlusPotential(**cfg, **kw)
        net.load_state_dict({k: v.float() for k, v in D.make_params(cfg, int(fx["seed"])).items()})           # key for key, strict
        net = net.to(DEV).eval()
        b = nq.Batch(torch.from_numpy(fx["pos"]).float(), torch.from_numpy(fx["z"]), torch.from_numpy(fx["batch"]), y=torch.from_numpy(fx["y"]).float(),
                     forces=torch.from_numpy(fx["forces_target"]).float()).to(DEV)
        _CACHE[key] = (fx, net, b)
    return _CACHE[key]


def energy_loss_grads(net, b):
    import nabladft_amd as nq
    task = nq.DimeNetPlusPlusLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=0.0)
    net.zero_grad(set_to_none=True)
    loss = task.step(b)
    loss.backward()
    return loss.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("name", list(CASES))
def test_model_matches_the_reference(name):
    fx, net, b = setup(name)
    worst = {}

    def cmp(q, err, own):
        bound = max(4 * own, 2e-6)
        if q not in worst or err / bound > worst[q][0] / worst[q][2]:
            worst[q] = (err, own, bound)
        assert err <= bound, (name, q, err, own, bound)

    E, F, rec = net(b, return_intermediates=True)
    plan = net.last_plan
    assert np.array_equal(plan.src.cpu().numpy(), fx["src"]) and np.array_equal(plan.dst.cpu().numpy(), fx["dst"])         # the same graph, the same edge order
    assert not F.requires_grad and F.grad_fn is None
    rows = fx["rows"]
    cmp("rbf", _rel(_np(rec["rbf"])[rows], fx["rbf"]), float(fx["own32x:rbf"]))
    cmp("rad", _rel(_np(rec["rad"])[rows], fx["rad"]), float(fx["own32x:rad"]))
    for k, x in enumerate(rec["block_out"]):
        cmp("block_out", _rel(_np(x)[rows], fx["block_out"][k]), float(fx["own32x:block_out"][k]))
    cmp("P", _rel(_np(rec["P"]), fx["P"]), float(fx["own32x:P"]))
    cmp("energy", _rel(_np(E), fx["energy"]), float(fx["own32x:energy"]))
    cmp("forces", _rel(_np(F), fx["forces"]), float(fx["own32x:forces"]))
    loss, grads = energy_loss_grads(net, b)
    assert abs(float(loss) - float(fx["loss"])) <= max(4 * float(fx["own32x:energy"]), 2e-6) * max(abs(float(fx["loss"])), float(np.abs(fx["energy"]).max()))
    for k, g in grads.items():
        nrm, own = float(fx["gnorm:" + k]), float(fx["own32x:grad:" + k])
        g64 = g.cpu().double()
        if "grad:" + k in fx:
            cmp("grad", float(np.linalg.norm(g64.numpy() - fx["grad:" + k])) / nrm, own)
        cmp("grad norm", abs(float(g64.norm()) - nrm) / nrm, own)
        cmp("grad probe", abs(float((g64 * D.probe_direction(k, tuple(g.shape))).sum()) - float(fx["gprobe:" + k])) / nrm, own)
    for q, (err, own, bound) in worst.items():
        _record(f"model {name:14s} {q:11s} err {err:.2e}  own32_exact_basis {own:.2e}  bound {bound:.2e}  ratio {err / bound:.2f}")
    with open("/proc/self/maps") as f:
        assert "libnablaq.so" in f.read()


def test_bitwise_reproducible_and_post_processing_rescales_the_energy_only():
    fx, net, b = setup("dimenet_small")
    E1, F1 = net(b)
    _, g1 = energy_loss_grads(net, b)
    E2, F2 = net(b)
    _, g2 = energy_loss_grads(net, b)
    assert torch.equal(bits(E1), bits(E2)) and torch.equal(bits(F1), bits(F2))
    assert all(torch.equal(bits(g1[k]), bits(g2[k])) for k in g1)
    _, post, _ = setup("dimenet_small", scaler=D.SCALER, do_postprocessing=True)
    Ep, Fp = post(b)
    assert torch.equal(bits(Fp), bits(F1))
    assert _rel(_np(Ep), D.SCALER["scale_"] * _np(E1) + D.SCALER["mean_"]) < 1e-6
    assert _rel(_np(Ep), fx["energy_post"]) <= max(4 * float(fx["own32x:energy_post"]), 2e-6)
    with torch.no_grad():                                                   # the calculator's context: forces all the same, nothing kept
        E3, F3 = net(b)
    assert torch.equal(bits(E3), bits(E1)) and torch.equal(bits(F3), bits(F1)) and not E3.requires_grad


def test_each_molecule_alone_equals_the_molecule_in_the_batch():
    import nabladft_amd as nq
    fx, net, b = setup("dimenet_small")
    E, F = net(b)
    off = 0
    for m, n in enumerate(D.SMALL_SIZES):
        one = nq.Batch(b.pos[off:off + n].clone(), b.z[off:off + n].clone(), torch.zeros(n, dtype=torch.long, device=DEV))
        e, f = net(one)
        assert abs(float(e[0].detach()) - float(E[m].detach())) <= 1e-6 * max(1.0, float(E.detach().abs().max())), n
        assert float((f - F[off:off + n]).abs().max()) <= 1e-6 * max(1.0, float(F.abs().max())), n
        off += n
    assert float(F[0].abs().max()) == 0.0                                   # the lone atom feels nothing


def test_rotation_and_permutation():
    import nabladft_amd as nq
    fx, net, b = setup("dimenet_small")
    E, F = net(b)
    rng = np.random.default_rng(3)
    Rm = torch.from_numpy(np.linalg.qr(rng.normal(size=(3, 3)))[0]).float().to(DEV)
    perm, off = [], 0
    for n in D.SMALL_SIZES:                                                 # inside each molecule; K = 8 keeps the FIRST neighbours in index order, so only
        perm.append(off + (np.arange(n) if n > 9 else rng.permutation(n)))    # molecules the cap does not bite (<= 9 atoms) are permuted
        off += n
    perm = torch.from_numpy(np.concatenate(perm)).to(DEV)
    b2 = nq.Batch((b.pos @ Rm.t())[perm].contiguous(), b.z[perm].contiguous(), b.batch.clone())
    E2, F2 = net(b2)
    assert _rel(_np(E2), _np(E)) <= 2e-5
    assert _rel(_np(F2), _np((F @ Rm.t())[perm])) <= 2e-5


def test_prepared_batches_and_stale_geometry():
    import nabladft_amd as nq
    fx, net, b = setup("dimenet_small")
    E, F = net(b)
    b2 = nq.Batch(b.pos.clone(), b.z, b.batch)
    b2.prepared = net.net.prepare(b2)
    E2, F2 = net(b2)
    assert torch.equal(bits(E2), bits(E)) and torch.equal(bits(F2), bits(F))
    b2.pos.add_(0.01)
    with pytest.raises(ValueError, match="another geometry"):
        net(b2)


def test_energy_loss_training_lowers_the_loss_and_force_loss_is_refused():
    import nabladft_amd as nq
    cfg, sizes = CASES["dimenet_small"]
    fx, ref_net, b = setup("dimenet_small")
    net = nq.DimeNetPlusPlusPotential(**cfg)
    net.load_state_dict(ref_net.state_dict())
    net = net.to(DEV).train()
    task = nq.DimeNetPlusPlusLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=0.0,
                                       optimizer=lambda p: torch.optim.Adam(p, lr=1e-3))
    opt = task.configure_optimizers()["optimizer"]
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = task.training_step(b, 0)
        loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        opt.step()
        losses.append(float(loss))
    assert float(task.step(b)) < losses[0], losses
    refuse = nq.DimeNetPlusPlusLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=1.0)
    with pytest.raises(NotImplementedError, match="second-order"):
        refuse.training_step(b, 0)
    assert float(refuse.validation_step(b, 0)) > 0 and float(refuse.test_step(b, 0)) > 0 and len(refuse.predict_step(b)) == 2


def test_lbfgs_with_the_batchwise_calculator_lowers_the_largest_force():
    import nabladft_amd as nq
    from nabladft_amd.optimization import ASEBatchwiseLBFGS, PyGBatchwiseCalculator
    fx, net, _ = setup("dimenet_small")
    mb = D.make_batch((5, 7, 9, 6), 11)
    calc = PyGBatchwiseCalculator(net, DEV, energy_unit="Hartree", position_unit="Ang")
    opt = ASEBatchwiseLBFGS(calc, logfile=None, maxstep=0.05)
    fmaxes = []
    inner = calc.calculate

    def calculate(batch):
        inner(batch)
        fmaxes.append(float(calc.forces.double().norm(dim=-1).max()))

    calc.calculate = calculate
    opt.run(nq.Batch(mb["pos"].float(), mb["z"], mb["batch"]).to(DEV), fmax=1e-4, steps=10)
    assert opt.nsteps == 10 and len(fmaxes) == 11
    print("largest force", fmaxes[0], "->", fmaxes[-1])
    assert fmaxes[-1] < fmaxes[0]
