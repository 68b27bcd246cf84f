"""nabladft_amd.DimeNetPlusPlusForceLightning on the GPU: the training step with a loss on the forces against the recorded float64 run of the real reference
wrapper (tests/golden/dimenet_force_*.npz, scripts/make_golden_dimenet_force.py), L1 losses with the coefficient pairs (energy, forces) = (1, 1) and (0, 1).

Bound of the loss and of every parameter gradient (norm, projection on tests/dimenet_ref.probe_direction, and the whole tensor where it is recorded), the rule of
tests/test_dimenet_gpu.py: max(4 x own32x, 2e-6), own32x = the error of the reference's float32 run with the bases evaluated in float64, in the same measure
(|g - g64| / |g64|; the loss relative to itself).  The closest ratio per quantity goes to the suite's parity report (kept as profiles/dimenet_parity.txt)."""
import numpy as np
import pytest
import torch

from tests import dimenet_force_ref as FR
from tests import dimenet_ref as D
from tests import test_dimenet_gpu as M
from tests.helpers import DEV, bits

pytestmark = pytest.mark.gpu

CASES = {"dimenet_small": "dimenet_force_small", "dimenet_yaml": "dimenet_force_yaml"}
_NETS = {}


def _task(name, pair, **kw):
    """(force fixture, task in training mode around a net of its own with the fixture's weights, batch)."""
    import nabladft_amd as nq
    fx, ref_net, b = M.setup(name)
    if name not in _NETS:
        net = nq.DimeNetPlusPlusPotential(**M.CASES[name][0])
        net.load_state_dict(ref_net.state_dict())
        _NETS[name] = (dict(np.load(M.os.path.join(M.GOLDEN, CASES[name] + ".npz"), allow_pickle=False)), net.to(DEV))
    ffx, net = _NETS[name]
    task = nq.DimeNetPlusPlusForceLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=pair[0], forces_loss_coef=pair[1], **kw)
    return ffx, task.train(), b


def _grads(task, b):
    task.net.zero_grad(set_to_none=True)
    loss = task.training_step(b, 0)
    loss.backward()
    return loss.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in task.net.named_parameters()}


@pytest.mark.parametrize("pair", FR.PAIRS, ids=FR.tag)
@pytest.mark.parametrize("name", list(CASES))
def test_force_loss_gradients_match_the_reference(name, pair):
    fx, task, b = _task(name, pair)
    t = FR.tag(pair)
    worst = {}

    def cmp(q, key, err, own):
        bound = max(4 * own, 2e-6)
        print(f"{name} {t} {q:10s} {key:50s} err {err:.3e} own32x {own:.3e} bound {bound:.3e}")
        if q not in worst or err / bound > worst[q][0] / worst[q][2]:
            worst[q] = (err, own, bound)
        assert err <= bound, (name, t, q, key, err, own, bound)

    loss, grads = _grads(task, b)
    ref = float(fx["loss:" + t])
    cmp("loss", "", abs(float(loss) - ref) / abs(ref), float(fx["own32x:loss:" + t]))
    for k, g in grads.items():
        nrm, own = float(fx[f"gnorm:{t}:{k}"]), float(fx[f"own32x:{t}:{k}"])
        if nrm == 0.0:                                                       # exactly zero in float64: no gradient, or zeros
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        assert g is not None and bool(torch.isfinite(g).all()), k
        g64 = g.cpu().double()
        if f"grad:{t}:{k}" in fx:
            cmp("grad", k, float(np.linalg.norm(g64.numpy() - fx[f"grad:{t}:{k}"])) / nrm, own)
        cmp("grad norm", k, abs(float(g64.norm()) - nrm) / nrm, own)
        cmp("grad probe", k, abs(float((g64 * D.probe_direction(k, tuple(g.shape))).sum()) - float(fx[f"gprobe:{t}:{k}"])) / nrm, own)
    for q, (err, own, bound) in worst.items():
        M._record(f"force loss {name:14s} {t} {q:11s} err {err:.2e}  own32_exact_basis {own:.2e}  bound {bound:.2e}  ratio {err / bound:.2f}")


def test_forces_with_the_graph_are_the_default_forces_and_gradients_are_reproducible():
    fx, task, b = _task("dimenet_small", (1.0, 1.0))
    net = task.net
    E0, F0 = net(b)
    E1, F1 = net(b, create_graph=True)
    assert F0.grad_fn is None and not F0.requires_grad and F1.grad_fn is not None
    assert torch.equal(bits(F0), bits(F1)) and torch.equal(bits(E0), bits(E1))
    E2, F2 = task(b)                                                         # the task in training mode asks for the graph
    assert F2.grad_fn is not None and torch.equal(bits(F2), bits(F0))
    with torch.no_grad():
        assert net(b, create_graph=True)[1].grad_fn is None
    l1, g1 = _grads(task, b)
    l2, g2 = _grads(task, b)
    assert torch.equal(bits(l1), bits(l2)) and all(torch.equal(bits(g1[k]), bits(g2[k])) for k in g1)
    energy_only, ref = M.energy_loss_grads(net, b)[1], M.energy_loss_grads(M.setup("dimenet_small")[1], b)[1]      # the first-order path next to it
    assert all(torch.equal(bits(energy_only[k]), bits(ref[k])) for k in ref)


def test_validation_in_eval_mode_returns_forces_without_a_graph():
    fx, task, b = _task("dimenet_small", (1.0, 1.0))
    task.eval()
    try:
        E, F = task(b)
        assert F.grad_fn is None and not F.requires_grad
        assert float(task.validation_step(b, 0).detach()) > 0 and float(task.test_step(b, 0).detach()) > 0 and len(task.predict_step(b)) == 2
    finally:
        task.train()


def test_force_loss_training_lowers_the_loss():
    import nabladft_amd as nq
    fx, ref_net, b = M.setup("dimenet_small")
    net = nq.DimeNetPlusPlusPotential(**M.CASES["dimenet_small"][0])
    net.load_state_dict(ref_net.state_dict())
    net = net.to(DEV).train()
    task = nq.DimeNetPlusPlusForceLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=0.0, forces_loss_coef=1.0,
                                            optimizer=lambda p: torch.optim.Adam(p, lr=1e-4))
    opt = task.configure_optimizers()["optimizer"]
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = task.training_step(b, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    losses.append(float(task.step(b).detach()))
    print("force loss over five Adam steps", losses)
    assert all(np.isfinite(losses)) and losses[-1] < 0.8 * losses[0], losses
