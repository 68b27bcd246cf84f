"""Passes the two reverse sweeps of the PaiNN step no longer make (csrc/node.hip, csrc/gemm*.h, csrc/engine.hip).

Top layer (plan_step's `top_layer`, NQ_NO_TOPLAYER=1 switches it off): the energy is read from x alone, so the adjoint of vec_upd entering layer L-1 and its
tangent-adjoint twin are zero arrays.  The TOP flavours of k_upd_rev1 / k_upd_rev2 neither read them nor the rows they multiply, the U input-gradient product of
that layer stores instead of adding to the zeros and its V2 input-gradient product contracts 2F of the 3F columns of G_Y.  Only exact zeros are dropped and what is
left rounds as the general expressions do, so energies, forces and gradients are value-equal (torch.equal) to the general code's.

Side stream rule: above 16 384 atoms the weight-gradient products run beside the chain unless the launch profiler records; results must not depend on it.

Fixtures: hidden_channels 64 and 128, num_rbf 20, L = 2 and L = 1 (the top layer is also layer 0); 86 atoms in molecules of 1, 2, 9, 30 and 44 atoms (a partial
128-row tile) and a second batch of 130 atoms (one row tile plus two rows)."""
import numpy as np
import pytest
import torch

from oracle import painn_ref as R
from tests.helpers import load_case
from tests.test_engine_gpu import _batch, _dev, _kernel_names_of, _model

pytestmark = pytest.mark.gpu

SIZES_86 = [1, 2, 9, 30, 44]
SIZES_130 = [44, 30, 9, 2, 1, 44]
SWITCHES = ("NQ_NO_FUSED_FILTER", "NQ_NO_MOLGW", "NQ_MOLGW", "NQ_MOLGW_CAP", "NQ_NO_LITE", "NQ_NO_LAYER0", "NQ_NO_FUSED_UPDATE", "NQ_NO_TOPLAYER",
            "NQ_SIDE_STREAM")


def _clear(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _synthetic(seed, sizes, spread=1.7):
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.concatenate([rng.uniform(0, (n ** (1 / 3)) * spread + 1.0, size=(n, 3)) for n in sizes]).astype(np.float32)
    bt = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)]).astype(np.int64)
    z = rng.choice([1, 6, 7, 8], size=len(pos)).astype(np.int64)
    y = rng.normal(size=len(sizes)).astype(np.float32)
    ft = rng.normal(0, 0.05, size=pos.shape).astype(np.float32)
    return torch.tensor(pos), torch.tensor(z), torch.tensor(bt), torch.tensor(y), torch.tensor(ft)


def _step(model, batch):
    """One training step as PaiNNLightning does it: loss, energies, forces and the flat gradient."""
    from nabladft_amd import L2Loss
    for p in model.parameters():
        p.grad = None
    model.train()
    energy, forces = model(batch)
    loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
    loss.backward()
    out = {"loss": loss.detach().clone(), "energy": energy.detach().clone(), "forces": forces.detach().clone(),
           "grad": torch.cat([p.grad.reshape(-1) for _, p in model.named_parameters()])}
    torch.cuda.synchronize()
    return out


def _fixture(F, L, sizes):
    import nabladft_amd as nq
    dev = _dev()
    cfg = R.PaiNNConfig(hidden_channels=F, num_layers=L, num_rbf=20)
    model = _model(cfg, R.make_params(cfg, seed=F + L), dev)
    batch = nq.Batch(*_synthetic(F + len(sizes), sizes)).to(dev)
    assert batch.num_nodes == sum(sizes)
    return model, batch


def _assert_equal(a, b, what):
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), (what, k)
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))
    assert float(a["grad"].abs().max()) > 0


FIXTURES = [(F, L, sizes) for F in (64, 128) for L in (2, 1) for sizes in (SIZES_86, SIZES_130)]
IDS = [f"F{F}-L{L}-{sum(s)}atoms" for F, L, s in FIXTURES]


# ---- top layer ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [1 | 32, 1 | 64], ids=["exact-f32", "split-bf16"])
@pytest.mark.parametrize("F,L,sizes", FIXTURES, ids=IDS)
def test_top_layer_flavours_equal_the_general_code(F, L, sizes, engine, monkeypatch):
    """NQ_NO_TOPLAYER unset against =1: loss, energies, forces and the flat gradient value-equal, with the stored-adjoint second-order sweep (the default) and
    with the full stacked sweep (NQ_NO_LITE=1), on the exact-f32 engine and with every eligible product on the split-bf16 engine.  The launch profiler sees
    the upd_rev_top class exactly when the flavour is on (two launches per sweep; at L = 1 no general upd_rev launch is left)."""
    from nabladft_amd import _lib
    _clear(monkeypatch)
    lib = _lib.load()
    model, batch = _fixture(F, L, sizes)
    lib.nq_set_gemm_variant(engine)
    try:
        for lite in (True, False):
            if lite:
                monkeypatch.delenv("NQ_NO_LITE", raising=False)
            else:
                monkeypatch.setenv("NQ_NO_LITE", "1")
            monkeypatch.setenv("NQ_NO_TOPLAYER", "1")
            general = _step(model, batch)
            names_general = _kernel_names_of(lambda: _step(model, batch))
            monkeypatch.delenv("NQ_NO_TOPLAYER")
            top = _step(model, batch)
            names_top = _kernel_names_of(lambda: _step(model, batch))
            _assert_equal(top, general, f"lite={lite}")
            assert "upd_rev_top" not in names_general and "upd_rev" in names_general, names_general
            assert "upd_rev_top" in names_top and (("upd_rev" in names_top) == (L > 1)), names_top
            nn_v2 = {n for n in names_top if n.startswith("gemm_nn:V2")}
            assert f"gemm_nn:V2[n={F},k={2 * F}]" in nn_v2 and ((f"gemm_nn:V2[n={F},k={3 * F}]" in nn_v2) == (L > 1)), nn_v2
            assert not any(n.startswith("gemm_nn:V2") and f"k={2 * F}]" in n for n in names_general), names_general
    finally:
        lib.nq_set_gemm_variant(1)


def test_seeded_sweep_keeps_the_general_kernels(monkeypatch):
    """direct_forces=True: the force head seeds a non-zero adjoint of vec_upd, so the backward sweep must run the general update-block reverse kernels and the
    full V2 product at its last layer too, whatever NQ_NO_TOPLAYER says -- and the golden gradients of the reference hold (tests/test_engine_gpu.py checks them
    as well; here next to the launch classes)."""
    from nabladft_amd import L2Loss
    from tests.helpers import check_grads
    _clear(monkeypatch)
    dev = _dev()
    fx, cfg, params = load_case("painn_small_direct.npz")
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    F = cfg.hidden_channels

    def step():
        for p in model.parameters():
            p.grad = None
        model.train()
        energy, forces = model(batch)
        (torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)).backward()
    names = _kernel_names_of(step)
    assert "upd_rev" in names and "upd_rev_top" not in names, names
    assert not any(n.startswith("gemm_nn:V2") and f"k={2 * F}]" in n for n in names), names
    check_grads(fx, {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}, 1e-4, "direct forces")


def test_backward_follows_the_top_layer_choice_of_its_forward_call(monkeypatch):
    """plan_step records `top_layer` with the plan: a backward call made after the switch has flipped runs what the forward call planned."""
    from nabladft_amd import L2Loss
    _clear(monkeypatch)
    model, batch = _fixture(64, 2, SIZES_86)
    monkeypatch.setenv("NQ_NO_TOPLAYER", "1")
    ref = _step(model, batch)

    def flipped():
        for p in model.parameters():
            p.grad = None
        monkeypatch.setenv("NQ_NO_TOPLAYER", "1")
        energy, forces = model(batch)
        loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
        monkeypatch.delenv("NQ_NO_TOPLAYER")
        loss.backward()
    names = _kernel_names_of(flipped)
    assert "upd_rev_top" not in names, names
    assert torch.equal(torch.cat([p.grad.reshape(-1) for _, p in model.named_parameters()]), ref["grad"])


# ---- side stream rule ----------------------------------------------------------------------------------------------------------------------------------------
def test_side_stream_above_16k_atoms_gives_the_single_stream_bits(monkeypatch):
    """400 molecules of 41 atoms (16 400 atoms: just above the former threshold), hidden_channels 64, L = 2.  NQ_SIDE_STREAM unset (the weight-gradient
    products run on the side stream, since no profiler records) against NQ_SIDE_STREAM=0: the same bits; the same step repeated: the same bits."""
    import nabladft_amd as nq
    _clear(monkeypatch)
    dev = _dev()
    cfg = R.PaiNNConfig(hidden_channels=64, num_layers=2, num_rbf=20)
    model = _model(cfg, R.make_params(cfg, seed=5), dev)
    batch = nq.Batch(*_synthetic(41, [41] * 400)).to(dev)
    assert batch.num_nodes == 16400 > 16384
    default = _step(model, batch)
    again = _step(model, batch)
    monkeypatch.setenv("NQ_SIDE_STREAM", "0")
    single = _step(model, batch)
    monkeypatch.setenv("NQ_SIDE_STREAM", "1")
    forced = _step(model, batch)
    _assert_equal(default, single, "default vs NQ_SIDE_STREAM=0")
    _assert_equal(default, again, "repeated")
    _assert_equal(default, forced, "default vs NQ_SIDE_STREAM=1")
