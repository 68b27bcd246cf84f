"""CPU: the float64 restatement of DimeNet++ (tests/dimenet_ref.py) against the recorded float64 run of the real reference wrapper
(tests/golden/dimenet_*.npz, scripts/make_golden_dimenet.py), and the host-side surface of nabladft_amd.dimenetplusplus (module tree, constructor keywords,
argument checks, the float64 Bessel table, exported symbols, the force-loss refusal).

The restatement-vs-fixture bound is 1e-10: the same function in the same precision.  Gradients are relative to the tensor's float64 norm."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import dimenet_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [("dimenet_small", D.SMALL, D.SMALL_SIZES), ("dimenet_yaml", D.YAML, D.YAML_SIZES)]


def _fx(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _batch(fx, sizes):
    b = D.make_batch(sizes, int(fx["seed"]) + 1)
    for k, f in (("z", "z"), ("pos", "pos"), ("y", "y"), ("forces", "forces_target"), ("batch", "batch")):
        assert np.array_equal(b[k].numpy(), fx[f])
    return b


@pytest.mark.parametrize("name,cfg,sizes", CASES)
def test_restatement_matches_the_reference(name, cfg, sizes):
    fx = _fx(name)
    out = D.run(cfg, D.make_params(cfg, int(fx["seed"])), _batch(fx, sizes))
    assert np.array_equal(out["src"], fx["src"]) and np.array_equal(out["dst"], fx["dst"]) and np.array_equal(out["n_triplets"], fx["n_triplets"])
    rows = fx["rows"]
    assert _rel(out["rbf"][rows], fx["rbf"]) < 1e-10 and _rel(out["rad"][rows], fx["rad"]) < 1e-10
    assert len(out["block_out"]) == cfg["dimenet_num_blocks"] + 1 == fx["block_out"].shape[0]
    for a, b in zip(out["block_out"], fx["block_out"]):
        assert _rel(a[rows], b) < 1e-10
    assert _rel(out["P"], fx["P"]) < 1e-10 and _rel(out["energy"], fx["energy"]) < 1e-10 and _rel(out["forces"], fx["forces"]) < 1e-10
    assert abs(float(out["loss"]) - float(fx["loss"])) < 1e-10 * abs(float(fx["loss"]))
    for k, g in out["grads"].items():
        nrm = float(fx["gnorm:" + k])
        assert nrm > 0, k                                  # every parameter, freq and the output layers included, is reached by the energy loss
        assert abs(float(g.norm()) - nrm) < 1e-10 * nrm, k
        assert abs(float((g * D.probe_direction(k, tuple(g.shape))).sum()) - float(fx["gprobe:" + k])) < 1e-10 * nrm, k
        if "grad:" + k in fx:
            assert np.linalg.norm(g.numpy() - fx["grad:" + k]) < 1e-10 * nrm, k
    # post-processing rescales the energies only
    assert _rel(fx["energy_post"], float(fx["scale"]) * fx["energy"] + float(fx["mean"])) < 1e-14 and np.array_equal(fx["forces_post"], fx["forces"])


def test_forces_are_minus_the_gradient_of_the_energy():
    fx = _fx("dimenet_small")
    params, b = D.make_params(D.SMALL, int(fx["seed"])), _batch(fx, D.SMALL_SIZES)
    model = D.build(D.SMALL, params)
    rng = np.random.default_rng(5)
    direction = torch.from_numpy(rng.normal(size=tuple(b["pos"].shape)))
    h = 1e-5
    _, F, _ = model(b["z"], b["pos"], b["batch"])
    Ep = model(b["z"], b["pos"] + h * direction, b["batch"])[0].detach().sum()
    Em = model(b["z"], b["pos"] - h * direction, b["batch"])[0].detach().sum()
    fd, an = float(Ep - Em) / (2 * h), -float((F * direction).sum())
    assert abs(fd - an) < 1e-7 * max(abs(an), 1.0), (fd, an)


def test_bessel_table_of_the_package_matches_the_fixture():
    from nabladft_amd.dimenetplusplus import bessel_table
    fx = _fx("dimenet_yaml")
    roots, norms = bessel_table(7, 6)
    assert roots.dtype == np.float64 and roots.shape == (7, 6)
    assert np.abs(roots / fx["roots"] - 1).max() < 1e-14 and np.abs(norms / fx["norms"] - 1).max() < 1e-14
    assert abs(roots[1, 0] - 4.493409457909064) < 1e-14 and abs(roots[0, 5] - 6 * np.pi) < 1e-14      # tan x = x; j_0 = sin x / x
    src = open(os.path.join(ROOT, "nabladft_amd", "dimenetplusplus.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|sympy)", src, flags=re.M)


def test_dn_symbols_declared_exported_and_bound():
    from nabladft_amd import _lib
    from nabladft_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nablaq.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nq_dn_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 13 and declared == {k for k in _lib.SYMBOLS if k.startswith("nq_dn_")}
    for name in declared:
        assert hasattr(lib, name)
    assert lib.nq_abi_version() == 17
    import nabladft_amd as nq
    assert nq.DimeNetPlusPlusPotential is nq.dimenetplusplus.DimeNetPlusPlusPotential and nq.DimeNetPlusPlusLightning
    assert "dimenet.hip" in __import__("nabladft_amd.build", fromlist=["SOURCES"]).SOURCES


def test_constructor_keywords_and_state_dict_keys_are_the_reference():
    import nabladft_amd as nq
    for name, cfg, _ in CASES:
        fx = _fx(name)
        net = nq.DimeNetPlusPlusPotential(**cfg)
        task = nq.DimeNetPlusPlusLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=1.0)
        assert list(task.state_dict().keys()) == [str(k) for k in fx["keys"]]
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == D.param_shapes(cfg)
        net.load_state_dict({k: v.float() for k, v in D.make_params(cfg, 0).items()})
    fx = _fx("dimenet_small")
    for cls, key in ((nq.DimeNetPlusPlusPotential, "potential_kwargs"), (nq.DimeNetPlusPlusLightning, "lightning_kwargs")):
        assert list(inspect.signature(cls.__init__).parameters)[1:] == [str(k) for k in fx[key]]
    ref_defaults = dict(scaler=None, dimenet_hidden_channels=128, dimenet_num_blocks=4, dimenet_int_emb_size=64, dimenet_basis_emb_size=8,
                        dimenet_out_emb_channels=256, dimenet_num_spherical=7, dimenet_num_radial=6, dimenet_max_num_neighbors=32, dimenet_envelope_exponent=5,
                        dimenet_num_before_skip=1, dimenet_num_after_skip=2, dimenet_num_output_layers=3, cutoff=5.0, do_postprocessing=False)
    sig = inspect.signature(nq.DimeNetPlusPlusPotential.__init__).parameters
    assert {k: sig[k].default for k in ref_defaults} == ref_defaults
    net = nq.DimeNetPlusPlusPotential(50)                   # the class defaults
    assert float(net.net.output_blocks[0].lin.weight.detach().abs().max()) == 0.0 and float(net.net.emb.emb.weight.detach().abs().max()) <= 3 ** 0.5
    assert torch.allclose(net.net.rbf.freq.detach(), torch.arange(1, 7) * torch.pi)
    sched = nq.DimeNetPlusPlusLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=1.0,
                                        lr_scheduler=torch.optim.lr_scheduler.ReduceLROnPlateau, scheduler_args=dict(factor=0.8, patience=10),
                                        optimizer=lambda p: torch.optim.AdamW(p, lr=1e-3)).configure_optimizers()
    assert isinstance(sched["lr_scheduler"], torch.optim.lr_scheduler.ReduceLROnPlateau) and sched["monitor"] == "val/loss"


def test_unsupported_sizes_raise():
    import nabladft_amd as nq
    for bad in (dict(dimenet_int_emb_size=96), dict(dimenet_int_emb_size=512), dict(dimenet_basis_emb_size=16), dict(dimenet_num_spherical=9),
                dict(dimenet_num_radial=17), dict(dimenet_hidden_channels=100), dict(dimenet_out_emb_channels=200), dict(dimenet_envelope_exponent=0),
                dict(dimenet_num_blocks=0)):
        with pytest.raises(NotImplementedError):
            nq.DimeNetPlusPlusPotential(50, **bad)
    net = nq.DimeNetPlusPlusPotential(50, dimenet_num_blocks=1)
    with pytest.raises(RuntimeError, match="MI355X only"):             # no CPU fallback
        net(nq.Batch(torch.zeros(3, 3), torch.tensor([1, 6, 8]), torch.zeros(3, dtype=torch.long)))


def test_training_step_refuses_a_force_loss_only():
    import nabladft_amd as nq
    net = nq.DimeNetPlusPlusPotential(50, dimenet_num_blocks=1)
    batch = nq.Batch(torch.zeros(3, 3), torch.tensor([1, 6, 8]), torch.zeros(3, dtype=torch.long))
    task = nq.DimeNetPlusPlusLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=1.0)     # constructing is fine
    with pytest.raises(NotImplementedError, match="second-order"):
        task.training_step(batch, 0)
    task = nq.DimeNetPlusPlusLightning(net=net, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=0.0)
    with pytest.raises(RuntimeError, match="MI355X only"):             # passes the refusal and reaches the model (which has no CPU path)
        task.training_step(batch, 0)
