"""CPU: the float64 ragged restatement of Graphormer3D (tests/graphormer_ref.py) against the recorded float64 run of the real reference class
(tests/golden/graphormer_*.npz, scripts/make_golden_graphormer.py), its analytic operator backwards against float64 autograd, and the host-side surface of
nabladft_amd.graphormer (module tree, argument checks, exported symbols).

The restatement-vs-fixture bound is 1e-10: the same function evaluated in the same precision, only the summation order differs.  Gradients are relative to
the tensor's float64 norm; the two whole tensors that vanish by the softmax's shift invariance (bias_proj.layer2.bias, node_proj.k_proj.bias) are relative
to the norm of the weight gradient of the same module."""
import os
import re

import numpy as np
import pytest
import torch

from tests import graphormer_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHIFT = {"bias_proj.layer2.bias": "bias_proj.layer2.weight", "node_proj.k_proj.bias": "node_proj.k_proj.weight"}


def _fx(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _batch(fx):
    b = G.make_batch(tuple(int(n) for n in fx["sizes"]), int(fx["seed"]) + 1)
    for k, f in (("z", "z"), ("pos", "pos"), ("y", "y"), ("forces", "forces_target")):              # the generator's inputs are the fixture's
        assert np.array_equal(b[k].numpy(), fx[f])
    return b


@pytest.mark.parametrize("name,cfg", [("graphormer_small", G.SMALL), ("graphormer_small_d32", G.SMALL_D32)])
def test_restatement_matches_the_reference(name, cfg):
    fx = _fx(name)
    assert [str(k) for k in fx["keys"]] == [k for k, _ in G.param_shapes(cfg)]
    params = G.make_params(cfg, int(fx["seed"]))
    out, loss, grads = G.loss_and_grads(params, cfg, _batch(fx))
    assert _rel(out["energy"].detach(), fx["energy"]) < 1e-10 and _rel(out["forces"].detach(), fx["forces"]) < 1e-10
    assert abs(float(loss.detach()) - float(fx["loss"])) < 1e-10 * abs(float(fx["loss"]))
    if "layer_out" in fx:
        na, npairs = int(fx["n_atoms_layers"]), int(fx["n_pairs"])
        assert _rel(out["efeat"].detach(), fx["efeat"]) < 1e-10
        assert _rel(out["gbf"].detach()[:npairs], fx["gbf"]) < 1e-10 and _rel(out["bias"].detach()[:npairs], fx["bias"]) < 1e-10
        assert fx["layer_out"].shape[0] == cfg["blocks"] * cfg["layers"]
        for a, b in zip(out["layer_out"].detach()[:, :na], fx["layer_out"]):
            assert _rel(a, b) < 1e-10
    for k, g in grads.items():
        ref = fx["grad:" + k]
        nrm = np.linalg.norm(fx["grad:" + SHIFT.get(k, k)])
        assert np.linalg.norm(g.numpy() - ref) < 1e-10 * nrm, k
    E = cfg["embed_dim"]                                       # the three shift-invariant gradients are zero in the reference
    assert np.linalg.norm(fx["grad:bias_proj.layer2.bias"]) < 1e-12 * np.linalg.norm(fx["grad:bias_proj.layer2.weight"])
    assert np.linalg.norm(fx["grad:layers.0.self_attn.in_proj.bias"][E:2 * E]) < 1e-12 * np.linalg.norm(fx["grad:layers.0.self_attn.in_proj.weight"])
    assert np.abs(fx["grad:tag_encoder.weight"][[0, 2]]).max() == 0 and np.abs(fx["grad:energy_agg_factor.weight"][[0, 2]]).max() == 0


def test_restatement_matches_the_reference_yaml():
    fx = _fx("graphormer_yaml")
    params = G.make_params(G.YAML, int(fx["seed"]))
    out, loss, grads = G.loss_and_grads(params, G.YAML, _batch(fx))
    assert _rel(out["energy"].detach(), fx["energy"]) < 1e-10 and _rel(out["forces"].detach(), fx["forces"]) < 1e-10
    assert abs(float(loss.detach()) - float(fx["loss"])) < 1e-10 * abs(float(fx["loss"]))
    for k, g in grads.items():
        nrm = float(fx["gnorm:" + SHIFT.get(k, k)])
        assert abs(float(g.norm()) - float(fx["gnorm:" + k])) < 1e-10 * nrm, k
        assert abs(float((g * G.probe_direction(k, tuple(g.shape))).sum()) - float(fx["gprobe:" + k])) < 1e-10 * nrm, k


# ---- analytic operator backwards against float64 autograd ---------------------------------------------------------------------------------------------------
def _ops_case(H=2, d=16, K=8, sizes=(1, 2, 5, 9), seed=3):
    g = torch.Generator().manual_seed(seed)
    b = G.make_batch(sizes, seed)
    ptr, pair_ptr, _ = G.structure(sizes)
    N, P, E = int(ptr[-1]), int(pair_ptr[-1]), H * d
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    keep = (torch.rand(P, H, generator=g) >= 0.3).to(torch.float64)
    return dict(b=b, ptr=ptr, pair_ptr=pair_ptr, N=N, P=P, E=E, H=H, K=K, qkv=r(N, 3 * E), bias=r(P, H), keep=keep, W3=r(3, E), b3=r(3), r=r,
                unit=G.pair_geometry(b["pos"], b["z"], ptr)[1])


def _close(a, b, tol=1e-11):
    assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-30), (float((a - b).abs().max()), float(b.abs().max()))


def test_pair_featuriser_backward_is_the_autograd_adjoint():
    c = _ops_case()
    r, K = c["r"], c["K"]
    mul = (1.0 + 0.2 * r(G.EDGE_TYPES, 1)).requires_grad_(True)
    bias = (0.2 * r(G.EDGE_TYPES, 1)).requires_grad_(True)
    means = (torch.rand(1, K, dtype=torch.float64) * 3).requires_grad_(True)
    stds = torch.tensor([[0.7, -1.3, 0.0, 2.0, -0.4, 1.1, 0.9, -2.5]], dtype=torch.float64, requires_grad=True)       # negative entries and an exact zero
    gbf, unit, dist, efeat = G.pair_features(c["b"]["pos"], c["b"]["z"], c["ptr"], mul, bias, means, stds)
    # the self pair: distance 0, unit vector 0; the truncated pi
    assert float(dist.detach()[0]) == 0.0 and float(unit.detach()[0].abs().max()) == 0.0
    s0 = abs(float(stds.detach()[0, 0])) + 1e-5
    x0 = float(bias.detach()[int(c["b"]["z"][0]) * 65, 0])                # x = mul * 0 + bias
    assert abs(float(gbf.detach()[0, 0]) - np.exp(-0.5 * ((x0 - float(means.detach()[0, 0])) / s0) ** 2) / ((2 * 3.14159) ** 0.5 * s0)) < 1e-14
    g_gbf, g_ef = r(*gbf.shape), r(*efeat.shape)
    ref = torch.autograd.grad((gbf * g_gbf).sum() + (efeat * g_ef).sum(), [means, stds, mul, bias])
    got = G.pair_features_backward(c["b"]["pos"], c["b"]["z"], c["ptr"], mul.detach(), bias.detach(), means.detach(), stds.detach(), g_gbf, g_ef)
    for a, b_ in zip(got, ref):
        _close(a.reshape(-1), b_.reshape(-1))
    assert float(got[1][2]) == 0.0                                       # stds exactly 0: torch's convention for |.|, gradient 0
    only_e = G.pair_features_backward(c["b"]["pos"], c["b"]["z"], c["ptr"], mul.detach(), bias.detach(), means.detach(), stds.detach(), None, g_ef)
    _close(only_e[0], torch.autograd.grad((G.pair_features(c["b"]["pos"], c["b"]["z"], c["ptr"], mul, bias, means, stds)[3] * g_ef).sum(), means)[0].reshape(-1))


@pytest.mark.parametrize("masked", [False, True])
def test_attention_backward_is_the_autograd_adjoint(masked):
    c = _ops_case()
    qkv, bias = c["qkv"].clone().requires_grad_(True), c["bias"].clone().requires_grad_(True)
    keep, scale = (c["keep"], 1.0 / 0.7) if masked else (None, 1.0)
    out = G.attention(qkv, bias, c["ptr"], c["pair_ptr"], c["H"], 0.25, keep, scale)
    g = c["r"](*out.shape)
    ref = torch.autograd.grad((out * g).sum(), [qkv, bias])
    got = G.attention_backward(qkv.detach(), bias.detach(), c["ptr"], c["pair_ptr"], c["H"], 0.25, g, keep, scale)
    _close(got[0], ref[0]), _close(got[1], ref[1])
    shifted = G.attention(qkv.detach(), bias.detach() + 3.0, c["ptr"], c["pair_ptr"], c["H"], 0.25, keep, scale)      # shift invariance of the softmax
    _close(shifted, out.detach(), 1e-12)


@pytest.mark.parametrize("masked", [False, True])
def test_force_head_backward_is_the_autograd_adjoint(masked):
    c = _ops_case()
    qkv, bias, W3, b3 = (c[k].clone().requires_grad_(True) for k in ("qkv", "bias", "W3", "b3"))
    keep, scale = (c["keep"], 1.0 / 0.7) if masked else (None, 1.0)
    f = G.force_head(qkv, bias, c["unit"], W3, b3, c["ptr"], c["pair_ptr"], c["H"], 0.25, keep, scale)
    g = c["r"](*f.shape)
    ref = torch.autograd.grad((f * g).sum(), [qkv, bias, W3, b3])
    got = G.force_head_backward(qkv.detach(), bias.detach(), c["unit"], W3.detach(), c["ptr"], c["pair_ptr"], c["H"], 0.25, g, keep, scale)
    for a, b_ in zip(got, ref):
        _close(a, b_)
    assert float(f[0].detach().sub(b3.detach()).abs().max()) == 0.0      # a single atom: only the self pair, unit vector 0


def test_gelu_and_layouts():
    x = torch.tensor([-9.0, -6.5, -1.0, -1e-3, 0.0, 1e-3, 0.5, 2.0, 6.5, 9.0], dtype=torch.float64, requires_grad=True)
    y = G.gelu(x)
    _close(y.detach(), torch.nn.functional.gelu(x.detach()), 1e-15)
    g = torch.linspace(-1, 1, x.numel(), dtype=torch.float64)
    _close(G.gelu_backward(x.detach(), g), torch.autograd.grad((y * g).sum(), x)[0], 1e-14)
    sizes, H = (1, 2, 5), 3
    pm = torch.arange(sum(n * n for n in sizes) * H, dtype=torch.float64).reshape(-1, H)
    hm = G.to_heads(pm, sizes)
    assert torch.equal(G.from_heads(hm, sizes, H), pm)
    assert float(hm[H * 1 + 1 * 4 + 1 * 2 + 0]) == float(pm[1 + 1 * 2 + 0, 1])      # molecule 1 (n = 2), head 1, pair (1, 0)


# ---- host-side surface -------------------------------------------------------------------------------------------------------------------------------------
def test_module_tree_is_the_reference_state_dict():
    import nabladft_amd as nq
    for name, cfg in (("graphormer_small", G.SMALL), ("graphormer_small_d32", G.SMALL_D32), ("graphormer_yaml", G.YAML)):
        net = nq.Graphormer3D(**cfg, **G.DROPOUTS)
        sd = net.state_dict()
        assert list(sd.keys()) == [str(k) for k in _fx(name)["keys"]]
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in G.param_shapes(cfg)]
    assert torch.equal(net.atom_encoder.weight[0], torch.zeros(512)) and torch.equal(net.gbf.mul.weight, torch.ones(4096, 1))
    assert float(net.gbf.bias.weight.abs().max()) == 0.0 and 0.0 <= float(net.gbf.stds.weight.min()) and float(net.gbf.means.weight.max()) <= 3.0
    assert float(net.energy_agg_factor.weight.abs().max()) < 0.1
    net.load_state_dict(G.make_params(G.YAML, 0))
    task = nq.Graphormer3DLightning("Graphormer3D-small", net, lambda params: torch.optim.Adam(params, lr=3e-4),
                                    lambda optimizer: nq.schedulers.get_linear_schedule_with_warmup(optimizer, 10, 100), torch.nn.L1Loss(), None, 10, 1.0, 1.0)
    opt = task.configure_optimizers()
    assert opt["lr_scheduler"]["interval"] == "step" and isinstance(opt["optimizer"], torch.optim.Adam)
    sched = opt["lr_scheduler"]["scheduler"]
    assert sched.get_last_lr()[0] == 0.0
    opt["optimizer"].step(), sched.step()
    assert abs(sched.get_last_lr()[0] - 3e-5) < 1e-12
    assert list(task.state_dict().keys())[0] == "net.atom_encoder.weight"


def test_unsupported_arguments_raise():
    import nabladft_amd as nq
    kw = dict(blocks=1, layers=1, ffn_embed_dim=32, num_kernel=8, **G.DROPOUTS)
    for E, H in ((64, 8), (64, 1), (48, 4), (60, 4)):                    # head dimensions 8, 64, 12, 15
        with pytest.raises(NotImplementedError):
            nq.Graphormer3D(embed_dim=E, attention_heads=H, **kw)
    net = nq.Graphormer3D(embed_dim=64, attention_heads=4, **kw)
    pos = torch.zeros(3, 3)
    for bad in (64, 0, -1, 100):
        with pytest.raises(ValueError):
            net(nq.Batch(pos, torch.tensor([1, 6, bad]), torch.zeros(3, dtype=torch.long)))
    with pytest.raises(RuntimeError, match="MI355X only"):             # no CPU fallback
        net(nq.Batch(pos, torch.tensor([1, 6, 8]), torch.zeros(3, dtype=torch.long)))


def test_g3d_symbols_declared_exported_and_bound():
    from nabladft_amd import _lib
    from nabladft_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nablaq.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nq_g3d_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 16 and declared == {k for k in _lib.SYMBOLS if k.startswith("nq_g3d_")}
    for name in declared:
        assert hasattr(lib, name)
    assert lib.nq_g3d_max_mol_atoms() >= 256
    import nabladft_amd as nq
    assert nq.Graphormer3D is nq.graphormer.Graphormer3D and nq.Graphormer3DLightning and nq.graphormer.max_molecule_atoms() == lib.nq_g3d_max_mol_atoms()
