"""Layer-0 flavours of the message path (csrc/edge.hip k_msgf_fwd<.., L0>, k_msgf_rev_l0, csrc/molpair.hip k_gwr_mol<true>; plan_step's `layer0`).

At layer 0 vec_in0 = 0 and every input tangent is 0, so part b of the radial filter only multiplies zeros.  The layer-0 flavours leave that work out;
NQ_NO_LAYER0=1 runs the general kernels at every layer.  The specialised kernels perform a subset of the general kernels' roundings, so against a float64
evaluation of the same step (oracle.painn_sweeps.Sweeps) they must not be further away than the general ones: bound 1.25 x the general flavour's error per
quantity (25 % for the different FMA contraction of the shortened expressions).  Both figures are printed before the assertion."""
import numpy as np
import pytest
import torch

from oracle import painn_ref as R
from oracle.painn_sweeps import Sweeps, loss_and_seeds
from tests.helpers import load_case, rel_err, check_grads
from tests.test_engine_gpu import _batch, _dev, _kernel_names_of, _lds_cap, _model

pytestmark = pytest.mark.gpu

FACTOR = 1.25
L0_CLASSES = {"msgf_fwd_l0", "msgf_tan_l0", "msgf_rev_force_l0", "msgf_rev_dual_ng_l0", "gwr_mol_l0"}


class _TracingSweeps(Sweeps):
    """Sweeps that also keeps the [N][3F] node adjoints it scatters: in a reverse sweep the last one is the adjoint of xh at layer 0."""

    def __init__(self, *a):
        super().__init__(*a)
        self.scattered = []

    def _scatter(self, src, index, n):
        out = super()._scatter(src, index, n)
        if out.dim() == 2 and out.shape[1] == 3 * self.F:
            self.scattered.append(out)
        return out


def _flavour(monkeypatch, general):
    if general:
        monkeypatch.setenv("NQ_NO_LAYER0", "1")
    else:
        monkeypatch.delenv("NQ_NO_LAYER0", raising=False)


def _clear(monkeypatch):
    for k in ("NQ_NO_FUSED_FILTER", "NQ_NO_MOLGW", "NQ_MOLGW", "NQ_MOLGW_CAP", "NQ_NO_LITE", "NQ_NO_LAYER0", "NQ_NO_FUSED_UPDATE"):
        monkeypatch.delenv(k, raising=False)


def _gpu_step(model, batch, gxh=True):
    """One step as PaiNNLightning does it; returns the compared quantities as flat float32 tensors on the device."""
    from nabladft_amd import L2Loss
    for p in model.parameters():
        p.grad = None
    model.train()
    energy, forces = model(batch)
    loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
    loss.backward()
    out = {"energy": energy.detach(), "forces": forces.detach().reshape(-1),
           "grad": torch.cat([p.grad.reshape(-1) for _, p in model.named_parameters()])}
    for name in ("x_msg", "vec_msg"):
        out[name] = model.workspace_view(name, 0).clone()
        out["t_" + name] = model.workspace_view(name, 0, True).clone()
    if gxh:
        out["gxh"] = model.workspace_view("gxh", 0).clone()
    torch.cuda.synchronize()
    return out


def _ref_step(cfg, params, pos, z, batch, y, ft, edge_index):
    """The same step in float64 on the CPU."""
    p64 = {k: v.double() for k, v in params.items()}
    sw = _TracingSweeps(p64, cfg, pos.double(), z, batch, edge_index)
    e, f = sw.energy_forces()
    _, gE, gF = loss_and_seeds(e, f, y.double(), ft.double())
    G = sw.backward(gE, gF)
    names = [k for k, _ in R.param_shapes(cfg)]
    ref = {"energy": e, "forces": f.reshape(-1), "grad": torch.cat([G[k].reshape(-1) for k in names]), "gxh": sw.scattered[-1].reshape(-1)}
    for name in ("x_msg", "vec_msg"):
        ref[name] = sw.ws[f"{name}0"].reshape(-1)
        ref["t_" + name] = sw.ws[f"t_{name}0"].reshape(-1)
    return {k: v.numpy() for k, v in ref.items()}


def _rbf_b_rows(model, cfg):
    """Rows F..2F of layer 0's rbf_proj weight and bias gradient."""
    F = cfg.hidden_channels
    g = dict(model.named_parameters())
    return g["message_layers.0.rbf_proj.weight"].grad[F:2 * F], g["message_layers.0.rbf_proj.bias"].grad[F:2 * F]


def _both_flavours(model, cfg, batch, monkeypatch, gxh=True):
    res = {}
    for tag in ("general", "layer0"):
        _flavour(monkeypatch, tag == "general")
        res[tag] = _gpu_step(model, batch, gxh)
        wb, bb = _rbf_b_rows(model, cfg)
        assert bool((wb == 0).all()) and bool((bb == 0).all()), f"{tag}: part b of the layer-0 rbf_proj gradient must be exactly zero"
    return res


def _assert_not_worse(case, res, ref):
    lines, bad = [], []
    for k in ref:
        eg, el = rel_err(res["general"][k].cpu().numpy(), ref[k]), rel_err(res["layer0"][k].cpu().numpy(), ref[k])
        lines.append(f"{case:28s} {k:10s} general {eg:.3e}  layer0 {el:.3e}  ratio {el / max(eg, 1e-30):.3f}")
        if not el <= FACTOR * eg:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


def _synthetic(seed, sizes, spread=1.7):
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.concatenate([rng.uniform(0, (n ** (1 / 3)) * spread + 1.0, size=(n, 3)) for n in sizes]).astype(np.float32)
    bt = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)]).astype(np.int64)
    z = rng.choice([1, 6, 7, 8], size=len(pos)).astype(np.int64)
    y = rng.normal(size=len(sizes)).astype(np.float32)
    ft = rng.normal(0, 0.05, size=pos.shape).astype(np.float32)
    return torch.tensor(pos), torch.tensor(z), torch.tensor(bt), torch.tensor(y), torch.tensor(ft)


def _float64_case(case, cfg, params, data, monkeypatch, expect=L0_CLASSES):
    import nabladft_amd as nq
    dev = _dev()
    pos, z, bt, y, ft = data
    ei, _, _ = R.build_graph(pos, bt, cfg.cutoff, cfg.max_neighbors)
    model = _model(cfg, params, dev)
    batch = nq.Batch(pos, z, bt, y, ft).to(dev)
    assert np.array_equal(model.generate_graph_values(batch)[0].cpu().numpy(), ei.numpy())
    res = _both_flavours(model, cfg, batch, monkeypatch)
    _flavour(monkeypatch, False)
    names = _kernel_names_of(lambda: _gpu_step(model, batch))
    assert expect <= names, names
    _flavour(monkeypatch, True)
    assert not (L0_CLASSES & _kernel_names_of(lambda: _gpu_step(model, batch)))
    _assert_not_worse(case, res, _ref_step(cfg, params, pos, z, bt, y, ft, ei))
    return model, batch, res


def test_ragged_fixture_against_float64(monkeypatch):
    """painn_small_ragged.npz with the per-molecule rbf_proj gradient forced: fewer than 2048 atoms (static striding), molecules of 1 to 40 atoms."""
    _clear(monkeypatch)
    monkeypatch.setenv("NQ_MOLGW", "1")
    fx, cfg, params = load_case("painn_small_ragged.npz")
    data = tuple(torch.tensor(fx[k]) for k in ("pos", "z", "batch", "y", "f_target"))
    _float64_case("ragged", cfg, params, data, monkeypatch)


@pytest.mark.parametrize("F,sizes", [(64, [5, 12, 1, 9, 20]), (128, [7, 3, 18, 11, 26, 2])])
def test_small_models_against_float64(F, sizes, monkeypatch):
    """F = 64: one slice, one channel per lane.  F = 128 below 2048 atoms: every row as two half-width slices (two wavefronts per atom)."""
    _clear(monkeypatch)
    monkeypatch.setenv("NQ_MOLGW", "1")
    cfg = R.PaiNNConfig(hidden_channels=F, num_layers=2, num_rbf=32)
    _float64_case(f"F={F}", cfg, R.make_params(cfg, seed=F), _synthetic(F, sizes), monkeypatch)


def test_long_rows_mixed_dispatch_and_an_empty_row_against_float64(monkeypatch):
    """A compact 80-atom cluster (rows of more than 64 edges: the chunk loop of the forward / tangent / force flavours; above the LDS limit of k_gwr_mol, so
    the mixed dispatch keeps the general pair-row dual kernel for ITS rows while the other molecules take the layer-0 flavour) next to a molecule with one atom
    beyond the cutoff of all others (an empty row: x_msg = x_in, vec_msg = 0 must still be written)."""
    _clear(monkeypatch)
    monkeypatch.setenv("NQ_MOLGW", "1")
    cfg = R.PaiNNConfig(hidden_channels=64, num_layers=2, num_rbf=24, cutoff=5.0, max_neighbors=100)
    params = R.make_params(cfg, seed=11)
    for k in params:  # keep activations O(1) at degree ~70
        if "rbf_proj" in k or "x_proj.2" in k:
            params[k] = params[k] * 0.3
    rng = np.random.Generator(np.random.PCG64(80))
    cluster = rng.uniform(0, 4.6, size=(80, 3))
    lone = np.concatenate([rng.uniform(0, 2.5, size=(5, 3)), [[30.0, 30.0, 30.0]]])
    others = [rng.uniform(0, (n ** (1 / 3)) * 1.7 + 1.0, size=(n, 3)) for n in (9, 17)]
    parts = [cluster, lone] + others
    pos = torch.tensor(np.concatenate(parts).astype(np.float32))
    bt = torch.tensor(np.concatenate([np.full(len(p), i) for i, p in enumerate(parts)]).astype(np.int64))
    z = torch.tensor(rng.choice([1, 6, 7, 8], size=len(pos)).astype(np.int64))
    y = torch.tensor(rng.normal(size=len(parts)).astype(np.float32))
    ft = torch.tensor(rng.normal(0, 0.05, size=tuple(pos.shape)).astype(np.float32))
    ei, _, _ = R.build_graph(pos, bt, cfg.cutoff, cfg.max_neighbors)
    deg = torch.bincount(ei[1], minlength=len(pos))
    assert int(deg.max()) > 64 and int(deg[80 + 5]) == 0
    assert 80 > _lds_cap()
    model, batch, res = _float64_case("cluster+lone atom", cfg, params, (pos, z, bt, y, ft), monkeypatch,
                                      expect=L0_CLASSES | {"msgf_rev_dual", "gwr_sorted"})
    F = cfg.hidden_channels
    for tag in ("general", "layer0"):   # the empty row
        emb = dict(model.named_parameters())["atom_emb.embeddings.weight"].detach()[z[85] - 1]
        assert torch.equal(res[tag]["x_msg"].view(-1, F)[85], emb)
        assert bool((res[tag]["vec_msg"].view(-1, 3 * F)[85] == 0).all()) and bool((res[tag]["t_vec_msg"].view(-1, 3 * F)[85] == 0).all())
        assert bool((res[tag]["t_x_msg"].view(-1, F)[85] == 0).all())


def test_bench_paths_both_flavours_agree(monkeypatch):
    """110 synthetic conformers (more than 4096 atoms): full-width rows with two channels per lane, rows claimed from counters, the default k_gwr_mol
    dispatch -- the paths of the timed region.  A float64 sweep of this batch takes minutes on the CPU, so the two GPU flavours are compared with each other:
    each is within 1e-5 of float64 (test_engine_gpu.py), their difference is held to the same 1e-5, and energies, forces and the layer-0 buffers to equality."""
    import nabladft_amd as nq
    from nabladft_amd.synth import gen_conformers
    _clear(monkeypatch)
    dev = _dev()
    cfg = R.PaiNNConfig(num_layers=3)
    model = _model(cfg, R.make_params(cfg, seed=21), dev)
    pos, z, bt, y, ft = gen_conformers(21, 110)
    assert pos.shape[0] >= 4096
    batch = nq.Batch(pos, z, bt, y, ft).to(dev)
    res = _both_flavours(model, cfg, batch, monkeypatch)
    _flavour(monkeypatch, False)
    assert L0_CLASSES <= _kernel_names_of(lambda: _gpu_step(model, batch))
    for k in res["general"]:
        e = rel_err(res["layer0"][k].cpu().numpy(), res["general"][k].cpu().numpy())
        print(f"110 conformers {k:10s} layer0 vs general {e:.3e}")
        assert e < 1e-5, (k, e)
        # The layer-0 kernels keep the roundings of the general expressions with the zeros filled in (edge.hip), so what the message path produces is the
        # same bits; the flat gradient alone differs: the layer-0 W1 / W2 weight gradients are summed over N rows instead of 2 N (other split points).
        if k != "grad":
            assert torch.equal(res["layer0"][k], res["general"][k]), k
    again = _gpu_step(model, batch)
    assert all(torch.equal(again[k], res["layer0"][k]) for k in again), "the layer-0 flavours are deterministic"


def _golden_grad_errs(fx, grads):
    """Per parameter, the error measure of tests.helpers.check_grads against the fixture's full ('grad:') or sampled ('gidx:' / 'gval:' / 'gnorm:') gradient."""
    # check_grads asserts a tolerance and returns only the worst figure; the per-parameter ratio needs every figure, so its two formulas are repeated here:
    # a change to the measure in tests/helpers.py:check_grads belongs here as well.
    errs = {}
    for key in fx:
        if key.startswith("grad:"):
            errs[key[5:]] = rel_err(np.asarray(grads[key[5:]]), fx[key])
        elif key.startswith("gidx:"):
            name = key[5:]
            g = np.asarray(grads[name]).reshape(-1).astype(np.float64)
            scale = fx["gnorm:" + name] / np.sqrt(g.size)
            e = float(np.abs(g[fx[key]] - fx["gval:" + name]).max() / max(np.abs(fx["gval:" + name]).max(), scale))
            errs[name] = max(e, abs(float(np.sqrt((g ** 2).sum())) - fx["gnorm:" + name]) / fx["gnorm:" + name])
    return errs


def test_direct_forces_configuration(monkeypatch):
    """direct_forces=True: a first-order backward sweep whose tangents are all zero; vec_in0 = 0 still holds, so the forward flavour and k_gwr_mol<true> run
    (the full dual reverse kernel has no layer-0 form).  The float64 sweeps do not model the force head, so the reference here is the real reference's golden
    vectors: per quantity (energy, forces, every parameter gradient) the layer-0 error <= 1.25 x the general error, next to the absolute bounds of
    test_engine_direct_forces_match_reference."""
    from nabladft_amd import L2Loss
    _clear(monkeypatch)
    monkeypatch.setenv("NQ_MOLGW", "1")
    dev = _dev()
    fx, cfg, params = load_case("painn_small_direct.npz")
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    errs = {}

    def step():
        for p in model.parameters():
            p.grad = None
        model.train()
        energy, forces = model(batch)
        loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
        loss.backward()
        return energy, forces

    for tag in ("general", "layer0"):
        _flavour(monkeypatch, tag == "general")
        out = []
        names = _kernel_names_of(lambda: out.append(step()))
        if tag == "general":
            assert not (L0_CLASSES & names), names
        else:
            assert {"msgf_fwd_l0", "gwr_mol_l0"} <= names, names
        energy, forces = out[0]
        grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
        check_grads(fx, grads, 1e-4, f"direct ({tag})")
        e = {"energy": rel_err(energy.detach().cpu().numpy(), fx["energy"]), "forces": rel_err(forces.detach().cpu().numpy(), fx["forces"])}
        assert e["energy"] < 2e-6 and e["forces"] < 2e-5, (tag, e)
        e.update({"grad " + k: v for k, v in _golden_grad_errs(fx, grads).items()})
        wb, bb = _rbf_b_rows(model, cfg)
        assert bool((wb == 0).all()) and bool((bb == 0).all())
        errs[tag] = e
    lines, bad = [], []
    for k in errs["general"]:
        eg, el = errs["general"][k], errs["layer0"][k]
        lines.append(f"direct forces {k:52s} general {eg:.3e}  layer0 {el:.3e}  ratio {el / max(eg, 1e-30):.3f}")
        if not el <= FACTOR * eg:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert len(lines) > 2 and not bad, "\n".join(bad)


def test_backward_follows_the_layer0_choice_of_its_forward_call(monkeypatch):
    """plan_step's `layer0` is recorded with the plan: a backward call made after the switch has flipped still runs what the forward call planned.  With
    NQ_NO_LAYER0=1 at the forward call every launch is a general kernel (no *_l0 class), and the step is bitwise the step run with the switch set throughout.
    That such a step is also bitwise the step of the commit before the layer-0 flavours cannot be checked from inside one tree: that comparison (bench.py
    --dump-outputs of both builds) is recorded in profiles/layer0_ab.txt, section 4."""
    _clear(monkeypatch)
    monkeypatch.setenv("NQ_MOLGW", "1")
    from nabladft_amd import L2Loss
    dev = _dev()
    fx, cfg, params = load_case("painn_small_ragged.npz")
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    _flavour(monkeypatch, True)
    ref = _gpu_step(model, batch)

    def flipped_step():
        for p in model.parameters():
            p.grad = None
        _flavour(monkeypatch, True)
        energy, forces = model(batch)
        loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
        _flavour(monkeypatch, False)      # flipped between the two calls of the step
        loss.backward()
    names = _kernel_names_of(flipped_step)
    assert not (L0_CLASSES & names), names
    grad = torch.cat([p.grad.reshape(-1) for _, p in model.named_parameters()])
    assert torch.equal(grad, ref["grad"])
    assert torch.equal(model.workspace_view("x_msg", 0, True), ref["t_x_msg"]) and torch.equal(model.workspace_view("gxh", 0), ref["gxh"])
