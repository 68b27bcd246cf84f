#!/usr/bin/env python
"""Writes tests/golden/graphormer_small.npz, graphormer_small_d32.npz and graphormer_yaml.npz from the REAL reference class.

    python scripts/make_golden_graphormer.py --reference /path/to/nablaDFT-checkout [--out tests/golden]

Needs a checkout of the reference (nothing of it is copied).  ``nablaDFT/graphormer/graphormer_3d.py`` is imported by file path behind two
stand-ins of our own: ``pytorch_lightning.LightningModule`` (a torch.nn.Module whose save_hyperparameters does nothing) and
``torch_geometric.utils.to_dense_batch``.  The reference runs in eval() mode, in float64 and in float32, on identical weights
(tests/graphormer_ref.make_params, keyed by parameter name) and inputs (tests/graphormer_ref.make_batch).

The reference casts to float32 inside GaussianLayer.forward and at the end of NodeTaskHead.forward (``.float()``) whatever the module's dtype; for the
float64 run ``torch.Tensor.float`` is made the identity, so that the float64 run is float64 throughout.

Recorded (float64): gbf / efeat / attention bias on real pairs (the large per-pair arrays only for the first molecules: a committed file stays below 1 MiB),
the output of every encoder layer application, E and F on real atoms, the Lightning loss (L1, coefficients 1 / 1, padded-mean semantics) and its parameter
gradients; ``own32_*``: the reference's own float32 error per array (max |a32 - a64| / max |a64|) and per gradient tensor (|g32 - g64| / |g64|, Frobenius).
The yaml configuration stores per gradient tensor its norm and its projection on tests/graphormer_ref.probe_direction.

Asserted here because the tests rely on it: no NaN; padding independence in float64 (every molecule alone == inside the padded batch: bit for bit at most sizes, < 1e-12 everywhere -- the CPU BLAS picks
its kernels by shape); the
three gradients that vanish by the softmax's shift invariance are < 1e-12 of their module's weight gradient norm; the ragged restatement
(tests/graphormer_ref.forward) agrees with the reference to 1e-10.
"""
import argparse
import importlib.util
import os
import sys
import types
from contextlib import contextmanager, nullcontext
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import graphormer_ref as G  # noqa: E402


def to_dense_batch(x, batch, batch_size=None):
    B = int(batch.max()) + 1 if batch_size is None else int(batch_size)
    counts = torch.bincount(batch, minlength=B)
    start = torch.cumsum(counts, 0) - counts
    local = torch.arange(batch.numel()) - start[batch]
    out = x.new_zeros((B, int(counts.max())) + tuple(x.shape[1:]))
    mask = torch.zeros(B, int(counts.max()), dtype=torch.bool)
    out[batch, local] = x
    mask[batch, local] = True
    return out, mask


def load_reference(path):
    class LightningModule(torch.nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass

    pl = types.ModuleType("pytorch_lightning")
    pl.LightningModule = LightningModule
    tg, tgu = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.utils")
    tgu.to_dense_batch = to_dense_batch
    tg.utils = tgu
    sys.modules.update({"pytorch_lightning": pl, "torch_geometric": tg, "torch_geometric.utils": tgu})
    spec = importlib.util.spec_from_file_location("ref_graphormer_3d", os.path.join(path, "nablaDFT", "graphormer", "graphormer_3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextmanager
def float_is_identity():
    torch.Tensor.float = lambda self: self
    try:
        yield
    finally:
        del torch.Tensor.float


def as_data(batch, dtype):
    sizes = batch["sizes"]
    return SimpleNamespace(z=batch["z"], pos=batch["pos"].to(dtype), batch=torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)),
                           y=batch["y"].to(dtype), forces=batch["forces"].to(dtype))


def run(ref, cfg, params, batch, dtype):
    """One eval() forward + Lightning loss + backward of the reference.  -> dict of real-atom / real-pair arrays (float64 numpy) and gradients."""
    sizes = batch["sizes"]
    net = ref.Graphormer3D(**cfg, **G.DROPOUTS).to(dtype)
    assert list(net.state_dict().keys()) == list(params.keys())
    assert all(tuple(v.shape) == tuple(params[k].shape) for k, v in net.state_dict().items())
    net.load_state_dict({k: v.to(dtype) for k, v in params.items()})
    net.eval()
    task = ref.Graphormer3DLightning("g3d", net, None, None, torch.nn.L1Loss(), None, 0, 1.0, 1.0)
    task.eval()
    cap = dict(layers=[])
    hooks = [net.gbf.register_forward_hook(lambda m, i, o: cap.__setitem__("gbf", o.detach())),
             net.bias_proj.register_forward_hook(lambda m, i, o: cap.__setitem__("bias", o.detach())),
             net.edge_proj.register_forward_pre_hook(lambda m, i: cap.__setitem__("efeat", i[0].detach()))]
    hooks += [lay.register_forward_hook(lambda m, i, o: cap["layers"].append(o.detach().transpose(0, 1))) for lay in net.layers]
    data = as_data(batch, dtype)
    with (float_is_identity() if dtype == torch.float64 else nullcontext()):
        energy, node, mask = net(data)
        cap_first = dict(cap, layers=list(cap["layers"]))
        loss = task.step(data)
        loss.backward()
    for h in hooks:
        h.remove()
    _, m = to_dense_batch(data.z, data.batch)
    pm = (m.unsqueeze(1) & m.unsqueeze(2))
    out = dict(energy=energy.detach(), forces=node.detach()[m], loss=loss.detach(), gbf=cap_first["gbf"][pm], bias=cap_first["bias"][pm], efeat=cap_first["efeat"][m],
               layer_out=torch.stack([t[m] for t in cap_first["layers"]]))
    assert bool(mask.squeeze(-1).eq(m).all())
    out = {k: v.double().numpy() for k, v in out.items()}
    out["grads"] = {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().double().numpy() for k, p in net.named_parameters()}
    for k, v in list(out.items()) + list(out["grads"].items()):
        if k != "grads":
            assert np.isfinite(v).all(), k
    return out


def shift_norm_name(name):
    """The tensor whose float64 gradient norm normalises ``name``: its own, except for the two whole tensors that vanish by shift invariance."""
    return {"bias_proj.layer2.bias": "bias_proj.layer2.weight", "node_proj.k_proj.bias": "node_proj.k_proj.weight"}.get(name, name)


def rel_max(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def record(ref, cfg, sizes, seed, full):
    params = G.make_params(cfg, seed)
    batch = G.make_batch(sizes, seed + 1)
    r64, r32 = run(ref, cfg, params, batch, torch.float64), run(ref, cfg, params, batch, torch.float32)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    # padding independence, float64: each molecule alone == inside the padded batch (exact, or an ulp where the BLAS kernel differs by shape)
    for b, n in enumerate(sizes):
        one = dict(z=batch["z"][ptr[b]:ptr[b + 1]], pos=batch["pos"][ptr[b]:ptr[b + 1]], y=batch["y"][b:b + 1], forces=batch["forces"][ptr[b]:ptr[b + 1]], sizes=(n,))
        alone = run(ref, cfg, params, one, torch.float64)
        de, df = rel_max(alone["energy"], r64["energy"][b:b + 1]), rel_max(alone["forces"], r64["forces"][ptr[b]:ptr[b + 1]])
        print("padding independence, molecule of %d atoms: E %.1e F %.1e" % (n, de, df))
        assert de < 1e-12 and df < 1e-12, ("padding", b, de, df)
    g64, E = r64["grads"], cfg["embed_dim"]
    wn = np.linalg.norm(g64["bias_proj.layer2.weight"])
    assert np.linalg.norm(g64["bias_proj.layer2.bias"]) < 1e-12 * wn
    assert np.linalg.norm(g64["node_proj.k_proj.bias"]) < 1e-12 * np.linalg.norm(g64["node_proj.k_proj.weight"])
    for l in range(cfg["layers"]):
        assert np.linalg.norm(g64[f"layers.{l}.self_attn.in_proj.bias"][E:2 * E]) < 1e-12 * np.linalg.norm(g64[f"layers.{l}.self_attn.in_proj.weight"])
    # the ragged restatement is the reference's function
    mine, mloss, mgrads = G.loss_and_grads(params, cfg, batch)
    for k in ("energy", "forces", "gbf", "efeat", "bias", "layer_out"):
        assert rel_max(mine[k].detach().numpy(), r64[k]) < 1e-10, (k, rel_max(mine[k].detach().numpy(), r64[k]))
    assert abs(float(mloss.detach()) - float(r64["loss"])) < 1e-10 * abs(float(r64["loss"]))
    for k, g in mgrads.items():
        assert np.linalg.norm(g.numpy() - g64[k]) < 1e-10 * np.linalg.norm(g64[shift_norm_name(k)]), k
    out = dict(keys=np.array(list(params.keys())), sizes=np.array(sizes), seed=np.array(seed), z=batch["z"].numpy(), pos=batch["pos"].numpy(), y=batch["y"].numpy(),
               forces_target=batch["forces"].numpy(), energy=r64["energy"], forces=r64["forces"], loss=r64["loss"])
    for k in ("energy", "forces"):
        out["own32_" + k] = np.array(rel_max(r32[k], r64[k]))
    out["own32_loss"] = np.array(abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"])))
    if full == "layers":
        n_at, n_pr = int(ptr[4]), int((np.asarray(sizes[:3]) ** 2).sum())          # first four molecules' atoms, first three molecules' pairs
        out.update(efeat=r64["efeat"], gbf=r64["gbf"][:n_pr], bias=r64["bias"][:n_pr], layer_out=r64["layer_out"][:, :n_at], n_atoms_layers=np.array(n_at),
                   n_pairs=np.array(n_pr))
        for k in ("efeat", "gbf", "bias"):
            out["own32_" + k] = np.array(rel_max(r32[k], r64[k]))
        out["own32_layer_out"] = np.array([rel_max(a, b) for a, b in zip(r32["layer_out"], r64["layer_out"])])
    for k, g in g64.items():
        nrm = np.linalg.norm(g64[shift_norm_name(k)])
        out["own32_grad:" + k] = np.array(np.linalg.norm(r32["grads"][k] - g) / nrm)
        if full == "probes":
            d = G.probe_direction(k, g.shape).numpy()
            out["gnorm:" + k], out["gprobe:" + k] = np.array(np.linalg.norm(g)), np.array((g * d).sum())
            out["own32_gprobe:" + k] = np.array(abs((r32["grads"][k] * d).sum() - (g * d).sum()) / nrm)
        else:
            out["grad:" + k] = g
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = load_reference(a.reference)
    for name, cfg, sizes, seed, full in (("graphormer_small", G.SMALL, G.SMALL_SIZES, 11, "layers"), ("graphormer_small_d32", G.SMALL_D32, G.SMALL_SIZES, 12, "grads"),
                                         ("graphormer_yaml", G.YAML, G.YAML_SIZES, 13, "probes")):
        fx = record(ref, cfg, sizes, seed, full)
        path = os.path.join(a.out, name + ".npz")
        np.savez_compressed(path, **fx)
        print(name, os.path.getsize(path), "bytes;  own32 E %.2e F %.2e worst grad %.2e" % (
            float(fx["own32_energy"]), float(fx["own32_forces"]), max(float(v) for k, v in fx.items() if k.startswith("own32_grad:"))))
        assert os.path.getsize(path) < (1 << 20), "a committed file stays below 1 MiB"
