#!/usr/bin/env python
"""Writes tests/golden/dimenet_small.npz and dimenet_yaml.npz from the REAL reference wrapper around the restated core.

    python scripts/make_golden_dimenet.py --reference /path/to/nablaDFT-checkout [--out tests/golden]

Needs a checkout of the reference (nothing of it is copied).  ``nablaDFT/dimenetplusplus/dimenetplusplus.py`` is imported by file path behind stand-ins of
our own: ``pytorch_lightning.LightningModule`` (a torch.nn.Module whose save_hyperparameters does nothing), ``torch_geometric.data.Data`` and
``torch_geometric.nn.models.DimeNetPlusPlus`` = tests/dimenet_ref.DimeNetPlusPlus, the restatement of the torch-geometric 2.4.0 class (torch-geometric itself
is not available: the core is RESTATED, UNPINNED; the wrapper -- head, forces, post-processing, Lightning ``step`` -- is the reference's own code).

The real ``DimeNetPlusPlusPotential`` and the real ``DimeNetPlusPlusLightning.step`` run in float64 and float32 on identical weights
(tests/dimenet_ref.make_params: every parameter random) and inputs (tests/dimenet_ref.make_batch).  Recorded (float64): inputs, edge list, triplet count per
edge, rbf / Rad / block outputs (on ``rows``, a subset of the edges: a committed file stays below 1 MiB), P, E and F with and without post-processing, the
energy loss (L1, coefficients 1 / 0) and, per gradient tensor, its norm and its projection on tests/dimenet_ref.probe_direction (in the small configuration also the whole tensor where it
has at most 2048 elements -- all of them would be megabytes); the constructor keyword names and the state_dict key list; ``own32:*`` the float32 run's error against
float64 and ``own32x:*`` the same with the bases evaluated in float64 and rounded once (the yardstick of the GPU tests).

Asserted here because the tests rely on it: the sizes include 1, 2 and 3 atoms and a molecule where the neighbour cap bites; an edge without a reverse edge; every
distance >= 0.9 A; |sin theta| > 1e-3 for every triplet; no NaN; each molecule alone equals the molecule inside the batch (float64, 1e-12).
"""
import argparse
import importlib.util
import inspect
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dimenet_ref as D  # noqa: E402


def load_reference(path):
    class LightningModule(torch.nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass

    pl = types.ModuleType("pytorch_lightning")
    pl.LightningModule = LightningModule
    mods = {n: types.ModuleType(n) for n in ("torch_geometric", "torch_geometric.data", "torch_geometric.nn", "torch_geometric.nn.models")}
    mods["torch_geometric.data"].Data = SimpleNamespace
    mods["torch_geometric.nn.models"].DimeNetPlusPlus = D.DimeNetPlusPlus
    sys.modules.update({"pytorch_lightning": pl, **mods})
    spec = importlib.util.spec_from_file_location("ref_dimenetplusplus", os.path.join(path, "nablaDFT", "dimenetplusplus", "dimenetplusplus.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def as_data(b, dtype):
    return SimpleNamespace(z=b["z"], pos=b["pos"].to(dtype).clone(), batch=b["batch"], y=b["y"].to(dtype), forces=b["forces"].to(dtype))


def run_real(ref, cfg, params, b, dtype, exact_basis):
    """The real wrapper: E / F with and without post-processing, the Lightning loss and its gradients."""
    torch.set_default_dtype(dtype)
    try:
        pot = ref.DimeNetPlusPlusPotential(**cfg, scaler=D.SCALER, do_postprocessing=False)
    finally:
        torch.set_default_dtype(torch.float32)
    pot = pot.to(dtype)
    pot.load_state_dict({k: v.to(dtype) for k, v in params.items()})
    pot.net.exact_basis = exact_basis
    pot.eval()
    E, F = pot(as_data(b, dtype))
    rec = pot.net.record
    out = dict(energy=E.detach(), forces=F.detach(), rbf=rec["rbf"].detach(), rad=rec["rad"].detach(), block_out=torch.stack([x.detach() for x in rec["block_out"]]),
               P=rec["P"].detach(), src=rec["src"], dst=rec["dst"], n_triplets=rec["n_triplets"], sin_min=rec["sin_min"], dist_min=rec["dist_min"])
    pot.do_postprocessing = True
    Ep, Fp = pot(as_data(b, dtype))
    out["energy_post"], out["forces_post"] = Ep.detach(), Fp.detach()
    pot.do_postprocessing = False
    task = ref.DimeNetPlusPlusLightning(net=pot, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=0.0)
    task.train()                      # the real forward keeps the graph of the prediction only with create_graph = self.training
    loss = task.step(as_data(b, dtype))
    loss.backward()
    out["loss"] = loss.detach()
    out["grads"] = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in pot.named_parameters()}
    out["keys"] = list(task.state_dict().keys())
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def make(ref, name, cfg, sizes, seed, n_rows, out_dir, full_grads):
    b = D.make_batch(sizes, seed + 1)
    params = D.make_params(cfg, seed)
    r64 = run_real(ref, cfg, params, b, torch.float64, False)
    r32 = run_real(ref, cfg, params, b, torch.float32, False)
    r32x = run_real(ref, cfg, params, b, torch.float32, True)
    src, dst = r64["src"], r64["dst"]
    E, K = len(src), cfg["dimenet_max_num_neighbors"]
    # what the tests rely on
    assert {1, 2, 3} <= set(sizes)
    deg = np.bincount(dst, minlength=len(b["z"]))
    in_cutoff = np.zeros_like(deg)
    pos = b["pos"].numpy()
    for i in range(len(pos)):
        same = np.nonzero(b["batch"].numpy() == int(b["batch"][i]))[0]
        in_cutoff[i] = sum(1 for j in same if j != i and np.linalg.norm(pos[i] - pos[j]) < cfg["cutoff"])
    assert (in_cutoff > K).any() and deg.max() == K, "the neighbour cap must bite"
    pairs = set(zip(src.tolist(), dst.tolist()))
    assert any((i, j) not in pairs for j, i in pairs), "an edge without a reverse edge is needed"
    assert (r64["n_triplets"] == 0).any() and r64["dist_min"] >= 0.9 and r64["sin_min"] > 1e-3
    for r in (r64, r32, r32x):
        for k in ("energy", "forces", "rbf", "rad", "block_out", "P", "loss"):
            assert bool(torch.isfinite(r[k]).all()), k
        assert all(bool(torch.isfinite(g).all()) for g in r["grads"].values())
    assert float(r64["forces"].abs().max()) > 1e-3, "the energy must depend on the positions"
    off = 0
    for n in sizes:                   # each molecule alone == the molecule inside the batch
        sel = slice(off, off + n)
        one = dict(z=b["z"][sel], pos=b["pos"][sel], batch=torch.zeros(n, dtype=torch.long), y=b["y"][:1], forces=b["forces"][sel])
        a = D.run(cfg, params, one, grads=False)
        m = sizes.index(n)
        assert abs(float(a["energy"][0] - r64["energy"][m])) < 1e-12 * max(1.0, abs(float(r64["energy"][m])))
        assert float((a["forces"] - r64["forces"][sel]).abs().max()) < 1e-12 * max(1.0, float(r64["forces"].abs().max()))
        off += n
    own = D.run(cfg, params, b)      # the tests' own wrapper arithmetic == the real wrapper
    assert rel(own["energy"], r64["energy"]) < 1e-12 and rel(own["forces"], r64["forces"]) < 1e-12
    rows = np.unique(np.linspace(0, E - 1, n_rows).astype(np.int64))
    roots, norms = D.bessel_table(cfg["dimenet_num_spherical"], cfg["dimenet_num_radial"])
    fx = dict(seed=np.int64(seed), sizes=np.array(sizes), z=b["z"].numpy(), pos=pos, batch=b["batch"].numpy(), y=b["y"].numpy(), forces_target=b["forces"].numpy(),
              src=src, dst=dst, n_triplets=r64["n_triplets"], rows=rows, rbf=r64["rbf"].numpy()[rows], rad=r64["rad"].numpy()[rows],
              block_out=r64["block_out"].numpy()[:, rows], P=r64["P"].numpy(), energy=r64["energy"].numpy(), forces=r64["forces"].numpy(),
              energy_post=r64["energy_post"].numpy(), forces_post=r64["forces_post"].numpy(), loss=r64["loss"].numpy(), roots=roots, norms=norms,
              scale=np.float64(D.SCALER["scale_"]), mean=np.float64(D.SCALER["mean_"]), keys=np.array(r64["keys"]),
              potential_kwargs=np.array(list(inspect.signature(ref.DimeNetPlusPlusPotential.__init__).parameters)[1:]),
              lightning_kwargs=np.array(list(inspect.signature(ref.DimeNetPlusPlusLightning.__init__).parameters)[1:]))
    for tag, r in (("own32", r32), ("own32x", r32x)):
        for k in ("energy", "forces", "rbf", "rad", "P", "energy_post"):
            fx[f"{tag}:{k}"] = np.float64(rel(r[k], r64[k]))
        fx[f"{tag}:block_out"] = np.array([rel(a, c) for a, c in zip(r["block_out"], r64["block_out"])])
        for k, g in r64["grads"].items():
            fx[f"{tag}:grad:{k}"] = np.float64(float((r["grads"][k].double() - g).norm()) / max(float(g.norm()), 1e-300))
    for k, g in r64["grads"].items():
        fx["gnorm:" + k] = np.float64(float(g.norm()))
        fx["gprobe:" + k] = np.float64(float((g * D.probe_direction(k, tuple(g.shape))).sum()))
        if full_grads and g.numel() <= 2048:
            fx["grad:" + k] = g.numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez(path, **fx)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"{name}: E {E}, T {int(r64['n_triplets'].sum())}, {size} bytes; own32 E {fx['own32:energy']:.2e} F {fx['own32:forces']:.2e} rad {fx['own32:rad']:.2e}; "
          f"own32x E {fx['own32x:energy']:.2e} F {fx['own32x:forces']:.2e} rad {fx['own32x:rad']:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_reference(a.reference)
    make(ref, "dimenet_small", D.SMALL, D.SMALL_SIZES, 0, 96, a.out, True)
    make(ref, "dimenet_yaml", D.YAML, D.YAML_SIZES, 1, 24, a.out, False)


if __name__ == "__main__":
    main()
