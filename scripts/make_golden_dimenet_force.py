#!/usr/bin/env python
"""Writes tests/golden/dimenet_force_small.npz and dimenet_force_yaml.npz: the training step WITH a force loss of the REAL reference wrapper around the restated
core (scripts/make_golden_dimenet.py explains the stand-ins; nothing of the reference is copied).

    python scripts/make_golden_dimenet_force.py --reference /path/to/nablaDFT-checkout [--out tests/golden]

The real ``DimeNetPlusPlusPotential`` and ``DimeNetPlusPlusLightning.step`` run with ``task.train()`` (the real forward takes the forces with
``create_graph=self.training``) in float64, float32 and float32 with the bases evaluated in float64, on the batches and weights of the existing fixtures
(tests/dimenet_ref: SMALL with seed 0, YAML with seed 1) and L1 losses with the coefficient pairs (energy, forces) = (1, 1) and (0, 1).

Recorded per pair ``<ce>_<cf>``: ``loss:<pair>``, ``own32:loss:<pair>`` / ``own32x:loss:<pair>`` and, per gradient tensor, ``gnorm``, ``gprobe`` (on
tests/dimenet_ref.probe_direction), ``own32`` / ``own32x`` (|g32 - g64| / |g64|; 0 where g64 is exactly zero) and, in the small case, the whole tensor where it has
at most 2048 elements; the constructor keyword names and the state_dict key list of the Lightning class.

Asserted here because the tests rely on it: everything finite; every gradient non-zero for (1, 1); ``regr_or_cls_nn.6.bias`` the only exactly-zero gradient for
(0, 1); min |F - F_target| and min |E - y| at least 20 x the float32 runs' absolute error (so the sign pattern of the L1 losses is the same in every
precision); tests/dimenet_force_ref.force_loss reproduces the real wrapper to 1e-12.
"""
import argparse
import inspect
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_dimenet import as_data, load_reference  # noqa: E402
from tests import dimenet_force_ref as FR  # noqa: E402
from tests import dimenet_ref as D  # noqa: E402


def run_real(ref, cfg, params, b, dtype, exact_basis, pair):
    torch.set_default_dtype(dtype)
    try:
        pot = ref.DimeNetPlusPlusPotential(**cfg, scaler=D.SCALER, do_postprocessing=False)
    finally:
        torch.set_default_dtype(torch.float32)
    pot = pot.to(dtype)
    pot.load_state_dict({k: v.to(dtype) for k, v in params.items()})
    pot.net.exact_basis = exact_basis
    task = ref.DimeNetPlusPlusLightning(net=pot, loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=pair[0], forces_loss_coef=pair[1])
    task.train()
    data = as_data(b, dtype)
    E, F = task.forward(data)
    assert F.grad_fn is not None
    loss = task.step(as_data(b, dtype))
    loss.backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in pot.named_parameters()}
    return dict(loss=loss.detach(), grads=grads, energy=E.detach(), forces=F.detach(), keys=list(task.state_dict().keys()))


def make(ref, name, cfg, sizes, seed, out_dir, full_grads):
    b = D.make_batch(sizes, seed + 1)
    params = D.make_params(cfg, seed)
    fx = dict(seed=np.int64(seed), sizes=np.array(sizes), pairs=np.array(FR.PAIRS),
              lightning_kwargs=np.array(list(inspect.signature(ref.DimeNetPlusPlusLightning.__init__).parameters)[1:]))
    for pair in FR.PAIRS:
        t = FR.tag(pair)
        r64 = run_real(ref, cfg, params, b, torch.float64, False, pair)
        r32 = run_real(ref, cfg, params, b, torch.float32, False, pair)
        r32x = run_real(ref, cfg, params, b, torch.float32, True, pair)
        fx["keys"] = np.array(r64["keys"])
        for r in (r64, r32, r32x):
            assert bool(torch.isfinite(r["loss"])) and all(bool(torch.isfinite(g).all()) for g in r["grads"].values())
        zero = [k for k, g in r64["grads"].items() if float(g.abs().max()) == 0.0]
        assert zero == ([] if pair == (1.0, 1.0) else ["regr_or_cls_nn.6.bias"]), (pair, zero)
        errF = max(float((r["forces"].double() - r64["forces"]).abs().max()) for r in (r32, r32x))
        errE = max(float((r["energy"].double() - r64["energy"]).abs().max()) for r in (r32, r32x))
        gapF, gapE = float((r64["forces"] - b["forces"]).abs().min()), float((r64["energy"] - b["y"]).abs().min())
        assert gapF >= 20 * errF and gapE >= 20 * errE, (name, gapF / errF, gapE / errE)
        loss, grads, _, _ = FR.force_loss(cfg, params, b, pair)          # the tests' own arithmetic == the real wrapper
        assert abs(float(loss - r64["loss"])) <= 1e-12 * abs(float(r64["loss"]))
        for k, g in r64["grads"].items():
            assert float((grads[k] - g).norm()) <= 1e-12 * max(float(g.norm()), 1e-300), k
        fx["loss:" + t] = r64["loss"].numpy()
        for tg, r in (("own32", r32), ("own32x", r32x)):
            fx[f"{tg}:loss:{t}"] = np.float64(abs(float(r["loss"]) - float(r64["loss"])) / abs(float(r64["loss"])))
            for k, g in r64["grads"].items():
                fx[f"{tg}:{t}:{k}"] = np.float64(float((r["grads"][k].double() - g).norm()) / float(g.norm()) if float(g.norm()) > 0 else 0.0)
        for k, g in r64["grads"].items():
            fx[f"gnorm:{t}:{k}"] = np.float64(float(g.norm()))
            fx[f"gprobe:{t}:{k}"] = np.float64(float((g * D.probe_direction(k, tuple(g.shape))).sum()))
            if full_grads and g.numel() <= 2048:
                fx[f"grad:{t}:{k}"] = g.numpy()
        print(f"{name} {t}: loss {float(r64['loss']):.6f}; min|F - F*| / err32 {gapF / errF:.0f}, min|E - y| / err32 {gapE / errE:.0f}; own32x loss "
              f"{fx['own32x:loss:' + t]:.2e}, worst own32x gradient {max(fx[f'own32x:{t}:{k}'] for k in r64['grads']):.2e}")
    path = os.path.join(out_dir, name + ".npz")
    np.savez(path, **fx)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"{name}: {size} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_reference(a.reference)
    make(ref, "dimenet_force_small", D.SMALL, D.SMALL_SIZES, 0, a.out, True)
    make(ref, "dimenet_force_yaml", D.YAML, D.YAML_SIZES, 1, a.out, False)


if __name__ == "__main__":
    main()
