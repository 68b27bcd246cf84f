"""Writes tests/golden/vib_painn.npz: the normal-mode restatement (tests/vib_ref.py) driven by the float64 PaiNN of oracle/painn_ref.energy_forces on the two
molecules tests/test_vib_gpu.py sends through ``PYGAseInterface.compute_normal_modes``.  Runs on a host without a GPU:

    python scripts/make_golden_vib.py

Recorded: ``z``, ``ptr``, ``pos`` (float32: what the interface's .xyz file holds), ``hess_ptr`` / ``dof_ptr``, the packed float64 ``hessian`` and ``omega2``
(forces of the float64 model at the float32 image positions), and ``spread_hessian`` / ``spread_omega2``: the largest deviation of the same restatement driven
by the float32 model (float32 parameters, positions and forces) -- the yardstick of the test's tolerance (10 x the spread).  ase is not involved.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vib_ref  # noqa: E402
from oracle import painn_ref as R  # noqa: E402

CFG = dict(hidden_channels=64, num_layers=2, num_rbf=20, cutoff=5.0, max_neighbors=100)
CONFORMER_SEED, PARAM_SEED, SIZE = 11, 3, (10, 20)


def main():
    from nabladft_amd.md import masses_for
    cfg = R.PaiNNConfig(**CFG)
    pos, z, batch, _, _ = R.gen_conformers(CONFORMER_SEED, 2, size=SIZE)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(batch.numpy()))])
    masses = masses_for(z.numpy())
    legs = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        P = R.make_params(cfg, seed=PARAM_SEED, dtype=dtype)

        def forces_of(p, dtype=dtype, P=P):
            return R.energy_forces(P, cfg, torch.from_numpy(p).to(dtype), z, batch)[1].numpy()

        legs[name] = vib_ref.VibNumpy(ptr, pos.double().numpy(), masses).run(forces_of, cast=np.float64 if name == "f64" else np.float32)
        print(name, "asymmetry", [f"{a:.2e}" for a in legs[name].asymmetry], "lowest omega2", [f"{w[0]:.3e}" for w in legs[name].omega2])
    a, b = legs["f64"], legs["f32"]
    spread_h = max(np.abs(x - y).max() for x, y in zip(a.hessian, b.hessian))
    spread_w = max(np.abs(x - y).max() for x, y in zip(a.omega2, b.omega2))
    print(f"float32-versus-float64 spread: hessian {spread_h:.3e} (largest entry {max(np.abs(x).max() for x in a.hessian):.3e}), omega2 {spread_w:.3e}")
    out = os.path.join(ROOT, "tests", "golden", "vib_painn.npz")
    np.savez(out, z=z.numpy(), ptr=ptr, pos=pos.numpy(), cfg=np.array(sorted(CFG.items()), dtype=object).astype(str), param_seed=PARAM_SEED,
             hess_ptr=a.pl["hess_ptr"], dof_ptr=a.pl["dof_ptr"], hessian=np.concatenate([h.ravel() for h in a.hessian]), omega2=np.concatenate(a.omega2),
             spread_hessian=spread_h, spread_omega2=spread_w)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
