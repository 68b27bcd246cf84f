"""CONTAINER-ONLY: records what the *real* reference optimiser (nablaDFT/optimization/optimizers.py, ASEBatchwiseLBFGS without line search) does, as fixtures
tests/golden/lbfgs_{A,B,C,D}*.npz.  Nothing of the reference is copied: the module is imported from the reference checkout given by --reference (the way
oracle/ref_import.py does) behind small stand-ins, all our own code, for the packages that are not installed: ase (Atoms, io.write, optimize.optimize.Dynamics,
parallel.barrier / world), schnetpack (interfaces.ase_interface, units.convert_units) and torch_geometric.data.

    python scripts/make_golden_lbfgs.py --reference /path/to/reference [--cases A,B,C,D]

Cases (tests/test_optimization_cpu.py, tests/test_optimization_gpu.py):
  A  seven molecules (5, 17, 42, 64, 90, 3, 130 atoms), Morse potential (tests/lbfgs_helpers.py), fmax 1e-5, memory 100, free-running until converged
  B  the same start, memory 5, maxstep 0.04, 60 steps: ring wrap and clamping
  C  a 320-atom and a 12-atom molecule, five fixed atoms, memory 20, 40 steps: the workgroup-per-molecule path
  D  the reference class driven by oracle/painn_ref.energy_forces on the smoke test's four molecules, float64 and float32, 10 steps each
For A-C the reference also runs on the same batch with the atoms permuted inside each molecule (summation order only); ``reorder_spread`` = the largest position
difference after un-permuting, the yardstick of the tests' tolerances.  Asserted here: at every recorded step every molecule's max |f|^2 is at least 1e-6
(relative) away from fmax^2, so rounding cannot flip a convergence decision (change the seed if it fails, not the tests).
The recorded per-molecule ``mask`` is computed here, from the forces the reference's step sees and with its formula (optimizers.py:462-468): the reference
keeps that mask in a local variable.  It is pinned to the reference indirectly, through the recorded r_{k+1} in which masked molecules do not move.
The geometries are compact jittered grids, not drug-like trees: with pairs below 3 A only, tree-shaped molecules have floppy modes and the reference needs
about 250 steps, too many for a fixture of committable size.  On the grids case A converges in 32 steps (4 normalisations) and case B, memory 5 and maxstep
0.04, converges at step 32 with 38 normalisations (counted per molecule): the ring wraps and the clamp fires, but B does not run its 60 steps unconverged.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lbfgs_helpers as H  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LIMIT = 1 << 20


# ---- stand-ins ----------------------------------------------------------------------------------------------------------------------------
class Atoms:
    def __init__(self, positions=None, numbers=None, pbc=False, cell=None):
        self.positions = np.array(positions, dtype=np.float64)
        self.numbers = np.array(numbers)
        self.pbc, self.cell = pbc, cell

    def get_positions(self):
        return self.positions.copy()

    def get_atomic_numbers(self):
        return self.numbers.copy()

    def copy(self):
        return Atoms(self.positions, self.numbers, self.pbc, self.cell)

    def __len__(self):
        return len(self.numbers)

    def __eq__(self, other):
        return np.array_equal(self.positions, other.positions) and np.array_equal(self.numbers, other.numbers)

    __hash__ = None


class Dynamics:
    def __init__(self, atoms, logfile=None, trajectory=None, append_trajectory=False, master=None):
        self.atoms, self.logfile, self.nsteps, self.max_steps = atoms, None, 0, 100000000


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference(root):
    world = types.SimpleNamespace(rank=0, size=1)
    _mod("ase", Atoms=Atoms)
    _mod("ase.io", write=lambda *a, **k: None)
    _mod("ase.optimize")
    _mod("ase.optimize.optimize", Dynamics=Dynamics)
    _mod("ase.parallel", barrier=lambda: None, world=world)
    _mod("schnetpack")
    _mod("schnetpack.interfaces")
    _mod("schnetpack.interfaces.ase_interface", AtomsConverter=object, AtomsConverterError=RuntimeError)
    _mod("schnetpack.units", convert_units=lambda a, b: 1.0)
    _mod("torch_geometric")
    _mod("torch_geometric.data", Batch=object, Data=object)
    pkg = _mod("nablaDFT")
    pkg.__path__ = [os.path.join(root, "nablaDFT")]
    opt = _mod("nablaDFT.optimization")
    opt.__path__ = [os.path.join(root, "nablaDFT", "optimization")]
    return importlib.import_module("nablaDFT.optimization.optimizers"), importlib.import_module("nablaDFT.optimization.calculator")


def make_calculator(calc_mod, fn):
    """The reference's BatchwiseCalculator (get_forces with its fixed-atom zeroing, result caching) around ``fn(positions) -> (forces, energy)``."""

    class Calc(calc_mod.BatchwiseCalculator):
        def __init__(self):
            self.results, self.atoms = None, None
            self.energy_key, self.force_key = "energy", "forces"

        def calculate(self, atoms):
            forces, energy = fn(np.concatenate([a.get_positions() for a in atoms]))
            self.results = {"energy": energy, "forces": forces}
            self.atoms = [a.copy() for a in atoms]

    return Calc()


def run_reference(ref, fn, pos, z, ptr, fmax, steps, fixed=None, **kw):
    """-> dict of the recorded run: r [K+1, N, 3], f [K+1, N, 3] (forces at every r), mask [K, B], nnorm [K] (cumulative), rho [L, B], nsteps, converged."""
    opt_mod, calc_mod = ref
    calc = make_calculator(calc_mod, fn)
    opt = opt_mod.ASEBatchwiseLBFGS(calc, logfile=None, fixed_atoms_mask=fixed, **kw)
    atoms = [Atoms(pos[a:b], z[a:b]) for a, b in zip(ptr[:-1], ptr[1:])]
    rec = {"r": [], "f": [], "mask": [], "nnorm": []}
    inner = opt.step
    cat = lambda: np.concatenate([a.get_positions() for a in opt.atoms])

    def step(f=None):
        r = cat()
        fk = np.array(calc.get_forces(opt.atoms, fixed_atoms_mask=fixed), dtype=np.float64)
        m2 = np.maximum.reduceat((fk ** 2).sum(1), ptr[:-1])
        assert (np.abs(m2 - fmax ** 2) >= 1e-6 * fmax ** 2).all(), "a molecule sits on the convergence threshold: change the seed"
        rec["r"].append(r), rec["f"].append(fk), rec["mask"].append(m2 < fmax ** 2)
        inner(f)
        rec["nnorm"].append(opt.n_normalizations)

    opt.step = step
    converged = bool(opt.run(atoms, fmax=fmax, steps=steps))
    rec["r"].append(cat())
    ff = np.array(calc.get_forces(opt.atoms, fixed_atoms_mask=fixed), dtype=np.float64)
    rec["f"].append(ff)
    m2 = np.maximum.reduceat((ff ** 2).sum(1), ptr[:-1])
    assert (np.abs(m2 - fmax ** 2) >= 1e-6 * fmax ** 2).all(), "the final forces sit on the convergence threshold: change the seed"
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(rho=np.array(opt.rho, dtype=np.float64), nsteps=opt.nsteps, converged=converged, energy=calc.results["energy"])
    return out


def save(name, **arrays):
    path = os.path.join(GOLDEN, name)
    np.savez(path, **arrays)
    size = os.path.getsize(path)
    assert size < LIMIT, (name, size)
    print(f"  wrote {name}: {size} bytes")


def cloud(rng, n, spacing=1.6, jitter=0.15):
    """A compact random geometry: the n sites of a cubic grid nearest to its centre, jittered, in random order (about 25 neighbours within 3 A: no floppy modes,
    so the reference converges in tens of steps and the recorded trajectory stays small)."""
    m = int(np.ceil(n ** (1 / 3))) + 2
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    g = g[np.argsort(((g - (m - 1) / 2) ** 2).sum(1), kind="stable")][:n]
    return (g * spacing + rng.normal(0.0, jitter, size=(n, 3)))[rng.permutation(n)]


def batch_of(rng, sizes):
    return np.concatenate([cloud(rng, n) for n in sizes]), np.ones(sum(sizes), dtype=np.int64), np.concatenate([[0], np.cumsum(sizes)])


def morse_case(ref, name, sizes, seed, fmax, steps, fixed=None, **kw):
    print(f"case {name}")
    rng = np.random.Generator(np.random.PCG64(seed))
    ref_pos, z, ptr = batch_of(rng, sizes)
    start = ref_pos + rng.normal(0.0, 0.08, size=ref_pos.shape)
    table = H.morse_table(ref_pos, ptr)
    run = run_reference(ref, lambda p: H.morse_np(p, table, ptr), start, z, ptr, fmax, steps, fixed=fixed, **kw)
    # the same batch with the atoms permuted inside each molecule
    perm = np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    ptable = H.permute_table(table, perm)
    prun = run_reference(ref, lambda p: H.morse_np(p, ptable, ptr), start[perm], z[perm], ptr, fmax, steps, fixed=None if fixed is None else sorted(inv[fixed].tolist()), **kw)
    assert prun["nsteps"] == run["nsteps"] and prun["converged"] == run["converged"] and np.array_equal(prun["mask"], run["mask"])
    spread = float(np.abs(prun["r"][:, inv] - run["r"]).max())
    fin = np.sqrt((run["f"][-1] ** 2).sum(1).max())
    print(f"  nsteps {run['nsteps']} converged {run['converged']} normalisations {int(run['nnorm'][-1])} final max force {fin:.3e} reorder_spread {spread:.3e}")
    print(f"  molecules first converged at steps {[int(np.argmax(run['mask'][:, b])) if run['mask'][:, b].any() else -1 for b in range(len(sizes))]}")
    meta = dict(ptr=ptr, z=z, nbr=table[0], d0=table[1], nbr_mask=table[2], mask=run["mask"], nnorm=run["nnorm"], rho=run["rho"], nsteps=run["nsteps"],
                converged=run["converged"], reorder_spread=spread, fmax=fmax, steps=steps, memory=kw.get("memory", 100), maxstep=kw.get("maxstep", 0.2),
                fixed=np.array([] if fixed is None else fixed, dtype=np.int64), energy=run["energy"])
    save(f"lbfgs_{name}.npz", r=run["r"], **meta)
    save(f"lbfgs_{name}_forces.npz", f=run["f"])


def painn_case(ref):
    print("case D")
    from oracle import painn_ref as R
    cfg = R.PaiNNConfig(hidden_channels=64, num_layers=2, num_rbf=20, cutoff=5.0, max_neighbors=100)
    params = R.make_params(cfg, seed=3)
    pos, z, batch, _, _ = R.gen_conformers(11, 4, size=(8, 20))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(batch.numpy()))])
    runs = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        P = {k: v.to(dt) for k, v in params.items()}
        energies = []

        def fn(p):
            e, f = R.energy_forces(P, cfg, torch.from_numpy(p).to(dt), z, batch)       # .float() of atoms_list_to_PYG in the float32 run
            energies.append(e.double().numpy())
            return f.numpy(), e.numpy()

        runs[tag] = run_reference(ref, fn, pos.double().numpy(), z.numpy(), ptr, 0.05, 10)
        runs[tag]["e_start"], runs[tag]["e_end"] = energies[0], runs[tag]["energy"].astype(np.float64)
    a, b = runs["f64"], runs["f32"]
    own = np.abs(a["r"] - b["r"]).reshape(a["r"].shape[0], -1).max(1)
    print("  own_spread", " ".join(f"{v:.2e}" for v in own))
    print("  energies", a["e_start"], "->", a["e_end"], "steps", a["nsteps"], b["nsteps"])
    assert (a["e_end"] < a["e_start"]).all()
    save("lbfgs_D.npz", ptr=ptr, r64=a["r"], r32=b["r"], f64=a["f"], e_start=a["e_start"], e_end=a["e_end"], e_end32=b["e_end"], own_spread=own,
         nnorm=a["nnorm"], nsteps=a["nsteps"], fmax=0.05, steps=10)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--cases", default="A,B,C,D")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    cases = args.cases.split(",")
    sizes = [5, 17, 42, 64, 90, 3, 130]
    if "A" in cases:
        morse_case(ref, "A", sizes, 101, 1e-5, 500)
    if "B" in cases:
        morse_case(ref, "B", sizes, 101, 1e-5, 60, memory=5, maxstep=0.04)
    if "C" in cases:
        morse_case(ref, "C", [320, 12], 303, 1e-3, 40, fixed=[0, 7, 100, 319, 325], memory=20)
    if "D" in cases:
        painn_case(ref)
