"""CPU: the unit table and the mass table of nabladft_amd/md.py, properties of the float64 numpy restatement the MD kernels are tested against
(tests/md_ref.py), the numpy Philox4x32-10, and the public surface of ``PYGAseInterface`` / ``BatchedMD`` against a literal list typed from
nablaDFT/optimization/pyg_ase_interface.py."""
import ctypes as C
import inspect

import numpy as np
import pytest

import md_ref
from lbfgs_helpers import morse_np, morse_table
from md_ref import MDNumpy


def test_constants_recomputed_from_the_si_inputs():
    """KAPPA = E_h fs^2 / (amu Angstrom^2), KB = k / E_h from CODATA 2014, recomputed here in exact rational arithmetic from the decimal SI values."""
    from fractions import Fraction
    e_h, amu, k = Fraction("4.359744650e-18"), Fraction("1.660539040e-27"), Fraction("1.38064852e-23")
    kappa = float(e_h * Fraction(10) ** -30 / (amu * Fraction(10) ** -20))
    kb = float(k / e_h)
    assert abs(kappa - 0.26255) < 1e-5 and abs(kb - 3.16681e-6) < 1e-11
    # the float64 evaluation may round each of its four operations: a few units in the last place
    assert abs(md_ref.KAPPA - kappa) <= 4 * np.spacing(kappa) and abs(md_ref.KB - kb) <= 4 * np.spacing(kb)


def test_package_constants_match_and_reach_the_library():
    from nabladft_amd import _lib, md
    from nabladft_amd.build import build
    build(verbose=False)
    assert md.KAPPA == md_ref.KAPPA and md.KB == md_ref.KB
    out = (C.c_double * 2)()
    assert _lib.load().nq_md_constants(out) == 0
    assert out[0] == md.KAPPA and out[1] == md.KB


def test_mass_table_refuses_unknown_z():
    from nabladft_amd.md import masses_for
    m = masses_for(np.array([1, 6, 7, 8, 9, 16, 17, 35]))
    assert np.allclose(m, [1.008, 12.011, 14.007, 15.999, 18.998403163, 32.06, 35.45, 79.904])
    for bad in ([0], [37], [6, 53]):
        with pytest.raises(ValueError):
            masses_for(np.array(bad))
    assert np.array_equal(masses_for(np.array([6, 53]), masses=[12.0, 126.9]), [12.0, 126.9])
    with pytest.raises(ValueError):
        masses_for(np.array([6, 53]), masses=[12.0])


def _morse_system(n=42, seed=3):
    x0 = md_ref.lattice_molecule(n, seed)
    ptr = np.array([0, n])
    rng = np.random.Generator(np.random.PCG64(seed))
    masses = rng.choice([1.008, 12.011, 15.999], size=n)
    return ptr, masses, x0, morse_table(x0 + rng.normal(0.0, 0.05, size=x0.shape), ptr)


def _run(md, table, steps, dt):
    for _ in range(steps):
        md.launch(morse_np(md.x, table)[0], 0, dt)
    md.launch(morse_np(md.x, table)[0], 0, dt, finish_only=True)


def test_velocity_verlet_is_time_reversible():
    """K steps, v -> -v, K steps: the map is its own inverse in exact arithmetic, so only rounding remains.  Bound: every step rounds x at |x| eps / 2 and
    v dt at the same scale, 2 K steps, and a bounded orbit of this stiffness (omega dt ~ 0.05) amplifies a perturbation by a small factor, taken as 10."""
    ptr, masses, x0, table = _morse_system()
    K, dt = 50, 0.5
    md = MDNumpy(ptr, masses, x0)
    zeta = np.random.Generator(np.random.PCG64(1)).normal(size=x0.shape)
    md.init_velocities(zeta, md_ref.KB * 300.0)
    _run(md, table, K, dt)
    assert np.abs(md.x - x0).max() > 1e-3                     # it moved
    md.v = -md.v
    _run(md, table, K, dt)
    bound = 10 * 2 * K * 2 * np.abs(x0).max() * 2.0 ** -53
    err = np.abs(md.x - x0).max()
    print(f"return error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_langevin_without_friction_and_noise_is_nve():
    """fr = 0: sigma = 0, c1 = dt / 2, c2 = 0, rnd = 0, and v = (x' - x) / dt reproduces the half-kicked velocity up to the rounding of x' (|x| eps / dt)."""
    ptr, masses, x0, v0 = md_ref.random_system([5, 17], 2)
    rng = np.random.Generator(np.random.PCG64(4))
    a, b = MDNumpy(ptr, masses, x0, v0), MDNumpy(ptr, masses, x0, v0)
    steps, dt = 6, 0.5
    for _ in range(steps):
        f = rng.normal(0.0, 0.05, size=x0.shape)
        xi, eta = rng.normal(size=x0.shape), rng.normal(size=x0.shape)
        a.launch(f, 0, dt)
        b.launch(f, 1, dt, md_ref.KB * 300.0, 0.0, xi, eta)
    eps_x = np.abs(x0).max() * 2.0 ** -52
    assert np.abs(a.x - b.x).max() <= 4 * steps * eps_x and np.abs(a.v - b.v).max() <= 4 * steps * eps_x / dt
    assert np.abs(a.x - x0).max() > 1e-3


def test_stationary_and_zero_rotation():
    sizes = [1, 2, 3, 40]
    ptr, masses, x0, _ = md_ref.random_system(sizes, 6)
    md = MDNumpy(ptr, masses, x0)
    md.init_velocities(np.random.Generator(np.random.PCG64(2)).normal(size=x0.shape), md_ref.KB * 300.0)
    o = md.observables()
    scale_p = md.seg(md.m * np.abs(md.v)).max() + 1e-300
    assert np.isfinite(md.v).all()
    # sums of n terms, each rounded at eps: n eps x the sum of magnitudes bounds the residual
    assert (o["p_norm"] <= 64 * 2.0 ** -52 * scale_p).all()
    d = np.abs(md.x - md.atoms(md.seg(md.m * md.x) / md.seg(md.m))).max()
    assert (o["l_norm"][2:] <= 1000 * 2.0 ** -52 * scale_p * d).all()           # non-linear: 3 and 40 atoms
    assert np.abs(md.v[ptr[1]:ptr[2]]).max() > 0.0                               # the diatomic keeps its vibration
    assert np.abs(md.v[0]).max() <= 4 * 2.0 ** -52 * np.sqrt(md_ref.KAPPA * md_ref.KB * 300.0 / masses[0])      # a single atom is at rest after Stationary, up to the rounding of (m v) / m
    # without the two removals the temperature estimate is the plain Maxwell-Boltzmann one
    md.init_velocities(np.ones_like(x0), md_ref.KB * 300.0, False, False)
    assert np.allclose(md.observables()["temperature"], 300.0, rtol=1e-12)


def test_fixed_atoms_do_not_move():
    ptr, masses, x0, v0 = md_ref.random_system([9], 8)
    md = MDNumpy(ptr, masses, x0, v0, fixed=[0, 4])
    rng = np.random.Generator(np.random.PCG64(9))
    for mode in (0, 1):
        for _ in range(3):
            md.launch(rng.normal(0.0, 0.05, size=x0.shape), mode, 0.5, md_ref.KB * 300.0, 0.01, rng.normal(size=x0.shape), rng.normal(size=x0.shape))
            assert np.array_equal(md.x[[0, 4]], x0[[0, 4]]) and not md.v[[0, 4]].any()
        md.launch(rng.normal(0.0, 0.05, size=x0.shape), mode, 0.5, md_ref.KB * 300.0, 0.01, finish_only=True)
    assert md.observables()["temperature"][0] > 0 and md.step == 6


def test_numpy_philox_known_answers_and_normal_layout():
    """Philox4x32-10 known answers of the Random123 distribution (counter / key all zero, all ones), and the draw layout of md_ref.normals."""
    z = np.zeros(1, dtype=np.uint64)
    assert [int(w[0]) for w in md_ref.philox4x32(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    assert [int(w[0]) for w in md_ref.philox4x32(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    ptr = np.array([0, 3, 10])
    xi, eta = md_ref.normals(7, 5, 0, ptr), md_ref.normals(7, 5, 1, ptr)
    assert np.isfinite(xi).all() and not np.array_equal(xi, eta)
    # the counter holds the molecule's key, not its place in the batch
    assert np.array_equal(md_ref.normals(7, 5, 0, np.array([0, 7]), mol_key=[1]), xi[3:])
    assert not np.array_equal(md_ref.normals(8, 5, 0, ptr), xi) and not np.array_equal(md_ref.normals(7, 6, 0, ptr), xi)


# pyg_ase_interface.py:136-150 (constructor), :183, :194, :207-215, :265-270, :284, :296, :317: typed from the reference, not imported from it
REFERENCE_INIT = ["molecule_path", "working_dir", "config", "model", "energy_key", "force_key", "energy_unit", "position_unit", "device", "dtype", "optimizer_class",
                  "fixed_atoms"]
REFERENCE_METHODS = {"save_molecule": ["name", "file_format", "append"], "calculate_single_point": [],
                     "init_md": ["name", "time_step", "temp_init", "temp_bath", "reset", "interval"],
                     "_init_velocities": ["temp_init", "remove_translation", "remove_rotation"], "run_md": ["steps"], "optimize": ["fmax", "steps"],
                     "compute_normal_modes": ["write_jmol"]}
REFERENCE_DEFAULTS = {"energy_key": "energy", "force_key": "forces", "energy_unit": "Hartree", "position_unit": "Angstrom", "device": "cpu", "fixed_atoms": None}


def test_public_surface_matches_the_reference_names():
    import nabladft_amd as nq
    from nabladft_amd import optimization
    assert nq.PYGAseInterface is optimization.PYGAseInterface and nq.BatchedMD is nq.md.BatchedMD
    assert "PYGAseInterface" in nq.__all__ and "BatchedMD" in nq.__all__ and "PYGAseInterface" in optimization.__all__
    sig = inspect.signature(nq.PYGAseInterface.__init__)
    names = [p for p in sig.parameters if p != "self"]
    assert names[:len(REFERENCE_INIT)] == REFERENCE_INIT
    for k, v in REFERENCE_DEFAULTS.items():
        assert sig.parameters[k].default == v, k
    for meth, args in REFERENCE_METHODS.items():
        got = [p for p in inspect.signature(getattr(nq.PYGAseInterface, meth)).parameters if p != "self"]
        assert got == args, meth
    d = {k: p.default for k, p in inspect.signature(nq.PYGAseInterface.init_md).parameters.items()}
    assert (d["time_step"], d["temp_init"], d["temp_bath"], d["reset"], d["interval"]) == (0.5, 300, None, False, 1)
    b = inspect.signature(nq.BatchedMD.__init__).parameters
    assert list(b)[1:12] == ["calculator", "time_step", "temp_bath", "friction", "fixed_atoms_mask", "masses", "seed", "interval", "frames", "store_velocities",
                             "check_every"]
    assert (b["time_step"].default, b["temp_bath"].default, b["friction"].default, b["interval"].default, b["frames"].default) == (0.5, None, 0.01, 1, None)
    assert [p for p in inspect.signature(nq.BatchedMD.init_velocities).parameters][1:] == ["batch", "temp_init", "remove_translation", "remove_rotation"]
    assert [p for p in inspect.signature(nq.BatchedMD.run).parameters][1:] == ["batch", "steps"]


def test_interface_reads_xyz_and_refuses_units_and_normal_modes(tmp_path):
    import nabladft_amd as nq
    from nabladft_amd.md import read_xyz, write_xyz
    z = np.array([8, 1, 1, 6, 1, 1, 1, 1])
    ptr = np.array([0, 3, 8])
    pos = np.random.Generator(np.random.PCG64(0)).normal(size=(8, 3))
    path = str(tmp_path / "two.xyz")
    write_xyz(path, z, ptr, pos)
    mols = read_xyz(path)
    assert [len(m[0]) for m in mols] == [3, 5] and np.array_equal(np.concatenate([m[0] for m in mols]), z)
    assert np.abs(np.concatenate([m[1] for m in mols]) - pos).max() < 1e-11
    model = lambda batch: None
    it = nq.PYGAseInterface(path, str(tmp_path / "work"), None, model, fixed_atoms=[0])
    assert np.array_equal(it.ptr, ptr) and np.array_equal(np.nonzero(it.fixed_mask)[0], [0, 3])
    it.save_molecule("copy", "extxyz")
    assert [len(m[0]) for m in read_xyz(str(tmp_path / "work" / "copy.extxyz"))] == [3, 5]
    with pytest.raises(NotImplementedError):
        it.compute_normal_modes()
    with pytest.raises(AttributeError):
        it.run_md(3)
    for kw in (dict(energy_unit="kcal/mol"), dict(energy_unit="eV"), dict(position_unit="Bohr")):
        with pytest.raises(NotImplementedError):
            nq.PYGAseInterface(path, str(tmp_path / "work"), None, model, **kw)
    with pytest.raises(RuntimeError, match="MI355X only"):       # no CPU fallback
        it.init_md("md")
