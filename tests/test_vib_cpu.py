"""CPU: properties of the float64 numpy restatement of the normal-mode arithmetic (tests/vib_ref.py, the yardstick of tests/test_vib_gpu.py), the unit
constants, the file writers and the public surface of nabladft_amd.vibrations.  Nothing here needs a GPU; ase is not available and nothing is pinned against it."""
import inspect
import math

import numpy as np
import pytest

import vib_ref
from lbfgs_helpers import morse_np, morse_table

C12 = 12.011


def quadratic(ptr, seed):
    """Per molecule a random symmetric K and the model F = -K (x - x0): block-diagonal over the batch."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Ks = []
    for n in np.diff(ptr):
        M = rng.normal(size=(3 * n, 3 * n))
        Ks.append(M + M.T)
    return Ks


def quadratic_forces(Ks, ptr, x0):
    def forces_of(pos):
        out = np.zeros_like(pos)
        for b, K in enumerate(Ks):
            a, e = ptr[b], ptr[b + 1]
            out[a:e] = -(K @ (pos[a:e] - x0[a:e]).ravel()).reshape(-1, 3)
        return out
    return forces_of


def test_restatement_returns_the_matrix_of_a_quadratic_model():
    """F = -K (x - x0) is exactly linear, so the central difference over the REALISED step returns K to rounding; over the nominal 2 delta it is off by the
    float32 rounding of the displaced coordinate (coordinates near 8 Angstrom: ulp32 / delta ~ 1e-4)."""
    ptr = np.array([0, 3, 8, 9])
    rng = np.random.Generator(np.random.PCG64(3))
    x0 = rng.normal(size=(9, 3)) + 8.0
    Ks = quadratic(ptr, 4)
    ref = vib_ref.VibNumpy(ptr, x0, np.ones(9)).run(quadratic_forces(Ks, ptr, x0))
    nominal = vib_ref.VibNumpy(ptr, x0, np.ones(9)).run(quadratic_forces(Ks, ptr, x0), nominal=True)
    for b, K in enumerate(Ks):
        top = np.abs(K).max()
        err, err_nom = np.abs(ref.hessian[b] - K).max() / top, np.abs(nominal.hessian[b] - K).max() / top
        print(f"quadratic model, molecule {b}: realised step {err:.2e}, nominal step {err_nom:.2e}")
        assert err <= 1e-12
        assert err_nom > 1e-7                                      # the departure matters
        assert np.abs(ref.omega2[b] - np.linalg.eigvalsh(K)).max() <= 1e-11 * top


def test_fixed_atoms_give_the_partial_matrix():
    ptr = np.array([0, 4, 7])
    rng = np.random.Generator(np.random.PCG64(5))
    x0 = rng.normal(size=(7, 3))
    Ks = quadratic(ptr, 6)
    fixed = [1, 4, 5, 6]                                               # the second molecule is fully fixed
    ref = vib_ref.VibNumpy(ptr, x0, np.ones(7), fixed=fixed).run(quadratic_forces(Ks, ptr, x0))
    keep = np.array([0, 1, 2, 6, 7, 8, 9, 10, 11])
    assert ref.hessian[0].shape == (9, 9) and np.abs(ref.hessian[0] - Ks[0][np.ix_(keep, keep)]).max() <= 1e-12 * np.abs(Ks[0]).max()
    assert ref.hessian[1].shape == (0, 0) and ref.omega2[1].shape == (0,)


def test_conversion_constants():
    from nabladft_amd import md, vibrations as v
    # omega^2 = 1 Hartree / (Angstrom^2 amu): sqrt(KAPPA) is the same angular frequency in rad / fs
    assert math.isclose(v.RAD_S_PER_SQRT_UNIT, math.sqrt(md.KAPPA) * 1e15, rel_tol=1e-14)
    assert math.isclose(v.CM1_PER_SQRT_UNIT, 2720.2, rel_tol=2e-5)
    assert math.isclose(v.HARTREE_PER_SQRT_UNIT, v.HBAR_SI * math.sqrt(md.KAPPA) * 1e15 / md.E_H_SI, rel_tol=1e-14)
    # h nu / (h c): the two conversions agree through h = 2 pi hbar
    assert math.isclose(v.CM1_PER_SQRT_UNIT, v.HARTREE_PER_SQRT_UNIT * md.E_H_SI / (2.0 * math.pi * v.HBAR_SI * v.C_SI * 100.0), rel_tol=1e-14)
    assert math.isclose(v.HARTREE_TO_EV, 27.211386, rel_tol=1e-7)       # CODATA 2014
    assert (v.HBAR_SI, v.C_SI, v.E_SI) == (1.054571800e-34, 299792458.0, 1.6021766208e-19)
    e = v.energies_from_omega2([4.0, -1.0, 0.0])
    assert e.dtype == np.complex128 and e[0] == 2.0 * v.HARTREE_PER_SQRT_UNIT and e[1] == 1j * v.HARTREE_PER_SQRT_UNIT and e[2] == 0
    f = v.frequencies_from_omega2([4.0, -1.0])
    assert f[0] == 2.0 * v.CM1_PER_SQRT_UNIT and f[1].real == 0 and f[1].imag == v.CM1_PER_SQRT_UNIT
    assert np.array_equal(v.zero_point_energy(e, [0, 2, 3]), [0.5 * e[0].real, 0.0])


@pytest.fixture(scope="module")
def morse_modes():
    ptr, x0 = vib_ref.molecules(vib_ref.SIZES)
    table = morse_table(x0, ptr)                                       # pair distances of x0 are the equilibrium distances: x0 is the minimum
    return vib_ref.VibNumpy(ptr, x0, np.full(len(x0), C12)).run(lambda p: morse_np(p, table)[0])


def test_near_zero_modes_at_the_morse_minimum(morse_modes):
    for n, w, H in zip(vib_ref.SIZES, morse_modes.omega2, morse_modes.hessian):
        k, gap = vib_ref.count_near_zero(w)
        print(f"{n} atoms: {k} near-zero modes, next at {gap:.3e} of the largest")
        if n == 1:
            assert k == 3 and not H.any()
            continue
        assert k == (5 if n == 2 else 6)
        assert gap > 1e-2


def test_a_collinear_molecule_has_five_zero_modes():
    ptr, x0, table = vib_ref.collinear_molecule()
    assert np.abs(morse_np(x0, table)[0]).max() < 1e-14               # a stationary point
    ref = vib_ref.VibNumpy(ptr, x0, np.full(3, C12)).run(lambda p: morse_np(p, table)[0])
    k, gap = vib_ref.count_near_zero(ref.omega2[0])
    assert k == 5 and gap > 1e-2


def test_jacobi_emulation_meets_the_bound_the_kernel_is_held_to():
    """The scheme the kernel implements (ordering, phases, stopping rule), emulated in numpy: within 10 m eps of np.linalg.eigh, at most 30 sweeps."""
    rng = np.random.Generator(np.random.PCG64(9))
    for m in (3, 6, 9, 42):
        M = rng.normal(size=(m, m))
        for A in (M + M.T, np.zeros((m, m)), np.diag(rng.normal(size=m))):
            w, V, sweeps, status = vib_ref.jacobi(A)
            errs = vib_ref.eig_errors(A, w, V)
            assert status == 0 and sweeps <= 30 and max(errs) <= 10.0, (m, sweeps, errs)


def test_file_writers_round_trip(tmp_path):
    from nabladft_amd import vibrations as v
    from nabladft_amd.md import read_xyz
    dof_ptr = np.array([0, 6, 9])
    omega2 = np.array([-1e-4, 0.0, 1e-6, 0.01, 0.02, 0.03, -0.5, 0.25, 1.0])
    energies = v.energies_from_omega2(omega2)
    path = str(tmp_path / "modes.txt")
    v.write_summary(path, energies, dof_ptr)
    back = v.read_summary(path)
    assert [len(b[0]) for b in back] == [6, 3]
    mev = 1000.0 * v.HARTREE_TO_EV * energies
    cm = v.frequencies_from_omega2(omega2)
    for (a, e), (got_mev, got_cm, zpe) in zip(zip(dof_ptr[:-1], dof_ptr[1:]), back):
        assert np.abs(got_mev - mev[a:e]).max() <= 0.05 + 1e-9 and np.abs(got_cm - cm[a:e]).max() <= 0.05 + 1e-9      # one decimal is written
        assert (got_mev.imag != 0).tolist() == (omega2[a:e] < 0).tolist()
        assert abs(zpe - v.HARTREE_TO_EV * 0.5 * energies[a:e].real.sum()) <= 5e-4
    lines = open(path).read().splitlines()
    assert lines[0] == "# molecule 0" and lines[2].split() == ["#", "meV", "cm^-1"] and lines[-1].startswith("Zero-point energy:")
    # one frame per mode; fixed atoms carry a zero displacement
    z, ptr = np.array([8, 1, 1, 6]), np.array([0, 3, 4])
    pos = np.arange(12, dtype=np.float64).reshape(4, 3)
    free = np.array([True, False, True, True])
    hess_ptr = np.array([0, 36, 45])
    modes = np.random.Generator(np.random.PCG64(2)).normal(size=45)
    xyz = str(tmp_path / "modes.xyz")
    v.write_jmol(xyz, z, ptr, pos, cm, modes, dof_ptr, hess_ptr, free)
    frames = read_xyz(xyz)
    assert [len(f[0]) for f in frames] == [3] * 6 + [1] * 3
    assert np.array_equal(frames[0][0], [8, 1, 1]) and np.abs(frames[0][1] - pos[:3]).max() < 1e-5
    text = open(xyz).read().splitlines()
    assert text[1] == "Mode #0, f = %.1fi cm^-1." % cm[0].imag and text[1 + 5 * 3].startswith("Mode #3, f = ")
    row = np.array([float(t) for t in text[3].split()[4:]])            # the fixed atom of frame 0
    assert not row.any()
    row = np.array([float(t) for t in text[4].split()[4:]])
    assert np.abs(row - modes[3:6]).max() < 1e-5


def test_public_names_and_signatures():
    import nabladft_amd as nq
    from nabladft_amd import optimization, vibrations
    assert nq.BatchedVibrations is vibrations.BatchedVibrations is optimization.BatchedVibrations
    assert "BatchedVibrations" in nq.__all__ and "BatchedVibrations" in optimization.__all__
    p = inspect.signature(nq.BatchedVibrations.__init__).parameters
    assert list(p)[1:6] == ["calculator", "delta", "fixed_atoms_mask", "masses", "images_per_call"]
    assert (p["delta"].default, p["fixed_atoms_mask"].default, p["masses"].default) == (0.01, None, None) and p["images_per_call"].default >= 2
    assert list(inspect.signature(nq.BatchedVibrations.run).parameters)[1:] == ["batch"]
    for name in ("hessian", "omega2", "modes", "asymmetry", "sweeps", "energies", "frequencies", "zero_point_energy"):
        assert isinstance(getattr(nq.BatchedVibrations, name), property), name
    assert list(inspect.signature(nq.PYGAseInterface.compute_normal_modes).parameters) == ["self", "write_jmol"]
    assert inspect.signature(nq.PYGAseInterface.compute_normal_modes).parameters["write_jmol"].default is True
    calc = optimization.PyGBatchwiseCalculator(lambda b: None, "cpu", energy_unit="Hartree", position_unit="Ang")
    with pytest.raises(NotImplementedError):
        nq.BatchedVibrations(calc, nfree=4)
    with pytest.raises(NotImplementedError):
        optimization.PyGBatchwiseCalculator(lambda b: None, "cpu", energy_unit="eV", position_unit="Ang")
    with pytest.raises(ValueError):
        nq.BatchedVibrations(calc, delta=0.0)
    assert vibrations.MAX_DOF == 576 and vibrations.LDS_MAX_DOF == 141


def test_plan_and_chunks_agree_with_the_restatement():
    from nabladft_amd import vibrations as v
    ptr = np.array([0, 3, 8, 9, 12])
    fixed = [1, 8, 9, 10, 11]
    pl, ref = v.plan(ptr, fixed), vib_ref.plan(ptr, fixed)
    assert np.array_equal(pl["dof_ptr"], ref["dof_ptr"]) and np.array_equal(pl["hess_ptr"], ref["hess_ptr"])
    assert pl["m"].tolist() == [6, 15, 0, 0] and pl["D"] == 21 and pl["P"] == 36 + 225
    assert np.array_equal(pl["disp_mol"], [b for b, _, _ in ref["disp"]])
    assert np.array_equal(np.repeat(pl["free_atom"], 3), [a for _, a, _ in ref["disp"]])
    assert np.array_equal(np.diff(pl["disp_off"]), [2 * (ptr[b + 1] - ptr[b]) for b, _, _ in ref["disp"]])
    ch = v.chunks(pl, 8)
    assert ch[0] == (0, 4) and ch[-1][1] == 21 and all(a[1] == b[0] for a, b in zip(ch[:-1], ch[1:])) and max(c1 - c0 for c0, c1 in ch) == 4
    assert v.chunks(pl, 3) == [(j, j + 1) for j in range(21)]           # an odd budget never splits a pair
    mask = np.zeros(12, dtype=bool)
    mask[fixed] = True
    assert np.array_equal(v.plan(ptr, mask)["free_atom"], pl["free_atom"])
