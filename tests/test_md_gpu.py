"""GPU: the device-resident batched MD (csrc/md.hip through the C ABI and through nabladft_amd.md) against the float64 numpy restatement (tests/md_ref.py,
whose properties tests/test_md_cpu.py pins) and against physical invariants.  ase is not available: nothing here is pinned against ase.

Tolerance rule (that of the L-BFGS tests): 1000 x the restatement's own spread, floor 1e-13 in the units of the compared quantity (Angstrom, Angstrom/fs).
The spread is the larger deviation of two re-evaluations of the restatement on the same inputs: atoms summed in a permuted order, and np.longdouble
(md_ref.spread_and_tolerance).  Measured on an MI355X (profiles/md_parity.txt): NVE has no per-molecule sum on the path to r and v, so its permuted spread is
exactly 0 and the floor applies; Langevin's spreads are of the order of 1e-15."""
import os

import numpy as np
import pytest
import torch

import md_ref
from lbfgs_helpers import morse_np, morse_table, morse_torch
from md_ref import KB, MDNumpy, SIZES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = {"b1": [193], "b5": [2, 64, 193, 3, 512], "sizes9": SIZES}
DT, T_BATH, FR = 0.5, 300.0, 0.01


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def new_state(ptr, x0, masses, v0=None, fixed=None, **kw):
    from nabladft_amd.md import MDState
    return MDState(ptr, dev(x0), masses, fixed, velocities=None if v0 is None else dev(v0), **kw)


def teacher_case(sizes, mode, with_fixed, seed=1, steps=8):
    ptr, masses, x0, v0 = md_ref.random_system(sizes, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 100))
    N = int(ptr[-1])
    forces = rng.normal(0.0, 0.05, size=(steps, N, 3))
    xi = rng.normal(size=(steps, N, 3)) if mode else None
    eta = rng.normal(size=(steps, N, 3)) if mode else None
    fixed = np.unique(np.concatenate([ptr[:-1], rng.integers(0, N, size=max(1, N // 7))])) if with_fixed else None      # first atom of every molecule + a seventh
    return ptr, masses, x0, v0, forces, xi, eta, fixed


@pytest.fixture(scope="module")
def tol1():
    """Test 1's tolerance for the plain NVE case on the nine sizes: what tests 3 and 8 refer to."""
    ptr, masses, x0, v0, forces, xi, eta, fixed = teacher_case(SIZES, 0, False)
    return md_ref.spread_and_tolerance(ptr, masses, x0, v0, forces, 0, DT, 0.0, 0.0, None, None, None)[1]


# ---- 1. teacher-forced replay ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cast", ["float64", "float32"])
@pytest.mark.parametrize("with_fixed", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("mode", [0, 1], ids=["nve", "langevin"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_teacher_forced_replay(batch, mode, with_fixed, cast):
    ptr, masses, x0, v0, forces, xi, eta, fixed = teacher_case(BATCHES[batch], mode, with_fixed)
    if cast == "float32":
        forces = forces.astype(np.float32)
    kT, fr = (KB * T_BATH, FR) if mode else (0.0, 0.0)
    (want_r, want_v), tol = md_ref.spread_and_tolerance(ptr, masses, x0, v0, forces.astype(np.float64), mode, DT, kT, fr, xi, eta, fixed)
    st = new_state(ptr, x0, masses, v0, fixed)
    assert st.n_small == int((np.diff(ptr) <= 192).sum())
    worst_r = worst_v = 0.0
    for k in range(forces.shape[0]):
        st.step(dev(forces[k]), None, mode, DT, kT, fr, xi=None if xi is None else dev(xi[k]), eta=None if eta is None else dev(eta[k]))
        got_r, got_v = st.r.cpu().numpy(), st.v.cpu().numpy()
        assert np.isfinite(got_r).all() and np.isfinite(got_v).all()
        worst_r, worst_v = max(worst_r, float(np.abs(got_r - want_r[k]).max())), max(worst_v, float(np.abs(got_v - want_v[k]).max()))
        assert torch.equal(st.pos32, st.r.float())
        if fixed is not None:
            assert np.array_equal(got_r[fixed], x0[fixed]) and not got_v[fixed].any()
    h = st.header()
    print(f"md_parity {batch} {'langevin' if mode else 'nve'} {'fixed' if with_fixed else 'free'} {cast}: "
          f"r spread perm {tol['r']['spread_permuted']:.3e} longdouble {tol['r']['spread_longdouble']:.3e} tol {tol['r']['tolerance']:.3e} worst {worst_r:.3e} | "
          f"v spread perm {tol['v']['spread_permuted']:.3e} longdouble {tol['v']['spread_longdouble']:.3e} tol {tol['v']['tolerance']:.3e} worst {worst_v:.3e}")
    assert h["step"] == forces.shape[0] and h["pending"] == (2 if mode else 1)
    assert worst_r <= tol["r"]["tolerance"] and worst_v <= tol["v"]["tolerance"]


# ---- 2. generator ---------------------------------------------------------------------------------------------------------------------------------
def test_generated_noise_equals_injected_normals_bitwise():
    ptr, masses, x0, v0, forces, _, _, _ = teacher_case(BATCHES["b5"], 1, False, steps=3)
    gen, inj = new_state(ptr, x0, masses, v0), new_state(ptr, x0, masses, v0)
    for k in range(3):
        f = dev(forces[k])
        xi, eta = inj.normals(77, k, 0), inj.normals(77, k, 1)
        gen.step(f, None, 1, DT, KB * T_BATH, FR, seed=77)
        inj.step(f, None, 1, DT, KB * T_BATH, FR, seed=77, xi=xi, eta=eta)
        assert torch.equal(bits(gen.r), bits(inj.r)) and torch.equal(bits(gen.v), bits(inj.v)), k
    gen.step(f, None, 1, DT, KB * T_BATH, FR, seed=77, finish_only=True)
    inj.step(f, None, 1, DT, KB * T_BATH, FR, seed=77, finish_only=True)
    assert torch.equal(bits(gen.v), bits(inj.v)) and not torch.equal(gen.r, dev(x0))


def test_normals_agree_with_the_numpy_philox():
    """First, a middle and the last atom of a molecule on each ownership path (192: wavefront, 512: workgroup) plus the 1-atom molecule; every draw.
    Box-Muller in float64 through two libraries' log / sin / cos: at most 4 units in the last place."""
    sizes = [192, 1, 512, 193]
    ptr, masses, x0, _ = md_ref.random_system(sizes, 3)
    key = np.array([5, -3, 2 ** 40 + 7, 11], dtype=np.int64)
    st = new_state(ptr, x0, masses, mol_key=key)
    atoms = [0, 96, 191, 192, 193, 193 + 256, 193 + 511, 705, 705 + 100, 705 + 192]
    worst = 0.0
    for seed, step in ((0, 0), (123456789012345, 7), (-5, 2 ** 31 - 1)):
        for draw in range(4):
            got = st.normals(seed, step, draw).cpu().numpy()
            want = md_ref.normals(seed, step, draw, ptr, key)
            ulps = np.abs(got[atoms] - want[atoms]) / np.spacing(np.abs(want[atoms]))
            worst = max(worst, float(ulps.max()))
    print(f"normals vs numpy Philox + Box-Muller: worst {worst:.2f} ulp")
    assert worst <= 4.0


def test_normal_statistics_over_2_20_draws():
    """342 molecules of 512 atoms x 3 components x 2 consecutive steps = 1 050 624 draws of xi.  Standard errors from the sample size: mean 1 / sqrt(n),
    variance sqrt(2 / n), fourth moment sqrt((105 - 9) / n) (E z^8 = 105, E z^4 = 3), lag-1 products of independent normals 1 / sqrt(pairs)."""
    ptr = np.arange(343) * 512
    st = new_state(ptr, np.zeros((int(ptr[-1]), 3)), np.ones(int(ptr[-1])))
    a, b = st.normals(2024, 10, 0).cpu().numpy(), st.normals(2024, 11, 0).cpu().numpy()
    z = np.concatenate([a.ravel(), b.ravel()])
    n = z.size
    assert n >= 2 ** 20
    checks = {"mean": (z.mean(), 0.0, 1.0 / np.sqrt(n)), "variance": ((z ** 2).mean(), 1.0, np.sqrt(2.0 / n)), "fourth": ((z ** 4).mean(), 3.0, np.sqrt(96.0 / n)),
              "lag1_atoms": ((a[:-1] * a[1:]).mean(), 0.0, 1.0 / np.sqrt(a[:-1].size)), "lag1_steps": ((a * b).mean(), 0.0, 1.0 / np.sqrt(a.size)),
              "xi_eta": ((a * st.normals(2024, 10, 1).cpu().numpy()).mean(), 0.0, 1.0 / np.sqrt(a.size))}
    for name, (got, want, se) in checks.items():
        print(f"{name}: {got:+.5f} (expected {want}, standard error {se:.2e}, {abs(got - want) / se:.2f} se)")
        assert abs(got - want) <= 5 * se, name


# ---- 3. physics with the Morse "model" -----------------------------------------------------------------------------------------------------------
def morse_setup():
    sizes = [42, 300]
    ptr = np.array([0, 42, 342])
    x0 = np.concatenate([md_ref.lattice_molecule(42, 1), md_ref.lattice_molecule(300, 2)])
    rng = np.random.Generator(np.random.PCG64(12))
    masses = rng.choice([1.008, 12.011, 14.007, 15.999], size=342)
    table = morse_table(x0 + rng.normal(0.0, 0.05, size=x0.shape), ptr)          # equilibrium distances near, not at, the start: forces from step 0
    return sizes, ptr, x0, masses, table


def morse_md(ptr, table, **kw):
    """BatchedMD on the float64 Morse potential evaluated on the master positions (the model reads state.r, as the L-BFGS free-running test does)."""
    from nabladft_amd.md import BatchedMD
    from nabladft_amd.optimization import PyGBatchwiseCalculator
    tdev = (dev(table[0]), dev(table[1]), dev(table[2]))
    B = len(ptr) - 1
    nmax = int(np.diff(ptr).max())
    gather = np.zeros((B, nmax), dtype=np.int64)
    valid = np.zeros((B, nmax), dtype=bool)
    for b in range(B):
        n = int(ptr[b + 1] - ptr[b])
        gather[b, :n], valid[b, :n] = np.arange(ptr[b], ptr[b + 1]), True
    gather, valid = dev(gather), dev(valid)
    holder = {}

    def model(batch):
        from lbfgs_helpers import MORSE_A, MORSE_D
        r = holder["md"].state.r
        nbr, d0, mask = tdev
        d = torch.where(mask, (r[:, None, :] - r[nbr]).pow(2).sum(-1).sqrt(), torch.ones_like(d0))
        per_atom = 0.5 * torch.where(mask, MORSE_D * (1.0 - torch.exp(-MORSE_A * (d - d0))) ** 2, torch.zeros_like(d0)).sum(1)
        energy = torch.where(valid, per_atom[gather], torch.zeros((), dtype=torch.float64, device=DEV)).sum(1)      # dense sum: fixed order
        return energy, morse_torch(r, tdev)

    md = holder["md"] = BatchedMD(PyGBatchwiseCalculator(model, DEV, energy_unit="Hartree", position_unit="Ang"), time_step=DT, **kw)
    return md


def batch_of(ptr, x0, z=None):
    from nabladft_amd import Batch
    B = len(ptr) - 1
    z = np.full(int(ptr[-1]), 6) if z is None else z
    return Batch(dev(x0), dev(z.astype(np.int64)), dev(np.repeat(np.arange(B), np.diff(ptr))), ptr=dev(np.asarray(ptr, dtype=np.int64)))


def test_nve_momentum_and_energy_with_the_morse_model(tol1):
    sizes, ptr, x0, masses, table = morse_setup()
    steps = 200
    md = morse_md(ptr, table, masses=masses, log_capacity=64, check_every=64)
    batch = batch_of(ptr, x0)
    md.init_velocities(batch, 300.0)
    v0 = md.velocities.cpu().numpy().copy()
    m = masses[:, None]
    p0 = np.add.reduceat(m * v0, ptr[:-1], axis=0)
    md.run(batch, steps)
    log = md.log
    assert log.shape == (steps + 1, 2, 8) and np.array_equal(log[:, 0, 0], np.arange(steps + 1))
    p1 = np.add.reduceat(m * md.velocities.cpu().numpy(), ptr[:-1], axis=0)
    bound_p = tol1["v"]["tolerance"] * steps
    print(f"|P1 - P0| {np.abs(p1 - p0).max():.3e}, bound {bound_p:.3e}")
    assert np.abs(p1 - p0).max() <= bound_p
    # the restatement on the same run: E_tot of the consistent (x, v) at every step
    ref = MDNumpy(ptr, masses, x0, v0)
    etot_ref = []
    for k in range(steps + 1):
        f, e = morse_np(ref.x, table, ptr)
        if k:
            ref.launch(f, 0, DT, finish_only=True)           # complete the velocities of this time ...
        etot_ref.append(ref.observables(e)["etot"])
        if k < steps:
            ref.launch(f, 0, DT)                             # ... and go on
    etot_ref = np.array(etot_ref)
    drift_ref = np.abs(etot_ref - etot_ref[0]).max(0)
    drift = np.abs(log[:, :, 1] - log[0, :, 1]).max(0)
    print(f"E_tot drift {drift}, restatement {drift_ref}; E_kin(0) {log[0, :, 3]}, T(0) {log[0, :, 4]}")
    assert (drift <= 2 * drift_ref).all()
    assert np.abs(log[:, :, 1] - etot_ref).max() <= 1e-9 and (log[:, :, 4] > 0).all()
    assert float(np.abs(md.positions.cpu().numpy() - x0).max()) > 1e-2


def test_nve_is_reversible_on_the_device():
    sizes, ptr, x0, masses, table = morse_setup()
    md = morse_md(ptr, table, masses=masses, log_capacity=0)
    batch = batch_of(ptr, x0)
    md.init_velocities(batch, 300.0)
    v0 = md.velocities.cpu().numpy().copy()
    md.run(batch, 100)
    assert md.state.header()["pending"] == 0
    moved = float(np.abs(md.positions.cpu().numpy() - x0).max())
    md.state.v.neg_()
    md.run(batch, 100)
    err = float(np.abs(md.positions.cpu().numpy() - x0).max())
    ref = MDNumpy(ptr, masses, x0, v0)
    for leg in range(2):
        for k in range(100):
            ref.launch(morse_np(ref.x, table)[0], 0, DT)
        ref.launch(morse_np(ref.x, table)[0], 0, DT, finish_only=True)
        ref.v = -ref.v
    err_ref = float(np.abs(ref.x - x0).max())
    print(f"moved {moved:.3e}; return error {err:.3e}, restatement {err_ref:.3e}")
    assert moved > 1e-2 and md.nsteps == 200
    assert err <= 2 * err_ref


# ---- 4. batch independence ------------------------------------------------------------------------------------------------------------------------
def batch_of_300(n, where=137):
    rng = np.random.Generator(np.random.PCG64(n))
    sizes = rng.integers(3, 80, size=300)
    sizes[::60] = 250                                                           # some workgroup-path neighbours
    sizes[where] = n
    return sizes


@pytest.mark.parametrize("n", [42, 300])
def test_a_molecule_alone_and_in_a_batch_of_300(n):
    where = 137
    sizes = batch_of_300(n, where)
    ptr, masses, x0, v0 = md_ref.random_system(sizes, 21)
    a, b = int(ptr[where]), int(ptr[where + 1])
    rng = np.random.Generator(np.random.PCG64(22))
    big = new_state(ptr, x0, masses, v0)
    solo = new_state(np.array([0, n]), x0[a:b], masses[a:b], v0[a:b], mol_key=[where])
    for k in range(10):
        f = rng.normal(0.0, 0.05, size=x0.shape)
        big.step(dev(f), None, 1, DT, KB * T_BATH, FR, seed=9)
        solo.step(dev(f[a:b]), None, 1, DT, KB * T_BATH, FR, seed=9)
        assert torch.equal(bits(big.r[a:b]), bits(solo.r)) and torch.equal(bits(big.v[a:b]), bits(solo.v)), k
    big.step(dev(f), None, 1, DT, KB * T_BATH, FR, seed=9, finish_only=True)
    solo.step(dev(f[a:b]), None, 1, DT, KB * T_BATH, FR, seed=9, finish_only=True)
    assert torch.equal(bits(big.v[a:b]), bits(solo.v))
    assert not torch.equal(big.r[a:b], dev(x0[a:b]))


# ---- 5. initialisation ----------------------------------------------------------------------------------------------------------------------------
def test_velocity_initialisation_on_the_mixed_batch():
    sizes = batch_of_300(300)
    sizes[[3, 4, 5, 6]] = [1, 2, 1, 2]
    ptr, masses, x0, _ = md_ref.random_system(sizes, 31)
    assert int(ptr[-1]) >= 10000
    st = new_state(ptr, x0, masses)
    T0 = 300.0
    st.init_velocities(T0, seed=4)
    v = st.v.cpu().numpy()
    assert np.isfinite(v).all()
    ref = MDNumpy(ptr, masses, x0, v)
    o = ref.observables()
    eps = 2.0 ** -52
    scale_p = ref.seg(ref.m * np.sqrt((v ** 2).sum(1, keepdims=True)))[:, 0]
    dd = x0 - ref.atoms(ref.seg(ref.m * x0) / ref.seg(ref.m))
    scale_l = ref.seg(ref.m * np.sqrt((dd ** 2).sum(1, keepdims=True)) * np.sqrt((v ** 2).sum(1, keepdims=True)))[:, 0]
    # every term of the sums is rounded at eps relative to its magnitude; 1000 x that, the project's factor between a format's precision and a bound
    assert (o["p_norm"] <= 1000 * eps * np.maximum(scale_p, 1e-300)).all()
    nonlinear = sizes >= 3
    print(f"|P| / scale {np.max(o['p_norm'] / np.maximum(scale_p, 1e-300)):.2e}, |L| / scale {np.max(o['l_norm'][nonlinear] / scale_l[nonlinear]):.2e}")
    assert (o["l_norm"][nonlinear] <= 1000 * eps * scale_l[nonlinear]).all()
    thermal = np.sqrt(md_ref.KAPPA * KB * T0 / masses)
    for b in np.nonzero(sizes == 1)[0]:                                                     # a single atom is at rest once its own momentum is removed
        assert np.abs(v[ptr[b]]).max() <= 1000 * eps * thermal[ptr[b]]
    for b in np.nonzero(sizes == 2)[0]:
        assert np.abs(v[ptr[b]:ptr[b + 1]]).max() > 0
    # the same normals through the restatement
    want = MDNumpy(ptr, masses, x0)
    want.init_velocities(st.normals(4, 0, 2).cpu().numpy(), KB * T0)
    assert np.abs(want.v - v).max() <= 1e-13 + 1000 * eps * np.abs(v).max() * 100          # omega carries cond(I) ~ 10-100 on random coordinates
    # temperature: E_kin is kT / 2 per remaining degree of freedom: 3 n minus 3 (translation) minus 3 / 2 / 0 (rotation of a body / a line / a point)
    removed = np.where(sizes == 1, 3, np.where(sizes == 2, 5, 6))
    D = float((3 * sizes - removed).sum())
    t_est = 2.0 * o["ekin"].sum() / (KB * D)
    se = T0 * np.sqrt(2.0 / D)                                                              # chi-square with D degrees of freedom: relative sd sqrt(2 / D)
    print(f"T estimate {t_est:.3f} K over D={D:.0f} degrees of freedom, standard error {se:.3f} K")
    assert abs(t_est - T0) <= 5 * se
    # the two removals can be switched off; then only the draw remains
    st.init_velocities(T0, seed=4, remove_translation=False, remove_rotation=False)
    plain = st.normals(4, 0, 2).cpu().numpy() * np.sqrt(md_ref.KAPPA * KB * T0 / masses)[:, None]
    assert np.abs(st.v.cpu().numpy() - plain).max() <= 4 * eps * np.abs(plain).max()


# ---- 6. rings and header --------------------------------------------------------------------------------------------------------------------------
def spring_md(**kw):
    from nabladft_amd.md import BatchedMD
    from nabladft_amd.optimization import PyGBatchwiseCalculator

    def model(batch):
        return torch.zeros(int(batch.ptr.shape[0]) - 1, device=DEV), -0.05 * batch.pos
    return BatchedMD(PyGBatchwiseCalculator(model, DEV, energy_unit="Hartree", position_unit="Ang"), time_step=DT, **kw)


def test_rings_drain_mid_run_and_finish_only_advances_nothing():
    sizes = [5, 200, 17]
    ptr, masses, x0, _ = md_ref.random_system(sizes, 41)
    runs = {}
    for name, caps in (("small", dict(frames=2, log_capacity=3)), ("ample", dict(frames=64, log_capacity=64))):
        md = spring_md(temp_bath=T_BATH, friction=FR, masses=masses, seed=3, interval=3, store_velocities=True, check_every=4, **caps)
        b = batch_of(ptr, x0)
        md.init_velocities(b, 300.0)
        md.run(b, 20)
        runs[name] = md
    s, a = runs["small"], runs["ample"]
    assert len(s._frames) > 1 and len(a._frames) == 1                                    # the small rings were drained mid-run
    assert s.log.shape == (7, 3, 8) and s.trajectory.shape == (7, int(ptr[-1]), 3) and s.trajectory_velocities.shape == s.trajectory.shape
    assert np.array_equal(s.log[:, 0, 0], np.arange(0, 20, 3))
    for x, y in ((s.log, a.log), (s.trajectory, a.trajectory), (s.trajectory_velocities, a.trajectory_velocities)):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    assert np.array_equal(s.trajectory[0], x0)
    h = s.state.header()
    assert h["step"] == 20 == s.nsteps and h["pending"] == 0 and h["overflow"] == 0 and h["log_rows"] == 0 and h["frames"] == 0
    st = s.state
    before = st.buf.clone()
    st.step(s.calculator.forces, None, 1, DT, KB * T_BATH, FR, interval=3, seed=3, finish_only=True)
    torch.cuda.synchronize()
    assert torch.equal(before, st.buf)
    # a second run continues the trajectory: 10 + 10 steps == 20 steps
    two = spring_md(temp_bath=T_BATH, friction=FR, masses=masses, seed=3, interval=3, frames=64, log_capacity=64)
    b = batch_of(ptr, x0)
    two.init_velocities(b, 300.0)
    two.run(b, 10)
    two.run(b, 10)
    assert torch.equal(bits(two.positions), bits(a.positions)) and torch.equal(bits(two.velocities), bits(a.velocities))
    assert np.array_equal(two.log.view(np.int64), a.log.view(np.int64))
    # a ring the host does not drain in time: the sample is dropped and the header says so
    tiny = new_state(ptr, x0, masses, log_capacity=1)
    f = dev(np.zeros_like(x0))
    tiny.step(f, None, 0, DT)
    tiny.step(f, None, 0, DT)
    h = tiny.header()
    assert h["log_rows"] == 1 and h["overflow"] == 1 and h["step"] == 2


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from nabladft_amd import _lib
    from nabladft_amd.md import BatchedMD, MDState
    from nabladft_amd.optimization import PyGBatchwiseCalculator
    lib = _lib.load()
    with pytest.raises(_lib.NablaqError) as e:
        MDState([0, 513, 520], torch.zeros(520, 3, device=DEV), np.ones(520))
    assert e.value.code == _lib.NQ_ERR_MOL_TOO_LARGE and "513 atoms" in str(e.value)
    m0 = np.ones(12)
    m0[7] = 0.0
    with pytest.raises(_lib.NablaqError) as e:
        MDState([0, 5, 12], torch.zeros(12, 3, device=DEV), m0)
    assert e.value.code == _lib.NQ_ERR_ARG and "mass" in str(e.value)
    assert lib.nq_md_state_bytes(12, 2, 0, 4, 1) == 0 and b"capacity 0" in lib.nq_last_error()
    assert lib.nq_md_state_bytes(12, 2, 4, 0, 3) == 0 and b"capacity 0" in lib.nq_last_error()
    st = MDState([0, 5, 12], torch.ones(12, 3, device=DEV, dtype=torch.float64), np.ones(12), log_capacity=4)
    f = torch.ones(12, 3, device=DEV)
    torch.cuda.synchronize()
    before = st.buf.clone()
    for bad in (dict(dt=0.0), dict(dt=-0.5), dict(kT=-1e-3), dict(friction=-0.01), dict(interval=0)):
        kw = dict(mode=1, dt=0.5, kT=1e-3, friction=0.01)
        kw.update(bad)
        with pytest.raises(_lib.NablaqError) as e:
            st.step(f, None, **kw)
        assert e.value.code == _lib.NQ_ERR_ARG
    with pytest.raises(_lib.NablaqError) as e:
        st.init_velocities(-300.0)
    assert e.value.code == _lib.NQ_ERR_ARG
    with pytest.raises(ValueError):
        st.step(torch.ones(11, 3, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(before, st.buf) and st.header()["step"] == 0
    # a negative bath temperature and an unknown element through the public class
    calc = PyGBatchwiseCalculator(lambda b: (torch.zeros(2, device=DEV), torch.zeros(12, 3, device=DEV)), DEV, energy_unit="Hartree", position_unit="Ang")
    ptr = np.array([0, 5, 12])
    with pytest.raises(_lib.NablaqError):
        BatchedMD(calc, temp_bath=-10.0).run(batch_of(ptr, np.zeros((12, 3))), 1)
    with pytest.raises(ValueError, match="no atomic mass"):
        BatchedMD(calc).run(batch_of(ptr, np.zeros((12, 3)), z=np.array([6] * 11 + [53])), 1)
    BatchedMD(calc, masses=np.full(12, 126.9)).run(batch_of(ptr, np.zeros((12, 3)), z=np.array([6] * 11 + [53])), 1)
    with pytest.raises(NotImplementedError):
        PyGBatchwiseCalculator(lambda b: None, DEV, energy_unit="eV", position_unit="Ang")
    # a step with other dimensions than the state was prepared for touches nothing and is reported
    rc = lib.nq_md_step(_lib.ptr(st.buf), 12, 2, 1, 4, 0, 1, _lib.ptr(f), 0, None, 0, _lib.ptr(st.pos32), 0, 0.5, 0.0, 0.0, 1, 0, None, None, 0, _lib.stream_ptr())
    assert rc == 0
    with pytest.raises(RuntimeError, match="other dimensions"):
        st.header()
    assert torch.equal(before[128:], st.buf[128:]) and int(st.header_dev[0]) == 0


# ---- 8. through a real engine ---------------------------------------------------------------------------------------------------------------------
def test_painn_nve_through_the_interface(tmp_path, tol1):
    import nabladft_amd as nq
    from nabladft_amd.md import masses_for, write_xyz
    from oracle import painn_ref as R
    cfg = R.PaiNNConfig(hidden_channels=64, num_layers=2, num_rbf=20, cutoff=5.0, max_neighbors=100)
    pos, z, batch, _, _ = R.gen_conformers(11, 2, size=(10, 20))
    sizes = np.bincount(batch.numpy())
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    path = str(tmp_path / "start.xyz")
    write_xyz(path, z.numpy(), ptr, pos.double().numpy())
    model = nq.PaiNN(cfg.hidden_channels, cfg.num_layers, cfg.num_rbf, cfg.cutoff, cfg.max_neighbors, {"name": "gaussian"},
                     {"name": "polynomial", "exponent": 5}, True, False, False, True, cfg.num_elements)
    model.load_state_dict(R.make_params(cfg, seed=3), strict=False)
    model.eval()
    it = nq.PYGAseInterface(path, str(tmp_path / "work"), None, model, device=DEV)
    assert np.array_equal(it.z, z.numpy()) and np.array_equal(it.ptr, ptr)
    it.calculate_single_point()
    assert it.energy.shape == (2,) and it.forces.shape == (int(ptr[-1]), 3) and os.path.exists(str(tmp_path / "work" / "single_point.xyz"))
    steps = 30
    it.init_md("nve", time_step=DT, temp_init=300, temp_bath=None, interval=1)
    st = it.dynamics.state
    x0, v0 = st.r.cpu().numpy().copy(), st.v.cpu().numpy().copy()
    recorded = []
    inner = it.calculator.calculate

    def calculate(b):
        inner(b)
        recorded.append(it.calculator.forces.cpu().numpy().copy())

    it.calculator.calculate = calculate
    it.run_md(steps)
    assert len(recorded) == steps + 1 and recorded[0].dtype == np.float32
    ref = MDNumpy(ptr, masses_for(z.numpy()), x0, v0)
    for k in range(steps):
        ref.launch(recorded[k], 0, DT)
    ref.launch(recorded[steps], 0, DT, finish_only=True)
    dr, dv = float(np.abs(it.positions - ref.x).max()), float(np.abs(it.velocities - ref.v).max())
    print(f"PaiNN NVE, {steps} steps: |dr| {dr:.3e} (bound {tol1['r']['tolerance']:.3e}), |dv| {dv:.3e}; moved {np.abs(it.positions - x0).max():.3e}")
    assert dr <= tol1["r"]["tolerance"] and dv <= tol1["v"]["tolerance"]
    assert np.abs(it.positions - x0).max() > 1e-3
    lines = open(str(tmp_path / "work" / "nve.log")).read().splitlines()
    assert len(lines) == 2 * (2 + steps + 1) and lines[0] == "# molecule 0" and lines[1].split() == ["Time[ps]", "Etot[Hartree]", "Epot[Hartree]", "Ekin[Hartree]", "T[K]"]
    rows = np.array([[float(t) for t in ln.split()] for ln in lines[2:2 + steps + 1]])
    assert rows.shape == (steps + 1, 5) and np.allclose(rows[:, 0], np.arange(steps + 1) * DT / 1000.0, atol=1e-4) and np.allclose(rows[:, 1], rows[:, 2] + rows[:, 3], atol=2e-8)
    npz = np.load(str(tmp_path / "work" / "nve.npz"))
    assert npz["positions"].shape == (steps + 1, int(ptr[-1]), 3) and np.array_equal(npz["ptr"], ptr) and np.array_equal(npz["z"], z.numpy())
    assert np.array_equal(npz["positions"][0], x0) and np.array_equal(npz["positions"][-1], it.positions)
    assert os.path.exists(str(tmp_path / "work" / "nve.extxyz"))
    with open("/proc/self/maps") as f:
        assert "libnablaq.so" in f.read()


# ---- the interface on an energy database: Langevin, then NVE with the kept velocities, then relaxation --------------------------------------------
def test_interface_on_a_database_langevin_nve_optimize(tmp_path):
    import nabladft_amd as nq
    db = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "energy_db_30.db")
    arena = nq.read_energy_database(db)
    target = (arena.pos.double() * 0.98).to(DEV)

    def model(batch):                                          # a harmonic pull of every atom towards a slightly shrunk geometry
        d = batch.pos.double() - target
        return torch.zeros(int(batch.ptr.shape[0]) - 1, device=DEV, dtype=torch.float64), -0.5 * d

    it = nq.PYGAseInterface(db, str(tmp_path / "work"), None, model, device=DEV, fixed_atoms=[0])
    B, N = 30, int(arena.pos.shape[0])
    assert len(it.ptr) == B + 1 and np.array_equal(it.ptr, arena.ptr.numpy()) and np.array_equal(it.z, arena.z.numpy())
    x0 = it.positions.copy()
    fixed = it.ptr[:-1]
    it.init_md("nvt", time_step=DT, temp_init=300, temp_bath=300, interval=2)
    it.run_md(6)
    assert np.array_equal(it.positions[fixed], x0[fixed]) and not it.velocities[fixed].any() and np.abs(it.positions - x0).max() > 1e-3
    lines = open(str(tmp_path / "work" / "nvt.log")).read().splitlines()
    assert len(lines) == B * (2 + 4) and lines[6] == "# molecule 1"                       # steps 0, 2, 4, 6
    npz = np.load(str(tmp_path / "work" / "nvt.npz"))
    assert npz["positions"].shape == (4, N, 3) and np.array_equal(npz["steps"], [0, 2, 4, 6]) and np.array_equal(npz["positions"][-1], it.positions)
    v_kept = it.velocities.copy()
    it.init_md("nve", time_step=DT, temp_bath=None, interval=1)                           # reset=False: the velocities stay
    assert np.array_equal(it.dynamics.velocities.cpu().numpy(), v_kept)
    it.run_md(3)
    npz = np.load(str(tmp_path / "work" / "nve.npz"))
    assert np.array_equal(npz["steps"], [7, 8, 9]) and npz["positions"].shape == (3, N, 3)  # step 6 was sampled by the first run
    assert it.dynamics.state.header()["step"] == 9
    it.init_md("again", time_step=DT, temp_bath=None, reset=True)
    assert not np.array_equal(it.dynamics.velocities.cpu().numpy(), it.velocities)
    assert it.optimize(fmax=1e-3, steps=60) is True
    assert it.dynamics is None and os.path.exists(str(tmp_path / "work" / "optimization.extxyz"))
    free = np.ones(N, dtype=bool)
    free[fixed] = False
    assert np.sqrt(((it.positions - target.cpu().numpy())[free] ** 2).sum(1)).max() < 2e-3 + 1e-6      # |f| = 0.5 |d| < fmax; the target is float32 data
    assert np.array_equal(it.positions[fixed], x0[fixed])
