"""GPU: the device-resident batched L-BFGS (csrc/lbfgs.hip through the C ABI and through nabladft_amd.optimization) against the recorded runs of the real
reference (tests/golden/lbfgs_*.npz, scripts/make_golden_lbfgs.py) and against the float64 numpy restatement (tests/lbfgs_helpers.py, pinned to the reference in
tests/test_optimization_cpu.py).

Tolerances come from the fixtures.  ``reorder_spread`` is what the reference's own positions move by when only its summation order changes; the kernel is
allowed 1000 x that, because it differs by more than a reordering (another reduction tree, contracted multiply-adds) and rho = 1/ys amplifies: about 1e-11 A on
steps of 0.01-0.2 A.  rho spans 1 .. 1e9, so the same factor is applied relative to its magnitude.  Masks, normalisation counts and step counts are integers
and booleans: compared exactly.  Case D (HIP PaiNN as the model, float32) is held to max(10 x own_spread[k], 1e-6 A) of the reference's float64 run, where
own_spread[k] is the distance between the reference's float32 and float64 runs at step k."""
import os
import shutil
import sqlite3

import numpy as np
import pytest
import torch

from lbfgs_helpers import LbfgsNumpy, morse_torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def load_case(name):
    fx = dict(np.load(os.path.join(GOLDEN, f"lbfgs_{name}.npz")))
    fx["f"] = np.load(os.path.join(GOLDEN, f"lbfgs_{name}_forces.npz"))["f"]
    return fx


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def new_state(ptr, r0, memory):
    from nabladft_amd.optimization import LBFGSState
    return LBFGSState(ptr, dev(r0), memory)


def fixed_mask(fx, N):
    if not fx["fixed"].size:
        return None
    m = torch.zeros(N, dtype=torch.uint8)
    m[torch.from_numpy(fx["fixed"])] = 1
    return m.to(DEV)


def ring(st, name, K):
    """The history of a state after K steps, oldest -> newest, like the reference's lists: pair p sits in slot p % memory."""
    L = min(K - 1, st.memory)
    slots = [p % st.memory for p in range(K - 1 - L, K - 1)]
    return getattr(st, name)[slots].cpu().numpy()


# ---- 1. teacher-forced replay of the reference's runs through the C ABI ---------------------------------------------------------------------------
@pytest.mark.parametrize("cast", ["float64", "float32"])
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_teacher_forced_replay(case, cast):
    fx = load_case(case)
    tol = 1000 * float(fx["reorder_spread"])
    ptr, K, fmax, mem, maxstep = fx["ptr"], int(fx["nsteps"]), float(fx["fmax"]), int(fx["memory"]), float(fx["maxstep"])
    st = new_state(ptr, fx["r"][0], mem)
    fixed = fixed_mask(fx, st.N)
    ref = LbfgsNumpy(ptr, memory=mem, maxstep=maxstep, fixed=fx["fixed"] if fx["fixed"].size else None)
    worst = 0.0
    for k in range(K):
        f = fx["f"][k] if cast == "float64" else fx["f"][k].astype(np.float32)
        st.r.copy_(dev(fx["r"][k]))
        st.step(dev(f), fmax, maxstep, 1.0, 1.0, fixed)
        want = ref.step(fx["r"][k], f, fmax)          # the restatement fed the same (cast) forces; equals the fixture's r[k + 1] for float64 (CPU test)
        if cast == "float64":
            want = fx["r"][k + 1]
            assert ref.n_normalizations == int(fx["nnorm"][k])
        h = st.header()
        got = st.r.cpu().numpy()
        assert np.array_equal(st.converged_dev.cpu().numpy().astype(bool), fx["mask"][k]), k
        assert np.array_equal(ref.mask, fx["mask"][k]), k
        assert h["normalizations"] == ref.n_normalizations and h["iteration"] == k + 1, (k, h)
        assert h["unconverged"] == int((~fx["mask"][k]).sum())
        worst = max(worst, float(np.abs(got - want).max()))
        assert torch.equal(st.pos32, st.r.float())
    print(f"case {case} {cast}: {K} steps, worst |dr| {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol
    rho, rho_ref = ring(st, "rho", K), np.array(ref.rho)
    assert rho.shape == rho_ref.shape
    rel = float((np.abs(rho - rho_ref) / np.maximum(1.0, np.abs(rho_ref))).max())
    print(f"  rho: worst relative deviation {rel:.3e}")
    assert rel <= tol
    if cast == "float64":
        assert (np.abs(rho - fx["rho"]) <= tol * np.maximum(1.0, np.abs(fx["rho"]))).all()
        assert np.array_equal(ring(st, "S", K), np.array(ref.s)) and np.array_equal(ring(st, "Y", K), np.array(ref.y))     # differences of identical doubles
    assert st.header()["latch"] == -1                 # the reference never saw an all-converged batch before its last model call


# ---- 2. free-running case A through the public class ----------------------------------------------------------------------------------------------
def free_run(fx, check_every=1, steps=None, **kw):
    from nabladft_amd import Batch
    from nabladft_amd.optimization import ASEBatchwiseLBFGS, PyGBatchwiseCalculator
    table = (dev(fx["nbr"]), dev(fx["d0"]), dev(fx["nbr_mask"]))
    ptr = fx["ptr"]
    holder = {}

    def model(batch):
        # "calculator in float64": the potential reads the float64 master positions, as the reference's calculator did in this case
        f = morse_torch(holder["opt"].state.r, table)
        return torch.zeros(len(ptr) - 1, device=DEV, dtype=torch.float64), f

    calc = PyGBatchwiseCalculator(model, DEV, energy_unit="Hartree", position_unit="Ang")
    opt = holder["opt"] = ASEBatchwiseLBFGS(calc, logfile=None, memory=int(fx["memory"]), maxstep=float(fx["maxstep"]), check_every=check_every, **kw)
    batch = Batch(dev(fx["r"][0]), dev(fx["z"]), dev(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))), ptr=dev(ptr))
    ok = opt.run(batch, fmax=float(fx["fmax"]), steps=int(fx["steps"]) if steps is None else steps)
    return ok, opt


@pytest.mark.parametrize("check_every", [1, 7])
def test_free_running_case_a(check_every):
    fx = load_case("A")
    tol = 1000 * float(fx["reorder_spread"])
    ok, opt = free_run(fx, check_every)
    dr = float(np.abs(opt.positions.cpu().numpy() - fx["r"][-1]).max())
    print(f"free run, check_every={check_every}: nsteps {opt.nsteps} (reference {int(fx['nsteps'])}), |dr| {dr:.3e}, bound {tol:.3e}")
    assert ok is True and bool(fx["converged"])
    assert opt.nsteps == int(fx["nsteps"]) and opt.n_normalizations == int(fx["nnorm"][-1])
    assert dr <= tol
    assert bool(opt.converged_mask.all()) and opt.converged()


def test_steps_exhausted_is_not_converged():
    fx = load_case("B")
    ok, opt = free_run(fx, steps=5)
    assert ok is False and opt.nsteps == 5 and opt.n_normalizations == int(fx["nnorm"][4])
    assert float(np.abs(opt.positions.cpu().numpy() - fx["r"][5]).max()) <= 1000 * float(fx["reorder_spread"])
    want = np.maximum.reduceat((fx["f"][5] ** 2).sum(1), fx["ptr"][:-1]) < float(fx["fmax"]) ** 2
    assert np.array_equal(opt.converged_mask.cpu().numpy(), want)


def test_two_runs_are_bit_identical():
    fx = load_case("A")
    a, b = free_run(fx)[1], free_run(fx)[1]
    n = a.nsteps                                     # ring slots written so far (memory 100 > nsteps); the rest is whatever the allocator left
    assert n == b.nsteps
    for x, y in ((a.positions, b.positions), (a.state.S[:n], b.state.S[:n]), (a.state.Y[:n], b.state.Y[:n]), (a.state.rho[:n], b.state.rho[:n])):
        assert torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))


# ---- 3. random operator cases against the restatement ---------------------------------------------------------------------------------------------
SIZES = [1, 2, 21, 22, 64, 65, 170, 171, 192, 193, 512]


def random_walk(sizes, memory, steps, seed, st_factory=None, maxstep=0.2, fmax=2e-3, perm=None):
    """A restatement run on anisotropic springs (per-atom stiffness, a little noise): yields (r_k, f_k, r_{k+1}, restatement) per step.  perm: the same run
    with the atoms renumbered (new atom i = old atom perm[i])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N = int(ptr[-1])
    centre = rng.normal(0.0, 2.0, size=(N, 3))
    kappa = rng.uniform(0.2, 1.6, size=(N, 3))
    r = centre + rng.normal(0.0, 0.15, size=(N, 3))
    noise = rng.normal(0.0, 1e-4, size=(steps, N, 3))
    if perm is not None:
        centre, kappa, r, noise = centre[perm], kappa[perm], r[perm], noise[:, perm]
    ref = LbfgsNumpy(ptr, memory=memory, maxstep=maxstep)
    for k in range(steps):
        f = -kappa * (r - centre) + noise[k]
        new = ref.step(r, f, fmax)
        yield r, f, new, ref
        r = new


def inner_perm(sizes, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    return np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])])


@pytest.mark.parametrize("B,memory,steps", [(2048, 1, 4), (2048, 3, 8), (44, 100, 106), (11, 3, 8)])
def test_random_batches_against_the_restatement(B, memory, steps):
    rng = np.random.Generator(np.random.PCG64(B + memory))
    if B >= 1024:       # mostly drug-sized molecules, every boundary size a few times, a handful of large ones
        sizes = np.concatenate([np.repeat(SIZES[:-1], 4), [512, 512], rng.integers(20, 60, size=B - 4 * (len(SIZES) - 1) - 2)])
    else:
        sizes = np.array((SIZES * (B // len(SIZES) + 1))[:B])
    sizes = sizes[rng.permutation(B)]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    perm = inner_perm(sizes, 5)
    inv = np.argsort(perm)
    st = None
    worst = spread = scale = 0.0
    worst_rho = 0.0
    clamps = 0
    for (r, f, want, ref), (_, _, pwant, _) in zip(random_walk(sizes, memory, steps, 7), random_walk(sizes, memory, steps, 7, perm=perm)):
        if st is None:
            st = new_state(ptr, r, memory)
            assert st.n_small == int((sizes <= 192).sum())
        st.r.copy_(dev(r))
        st.step(dev(f), 2e-3, 0.2, 1.0, 1.0)
        got = st.r.cpu().numpy()
        assert not np.isnan(got).any()
        assert np.array_equal(st.converged_dev.cpu().numpy().astype(bool), ref.mask)
        assert st.header()["normalizations"] == ref.n_normalizations
        worst = max(worst, float(np.abs(got - want).max()))
        spread = max(spread, float(np.abs(pwant[inv] - want).max()))
        scale = max(scale, float(np.abs(want).max()))
        if ref.iteration > 1:
            slot = (ref.iteration - 2) % memory
            assert np.array_equal(st.S[slot].cpu().numpy(), ref.s[-1]) and np.array_equal(st.Y[slot].cpu().numpy(), ref.y[-1])
            worst_rho = max(worst_rho, float((np.abs(st.rho[slot].cpu().numpy() - ref.rho[-1]) / np.maximum(1.0, np.abs(ref.rho[-1]))).max()))
        clamps = ref.n_normalizations
    # 1000 x the restatement's own spread under permutation; only where that spread is exactly zero (nothing to reorder) one unit in the last place of the coordinates
    tol = 1000 * (spread if spread > 0.0 else scale * 2.0 ** -52)
    print(f"B={B} memory={memory}: {steps} steps, {clamps} clamps, worst |dr| {worst:.3e}, restatement spread {spread:.3e}, bound {tol:.3e}, rho {worst_rho:.3e}")
    assert worst <= tol and worst_rho <= tol
    assert steps > memory + 1 and clamps > 0                                   # the ring wrapped, the clamp fired


# ---- 4. batch invariance --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [42, 300])
def test_a_molecule_alone_and_in_a_batch_of_300(n):
    rng = np.random.Generator(np.random.PCG64(n))
    sizes = rng.integers(3, 80, size=300)
    sizes[::60] = 250                                                           # some workgroup-path neighbours
    where = 137
    sizes[where] = n
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    a, b = int(ptr[where]), int(ptr[where + 1])
    big = solo = None
    for r, f, want, ref in random_walk(sizes, 3, 8, 11):
        if big is None:
            big, solo = new_state(ptr, r, 3), new_state(np.array([0, n]), r[a:b], 3)
        big.r.copy_(dev(r)), solo.r.copy_(dev(r[a:b]))
        big.step(dev(f), 2e-3, 0.2, 1.0, 1.0)
        solo.step(dev(f[a:b]), 2e-3, 0.2, 1.0, 1.0)
        bits = lambda t: t.contiguous().view(torch.int64)
        assert torch.equal(bits(big.r[a:b]), bits(solo.r))
        assert torch.equal(bits(big.S[:, a:b]), bits(solo.S)) or ref.iteration <= 3     # unwritten slots hold whatever the allocator left
        if ref.iteration > 3:
            assert torch.equal(bits(big.Y[:, a:b]), bits(solo.Y)) and torch.equal(bits(big.rho[:, where]), bits(solo.rho[:, 0]))
        assert int(big.converged_dev[where]) == int(solo.converged_dev[0])
    assert ref.iteration == 8


# ---- 5. case D: the HIP PaiNN as the model --------------------------------------------------------------------------------------------------------
def test_case_d_painn_trajectory():
    import nabladft_amd as nq
    from nabladft_amd.optimization import ASEBatchwiseLBFGS, PyGBatchwiseCalculator
    from oracle import painn_ref as R
    fx = dict(np.load(os.path.join(GOLDEN, "lbfgs_D.npz")))
    cfg = R.PaiNNConfig(hidden_channels=64, num_layers=2, num_rbf=20, cutoff=5.0, max_neighbors=100)
    pos, z, batch, _, _ = R.gen_conformers(11, 4, size=(8, 20))
    model = nq.PaiNN(cfg.hidden_channels, cfg.num_layers, cfg.num_rbf, cfg.cutoff, cfg.max_neighbors, {"name": "gaussian"},
                     {"name": "polynomial", "exponent": 5}, True, False, False, True, cfg.num_elements)
    model.load_state_dict(R.make_params(cfg, seed=3), strict=False)
    model.eval()
    calc = PyGBatchwiseCalculator(model, DEV, energy_unit="Hartree", position_unit="Ang")
    opt = ASEBatchwiseLBFGS(calc, logfile=None)
    traj, energies = [], []
    inner = calc.calculate

    def calculate(b):
        inner(b)
        traj.append(opt.state.r.cpu().numpy().copy()), energies.append(calc.energy.cpu().double().numpy().copy())

    calc.calculate = calculate
    ok = opt.run(nq.Batch(pos, z, batch).to(DEV), fmax=float(fx["fmax"]), steps=int(fx["steps"]))
    assert opt.nsteps == int(fx["nsteps"]) == 10 and len(traj) == 11
    assert opt.n_normalizations == int(fx["nnorm"][-1])
    for k in range(11):
        d = float(np.abs(traj[k] - fx["r64"][k]).max())
        bound = max(10 * float(fx["own_spread"][k]), 1e-6)
        print(f"step {k}: |r - r64| {d:.3e}  bound {bound:.3e}  (reference's own float32 run: {float(fx['own_spread'][k]):.3e})")
        assert d <= bound, k
    print("energies", energies[0], "->", energies[-1], "reference", fx["e_start"], "->", fx["e_end"])
    assert (energies[-1] < energies[0]).all()
    with open("/proc/self/maps") as f:
        assert "libnablaq.so" in f.read()


# ---- 6. error paths through the ABI (argument checks on the host, before any launch) --------------------------------------------------------------
def test_error_paths():
    from nabladft_amd import _lib
    from nabladft_amd.optimization import LBFGSState
    lib = _lib.load()
    with pytest.raises(_lib.NablaqError) as e:
        LBFGSState([0, 513, 520], torch.zeros(520, 3, device=DEV), 10)
    assert e.value.code == _lib.NQ_ERR_MOL_TOO_LARGE and "513 atoms" in str(e.value)
    with pytest.raises(_lib.NablaqError) as e:
        LBFGSState([0, 5], torch.zeros(5, 3, device=DEV), 0)
    assert e.value.code == _lib.NQ_ERR_ARG and "memory=0" in str(e.value)
    st = LBFGSState([0, 5, 12], torch.ones(12, 3, device=DEV, dtype=torch.float64), 4)
    before = st.buf.clone()
    f = torch.ones(12, 3, device=DEV)
    for bad in (dict(maxstep=0.0), dict(maxstep=-1.0), dict(alpha=0.0)):
        kw = dict(fmax=0.05, maxstep=0.2, damping=1.0, alpha=1.0)
        kw.update(bad)
        with pytest.raises(_lib.NablaqError) as e:
            st.step(f, **kw)
        assert e.value.code == _lib.NQ_ERR_ARG
    rc = lib.nq_lbfgs_step(_lib.ptr(st.buf), 12, 2, 0, 2, _lib.ptr(f), 0, None, _lib.ptr(st.pos32), 0.05, 0.2, 1.0, 1.0, 0, _lib.stream_ptr())
    assert rc == _lib.NQ_ERR_ARG and b"memory=0" in lib.nq_last_error()
    torch.cuda.synchronize()
    assert torch.equal(before, st.buf) and st.header()["iteration"] == 0
    with pytest.raises(ValueError):
        st.step(torch.ones(11, 3, device=DEV), 0.05, 0.2, 1.0, 1.0)
    # a step with other dimensions than the state was prepared for touches nothing and is reported
    rc = lib.nq_lbfgs_step(_lib.ptr(st.buf), 12, 2, 4, 1, _lib.ptr(f), 0, None, _lib.ptr(st.pos32), 0.05, 0.2, 1.0, 1.0, 0, _lib.stream_ptr())
    assert rc == 0
    with pytest.raises(RuntimeError, match="other dimensions"):
        st.header()
    assert torch.equal(before[64:], st.buf[64:])


# ---- the task with the real optimiser ---------------------------------------------------------------------------------------------------------------
def test_task_on_the_device(tmp_path):
    from nabladft_amd import read_energy_database
    from nabladft_amd.data import _decode_ase_blob
    from nabladft_amd.optimization import ASEBatchwiseLBFGS, BatchwiseOptimizeTask, PyGBatchwiseCalculator
    inp, out = str(tmp_path / "in.db"), str(tmp_path / "out.db")
    shutil.copy(os.path.join(GOLDEN, "energy_db_30.db"), inp)
    finals = []

    class Recording(ASEBatchwiseLBFGS):
        def run(self, *a, **k):
            ok = super().run(*a, **k)
            finals.append((ok, self.nsteps, self.positions.cpu().numpy().copy()))
            return ok

    opt = Recording(PyGBatchwiseCalculator(spring_model_dev, DEV, energy_unit="Hartree", position_unit="Ang"), logfile=None, check_every=3)
    BatchwiseOptimizeTask(inp, out, opt, batch_size=8, fmax=1e-3, steps=50).run()
    assert len(finals) == 4 and all(ok and 0 < n < 50 for ok, n, _ in finals)
    final = np.concatenate([p for _, _, p in finals])
    con = sqlite3.connect(out)
    rows = con.execute("select positions, data, natoms from systems order by id").fetchall()
    con.close()
    assert len(rows) == 30
    assert np.array_equal(np.concatenate([np.frombuffer(p, dtype=np.float64).reshape(-1, 3) for p, _, _ in rows]), final)
    for p, d, n in rows:
        d = _decode_ase_blob(d)
        assert d["model_forces"].shape == (n, 3) and np.sqrt((d["model_forces"].astype(np.float64) ** 2).sum(1).max()) < 1e-3 and len(d["model_energy"]) == 1
    assert torch.equal(read_energy_database(out).pos, torch.from_numpy(final.astype(np.float32)))


def spring_model_dev(batch):
    """tests/test_optimization_cpu.py: spring_model, with a gather-free deterministic centroid (segment mean through cumulative sums would lose digits)."""
    B = int(batch.ptr.shape[0]) - 1
    onehot = torch.nn.functional.one_hot(batch.batch, B).to(batch.pos.dtype)             # [N, B]: small batches only
    cen = (onehot.t() @ batch.pos) / onehot.sum(0)[:, None]
    d = batch.pos - cen[batch.batch]
    return 0.25 * (onehot.t() @ d.pow(2).sum(1, keepdim=True)).reshape(-1), -0.5 * d
