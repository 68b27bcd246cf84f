"""GPU: batched normal modes (csrc/vib.hip through the C ABI and through nabladft_amd.vibrations) against the float64 numpy restatement (tests/vib_ref.py,
whose properties tests/test_vib_cpu.py pins), against ``np.linalg.eigh`` and against a float64 PaiNN fixture.  ase is not available: nothing is pinned against it.

Bounds.  Displace / accumulate: bitwise (the kernels and the restatement do the same IEEE operations; the file is built without contraction).  Eigensolver:
10 m 2^-52, relative to |A|_2 for eigenvalues and residual and to 1 for orthogonality -- Jacobi and LAPACK are both backward stable to O(m eps |A|_2), the numpy
emulation of this ordering measures 0.2-1.7 in those units, ten leaves room for another rounding order.  Hessians through a model: 10 x the restatement's own
spread between float64 forces and forces rounded to float32 (the convention of the L-BFGS case D).  Measured ratios: profiles/vib_parity.txt."""
import os

import numpy as np
import pytest
import torch

import vib_ref
from lbfgs_helpers import morse_np, morse_table, morse_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C12 = 12.011
EIG_SIZES = [3, 6, 9, 126, 141, 144, 192]
KINDS = ["random", "zero", "diagonal", "hessian"]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def calculator(model):
    from nabladft_amd.optimization import PyGBatchwiseCalculator
    return PyGBatchwiseCalculator(model, DEV, energy_unit="Hartree", position_unit="Ang")


def batch_of(ptr, x0, z=None):
    from nabladft_amd import Batch
    B = len(ptr) - 1
    z = np.full(int(ptr[-1]), 6) if z is None else z
    return Batch(dev(x0), dev(np.asarray(z).astype(np.int64)), dev(np.repeat(np.arange(B), np.diff(ptr))), ptr=dev(np.asarray(ptr, dtype=np.int64)))


# ---- 1. displace and accumulate, teacher-forced ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cast", ["float32", "float64"])
def test_displace_and_accumulate_bitwise(cast):
    """1, 2, 3, 42 and 48 atoms, a molecule with fixed atoms and a fully fixed one; 100 displacements per call split the larger molecules across calls."""
    from nabladft_amd.vibrations import VibState, chunks
    sizes = [1, 2, 3, 42, 48, 5, 3]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.Generator(np.random.PCG64(21))
    N = int(ptr[-1])
    x0 = rng.normal(size=(N, 3)) * 3.0 + 8.0
    fixed = [96, 98, 101, 102, 103]                                    # two atoms of the 5-atom molecule, all of the last one
    masses = rng.choice([1.008, 12.011, 15.999], size=N)
    st = VibState(ptr, dev(x0), masses, fixed)
    pl = vib_ref.plan(ptr, fixed)
    assert st.D == len(pl["disp"]) == 3 * (N - 5) and np.array_equal(st.plan["hess_ptr"], pl["hess_ptr"])
    G = [np.zeros((m, m)) for m in np.diff(pl["dof_ptr"])]
    todo = chunks(st.plan, 200)
    assert len(todo) > 2 and any(pl["disp"][c0][0] == pl["disp"][c0 - 1][0] for c0, _ in todo[1:])      # a molecule's displacements are split
    for c0, c1 in todo:
        img_ref, steps = vib_ref.images(x0, pl, c0, c1, 0.01)
        img = torch.full((st.image_atoms(c0, c1), 3), float("nan"), dtype=torch.float32, device=DEV)
        assert img.shape[0] == img_ref.shape[0]
        st.displace(c0, c1, 0.01, img)
        assert np.array_equal(img.cpu().numpy().view(np.int32), img_ref.view(np.int32))
        assert np.array_equal(st.h[c0:c1].cpu().numpy().view(np.int64), steps.view(np.int64))
        forces = rng.normal(0.0, 0.05, size=img_ref.shape).astype(cast)
        st.accumulate(c0, c1, dev(forces))
        for (b, row), val in vib_ref.rows(forces, steps, pl, c0, c1):
            G[b][row] = val
    work = st.work.cpu().numpy()
    for b, g in enumerate(G):
        got = work[pl["hess_ptr"][b]:pl["hess_ptr"][b + 1]].reshape(g.shape)
        assert np.array_equal(got.view(np.int64), g.view(np.int64)), b
    # finish: the symmetrised matrix, the asymmetry and the mass-weighted matrix, all exactly symmetric
    st.finish()
    hess, A, asym = st.hessian.cpu().numpy(), st.work.cpu().numpy(), st.asymmetry.cpu().numpy()
    for b, g in enumerate(G):
        sl = slice(pl["hess_ptr"][b], pl["hess_ptr"][b + 1])
        mol = slice(ptr[b], ptr[b + 1])
        im = np.repeat(1.0 / np.sqrt(masses[mol][pl["free"][mol]]), 3)
        H_ref, asym_ref, A_ref = vib_ref.finish(g, im)
        assert np.array_equal(hess[sl].reshape(g.shape), H_ref) and asym[b] == asym_ref
        assert np.array_equal(A[sl].reshape(g.shape), A_ref)
    assert st.header()["status"] == 0


# ---- 2. the eigensolver -----------------------------------------------------------------------------------------------------------------------------
def eig_state(ms):
    """A state whose molecule b has ms[b] / 3 free atoms of unit mass: the carrier of arbitrary symmetric matrices for nq_vib_eigh."""
    from nabladft_amd.vibrations import VibState
    ptr = np.concatenate([[0], np.cumsum([m // 3 for m in ms])])
    return VibState(ptr, torch.zeros(int(ptr[-1]), 3, dtype=torch.float64, device=DEV), np.ones(int(ptr[-1])))


def run_eigh(mats):
    st = eig_state([a.shape[0] for a in mats])
    st.work.copy_(dev(np.concatenate([a.ravel() for a in mats])))
    st.eigh(scale_modes=False)
    hp, dp = st.plan["hess_ptr"], st.plan["dof_ptr"]
    w, V = st.omega2.cpu().numpy(), st.modes.cpu().numpy()
    out = [(w[dp[b]:dp[b + 1]], V[hp[b]:hp[b + 1]].reshape(a.shape).T) for b, a in enumerate(mats)]      # eigenvectors as columns
    return out, st.sweeps.cpu().numpy(), st.status.cpu().numpy(), st


@pytest.fixture(scope="module")
def morse_hessians():
    """Mass-weighted Morse Hessians (restatement, equal masses) of compact molecules of m / 3 atoms at the minimum: six null modes (three for one atom, five for two)."""
    sizes = [m // 3 for m in EIG_SIZES]
    ptr, x0 = vib_ref.molecules(sizes, seed=31)
    table = morse_table(x0, ptr)
    ref = vib_ref.VibNumpy(ptr, x0, np.full(len(x0), C12)).run(lambda p: morse_np(p, table)[0])
    return dict(zip(EIG_SIZES, ref.A))


@pytest.fixture(scope="module")
def eig_cases(morse_hessians):
    rng = np.random.Generator(np.random.PCG64(17))
    mats, names = [], []
    for m in EIG_SIZES:
        M = rng.normal(size=(m, m))
        for kind, A in zip(KINDS, (M + M.T, np.zeros((m, m)), np.diag(rng.normal(size=m)), morse_hessians[m])):
            mats.append(np.ascontiguousarray(A))
            names.append((m, kind))
    out, sweeps, status, _ = run_eigh(mats)
    return {nm: (A, w, V, int(s), int(t)) for nm, A, (w, V), s, t in zip(names, mats, out, sweeps, status)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", EIG_SIZES)
def test_eigensolver_against_numpy(eig_cases, m, kind):
    A, w, V, sweeps, status = eig_cases[(m, kind)]
    e_val, e_res, e_orth = vib_ref.eig_errors(A, w, V)
    print(f"vib_parity eigh m={m} {kind}: eigenvalues {e_val:.3f} residual {e_res:.3f} orthogonality {e_orth:.3f} (units of m 2^-52, bound 10), sweeps {sweeps}")
    assert status == 0 and sweeps <= 30
    assert np.all(np.diff(w) >= 0)
    assert e_val <= 10.0 and e_res <= 10.0 and e_orth <= 10.0
    if kind in ("zero", "diagonal"):
        assert sweeps == 0


def test_eigensolver_above_256_pairs_per_round():
    """m = 516 is the first carrier size with more pairs per round (258) than threads: the rotation parameters take a second pass (about 3 s: the
    global-memory path is one workgroup per matrix)."""
    M = np.random.Generator(np.random.PCG64(516)).normal(size=(516, 516))
    A = M + M.T
    out, sweeps, status, _ = run_eigh([A])
    errs = vib_ref.eig_errors(A, *out[0])
    print(f"vib_parity eigh m=516 random: eigenvalues {errs[0]:.3f} residual {errs[1]:.3f} orthogonality {errs[2]:.3f} (units of m 2^-52, bound 10), sweeps {sweeps[0]}")
    assert status[0] == 0 and sweeps[0] <= 30 and max(errs) <= 10.0


@pytest.mark.parametrize("m", [126, 144])
def test_a_matrix_alone_and_among_300_others(morse_hessians, m):
    """Bitwise: the LDS path (126) and the global-memory path (144)."""
    rng = np.random.Generator(np.random.PCG64(m))
    target = morse_hessians[m]
    others = []
    for i in range(300):
        k = [3, 9, 48, 126, 150][i % 5]
        M = rng.normal(size=(k, k))
        others.append(M + M.T)
    alone, s1, t1, _ = run_eigh([target])
    crowd, s2, t2, _ = run_eigh(others[:137] + [target] + others[137:])
    assert t1[0] == 0 and not t2.any() and s1[0] == s2[137]
    assert np.array_equal(alone[0][0].view(np.int64), crowd[137][0].view(np.int64))
    assert np.array_equal(np.ascontiguousarray(alone[0][1]).view(np.int64), np.ascontiguousarray(crowd[137][1]).view(np.int64))


# ---- 3. through BatchedVibrations -------------------------------------------------------------------------------------------------------------------
def image_molecules(batch):
    """The molecule of each image and the index inside its molecule of each image atom: the test models mark molecule b with atomic number b + 1."""
    mol = batch.z[batch.ptr[:-1]] - 1
    local = torch.arange(batch.pos.shape[0], device=DEV) - batch.ptr[batch.batch]
    return mol, local


def test_quadratic_model_returns_its_matrix():
    """F = -K (x - x0) on the device: the realised step returns K within 1e-10 relative (with the nominal 2 delta the error is 2e-5: coordinates near 8 Angstrom)."""
    from nabladft_amd.vibrations import BatchedVibrations
    sizes = [3, 5, 1]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.Generator(np.random.PCG64(3))
    x0 = rng.normal(size=(9, 3)) + 8.0
    nmax = max(sizes)
    K = np.zeros((3, 3 * nmax, 3 * nmax))
    X0 = np.zeros((3, nmax, 3))
    for b, n in enumerate(sizes):
        M = rng.normal(size=(3 * n, 3 * n))
        K[b, :3 * n, :3 * n] = M + M.T
        X0[b, :n] = x0[ptr[b]:ptr[b + 1]]
    Kd, X0d = dev(K), dev(X0)

    def model(batch):
        mol, local = image_molecules(batch)
        X = X0d[mol].clone()
        X[batch.batch, local] = batch.pos.double()
        F = -torch.bmm(Kd[mol], (X - X0d[mol]).reshape(len(mol), -1, 1)).reshape(len(mol), nmax, 3)
        return torch.zeros(len(mol), dtype=torch.float64, device=DEV), F[batch.batch, local]

    vib = BatchedVibrations(calculator(model), masses=np.ones(9), images_per_call=10)
    vib.run(batch_of(ptr, x0, z=np.repeat(np.arange(3) + 1, sizes)))
    H = vib.hessian.cpu().numpy()
    for b, n in enumerate(sizes):
        got = H[vib.hess_ptr[b]:vib.hess_ptr[b + 1]].reshape(3 * n, 3 * n)
        err = np.abs(got - K[b, :3 * n, :3 * n]).max() / np.abs(K[b]).max()
        print(f"vib_parity quadratic model, {n} atoms: |H - K| / max|K| = {err:.3e} (bound 1e-10)")
        assert err <= 1e-10
    w = vib.omega2.cpu().numpy()
    assert np.abs(w[:9] - np.linalg.eigvalsh(K[0, :9, :9])).max() <= 1e-9 * np.abs(K[0]).max()
    assert not vib.status.cpu().numpy().any()


def concat_tables(tables, starts):
    kmax = max(t[0].shape[1] for t in tables)
    nbr, d0, mask = [], [], []
    for (n_, d_, m_), s in zip(tables, starts):
        n, k = n_.shape
        own = np.repeat(np.arange(n)[:, None] + s, kmax, 1)
        own[:, :k] = n_ + s
        nbr.append(own)
        d0.append(np.concatenate([d_, np.ones((n, kmax - k))], 1))
        mask.append(np.concatenate([m_, np.zeros((n, kmax - k), dtype=bool)], 1))
    return np.concatenate(nbr), np.concatenate(d0), np.concatenate(mask)


@pytest.fixture(scope="module")
def morse_case():
    """The seven compact molecules and the stressed collinear triatomic at their Morse minimum, run on the device (float32 forces out of the model) and by the
    restatement with float64 forces and with forces rounded to float32."""
    from nabladft_amd.vibrations import BatchedVibrations
    ptr7, x7 = vib_ref.molecules(vib_ref.SIZES)
    _, x3, t3 = vib_ref.collinear_molecule()
    ptr = np.concatenate([ptr7, [ptr7[-1] + 3]])
    x0 = np.concatenate([x7, x3]).astype(np.float32).astype(np.float64)          # float32-representable: the restatement and the device see the same geometry
    table = concat_tables([morse_table(x7, ptr7), t3], [0, ptr7[-1]])
    masses = np.full(len(x0), C12)
    nbr, d0, mask = dev(table[0]), dev(table[1]), dev(table[2])
    start = dev(ptr[:-1])

    def model(batch):
        mol, local = image_molecules(batch)
        shift = (batch.ptr[:-1] - start[mol])[batch.batch]                        # image atom index minus the atom's index in the original batch
        orig = local + start[mol][batch.batch]
        f = morse_torch(batch.pos.double(), (nbr[orig] + shift[:, None], d0[orig], mask[orig]))
        return torch.zeros(len(mol), dtype=torch.float32, device=DEV), f.float()

    z = np.repeat(np.arange(len(ptr) - 1) + 1, np.diff(ptr))
    runs = {}
    for scale in (1.0, 4.0):
        vib = BatchedVibrations(calculator(model), masses=masses * scale, images_per_call=256)
        vib.run(batch_of(ptr, x0, z=z))
        runs[scale] = vib
    f_of = lambda p: morse_np(p, table)[0]
    ref64 = vib_ref.VibNumpy(ptr, x0, masses).run(f_of)
    ref32 = vib_ref.VibNumpy(ptr, x0, masses).run(f_of, cast=np.float32)
    return ptr, runs, ref64, ref32


def test_morse_hessian_against_the_restatement(morse_case):
    ptr, runs, ref64, ref32 = morse_case
    vib = runs[1.0]
    H = vib.hessian.cpu().numpy()
    assert not vib.status.cpu().numpy().any() and int(vib.sweeps.max()) <= 30
    for b in range(len(ptr) - 1):
        m = 3 * int(ptr[b + 1] - ptr[b])
        got = H[vib.hess_ptr[b]:vib.hess_ptr[b + 1]].reshape(m, m)
        top = max(np.abs(ref64.hessian[b]).max(), 1e-300)
        spread = np.abs(ref64.hessian[b] - ref32.hessian[b]).max()
        err = np.abs(got - ref64.hessian[b]).max()
        print(f"vib_parity morse {m // 3} atoms: |H - H_ref| {err / top:.3e}, float32 spread {spread / top:.3e} of the largest entry (bound 10 x spread)")
        assert np.array_equal(got, got.T)
        assert err <= 10.0 * spread


def test_morse_near_zero_modes_on_the_device(morse_case):
    ptr, runs, ref64, _ = morse_case
    w = runs[1.0].omega2.cpu().numpy()
    dp = runs[1.0].dof_ptr
    expected = [3, 5, 6, 6, 6, 6, 6, 5]                                           # one atom, two atoms, ..., the collinear triatomic
    for b, want in enumerate(expected):
        k, gap = vib_ref.count_near_zero(w[dp[b]:dp[b + 1]])
        print(f"vib_parity morse {(dp[b + 1] - dp[b]) // 3} atoms: {k} near-zero modes, next at {gap:.3e} of the largest")
        assert k == want
        if b > 0:
            assert gap > 1e-2
    freqs = runs[1.0].frequencies
    assert freqs.dtype == np.complex128 and runs[1.0].energies.dtype == np.complex128
    zpe = runs[1.0].zero_point_energy
    assert zpe.shape == (8,) and zpe[0] == 0.5 * runs[1.0].energies[:3].real.sum() and np.all(zpe[1:] > 0)


def test_quadrupled_masses_halve_every_frequency(morse_case):
    _, runs, _, _ = morse_case
    f1, f4 = runs[1.0].frequencies, runs[4.0].frequencies
    assert np.abs(f4 - 0.5 * f1).max() <= 1e-12 * np.abs(f1).max()
    assert torch.equal(runs[1.0].hessian, runs[4.0].hessian)


def test_refusals():
    from nabladft_amd import _lib
    from nabladft_amd.optimization import PyGBatchwiseCalculator
    from nabladft_amd.vibrations import MAX_DOF, BatchedVibrations, VibState
    lib = _lib.load()
    calc = calculator(lambda b: (torch.zeros(1, device=DEV), torch.zeros_like(b.pos)))
    with pytest.raises(NotImplementedError):
        BatchedVibrations(calc, nfree=4)
    with pytest.raises(NotImplementedError):
        PyGBatchwiseCalculator(lambda b: None, DEV, energy_unit="eV", position_unit="Ang")
    with pytest.raises(NotImplementedError):
        PyGBatchwiseCalculator(lambda b: None, DEV, energy_unit="Hartree", position_unit="Bohr")
    n = MAX_DOF // 3 + 1
    with pytest.raises(_lib.NablaqError) as e:
        BatchedVibrations(calc).run(batch_of(np.array([0, 4, 4 + n]), np.zeros((4 + n, 3))))
    assert e.value.code == _lib.NQ_ERR_MOL_TOO_LARGE and str(MAX_DOF) in str(e.value)
    # the library refuses it as well, and fixing one atom brings the molecule under the cap
    assert lib.nq_vib_state_bytes(n, 1, 3 * n, (3 * n) ** 2) == 0
    VibState([0, n], torch.zeros(n, 3, device=DEV), np.ones(n), fixed=[0])
    with pytest.raises(_lib.NablaqError) as e:
        VibState([0, 5, 12], torch.zeros(12, 3, device=DEV), np.zeros(12))
    assert e.value.code == _lib.NQ_ERR_ARG and "mass" in str(e.value)
    st = VibState([0, 5, 12], torch.ones(12, 3, device=DEV, dtype=torch.float64), np.ones(12))
    img = torch.zeros(st.image_atoms(0, 4), 3, device=DEV)
    for bad in ((4, 4), (-1, 3), (30, 37)):
        with pytest.raises(ValueError):
            st.displace(*bad, 0.01, img)
    with pytest.raises(ValueError):
        st.displace(0, 4, 0.01, img[:-1])
    with pytest.raises(_lib.NablaqError):
        st.displace(0, 4, 0.0, img)
    with pytest.raises(ValueError):
        st.accumulate(0, 4, torch.zeros(3, 3, device=DEV))
    # calls with other dimensions than the state was prepared for touch nothing and are reported
    torch.cuda.synchronize()
    before = st.buf.clone()
    N, B, D, P = st._dims
    assert lib.nq_vib_finish(_lib.ptr(st.buf), N, B + 1, D, P, _lib.stream_ptr()) == 0
    assert lib.nq_vib_eigh(_lib.ptr(st.buf), N, B, D, P - 9, st.n_lds, st.max_m_lds, st.max_m, 1, _lib.stream_ptr()) == 0
    with pytest.raises(RuntimeError, match="other dimensions"):
        st.header()
    assert torch.equal(before[64:], st.buf[64:])


# ---- 4. through the interface, with a real engine ---------------------------------------------------------------------------------------------------
def test_painn_normal_modes_through_the_interface(tmp_path, golden_dir):
    import nabladft_amd as nq
    from nabladft_amd.md import read_xyz, write_xyz
    from nabladft_amd.vibrations import read_summary
    from oracle import painn_ref as R
    gold = np.load(os.path.join(golden_dir, "vib_painn.npz"))
    cfg = R.PaiNNConfig(**{k: (float(v) if k == "cutoff" else int(v)) for k, v in gold["cfg"]})
    z, ptr, pos = gold["z"], gold["ptr"], gold["pos"]
    path = str(tmp_path / "start.xyz")
    write_xyz(path, z, ptr, pos.astype(np.float64))
    model = nq.PaiNN(cfg.hidden_channels, cfg.num_layers, cfg.num_rbf, cfg.cutoff, cfg.max_neighbors, {"name": "gaussian"},
                     {"name": "polynomial", "exponent": 5}, True, False, False, True, cfg.num_elements)
    model.load_state_dict(R.make_params(cfg, seed=int(gold["param_seed"])), strict=False)
    model.eval()
    work = tmp_path / "work"
    it = nq.PYGAseInterface(path, str(work), None, model, device=DEV)
    assert np.array_equal(it.positions.astype(np.float32), pos)
    it.compute_normal_modes()
    npz = np.load(str(work / "normal_modes.npz"))
    for key in ("hessian", "hess_ptr", "dof_ptr", "omega2", "modes", "asymmetry", "sweeps", "status", "energies", "frequencies", "zero_point_energy", "ptr", "z"):
        assert key in npz.files, key
    assert np.array_equal(npz["ptr"], ptr) and np.array_equal(npz["z"], z) and np.array_equal(npz["hess_ptr"], gold["hess_ptr"])
    assert not npz["status"].any() and npz["sweeps"].max() <= 30 and npz["energies"].dtype == np.complex128
    top = np.abs(gold["hessian"]).max()
    err_h, err_w = np.abs(npz["hessian"] - gold["hessian"]).max(), np.abs(npz["omega2"] - gold["omega2"]).max()
    print(f"vib_parity painn: |H - H_ref| {err_h:.3e} (float32 spread {float(gold['spread_hessian']):.3e}, largest entry {top:.3e}), "
          f"|omega2 - ref| {err_w:.3e} (spread {float(gold['spread_omega2']):.3e}), asymmetry {npz['asymmetry'].max():.3e}")
    blocks = read_summary(str(work / "normal_modes.txt"))
    assert [len(b[0]) for b in blocks] == np.diff(gold["dof_ptr"]).tolist()
    assert np.abs(np.concatenate([b[1] for b in blocks]) - npz["frequencies"]).max() <= 0.05 + 1e-9
    frames = read_xyz(str(work / "normal_modes.xyz"))
    assert len(frames) == int(gold["dof_ptr"][-1]) and np.array_equal(frames[0][0], z[:ptr[1]]) and np.array_equal(frames[-1][0], z[ptr[1]:])
    it.compute_normal_modes(write_jmol=False)
    assert err_h <= 10.0 * float(gold["spread_hessian"]) and err_w <= 10.0 * float(gold["spread_omega2"])
    with open("/proc/self/maps") as f:
        assert "libnablaq.so" in f.read()
