"""GPU: batched orbital energies (csrc/orbitals.hip through the C ABI and through nabladft_amd.orbitals) against the float64 numpy yardstick
(tests/orbitals_ref.py, whose conditions tests/test_orbitals_cpu.py pins).

Bound: 10 on every figure, in units of u = m 2^-52 -- the bound the project already holds its eigensolver to (tests/test_vib_gpu.py).  Generalized problem:
e_val relative to |H|_2 |S^-1|_2, e_res to |H|_2 |C|_2, e_orth to kappa_2(S) (``orbitals_ref.errors``); standard problem: ``vib_ref.eig_errors`` verbatim.
The numpy route itself measures up to 1.5 in these units on the cases below and a numpy emulation of the kernels' algorithm up to 1.5; ten leaves room for
another rounding order.  Seeds of the generated cases were fixed on the yardstick's own figures (its e_res <= 2), never on the kernels'.
Every test prints its figures as ``orbitals_parity ...`` lines (kept in profiles/orbitals_parity.txt)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import orbitals_ref as R
import vib_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUND = 10.0


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def pack(mats, dtype=np.float64, poison=None):
    """Per-molecule matrices -> one packed array.  ``poison``: written over the strict upper triangles, which the kernels must not read."""
    out = []
    for a in mats:
        a = np.array(a, dtype=np.float64)
        if poison is not None:
            a[np.triu_indices(a.shape[0], 1)] = poison
        out.append(a.reshape(-1))
    return np.concatenate(out).astype(dtype)


def ptrs(mats):
    m = np.array([a.shape[0] for a in mats], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(m)]), np.concatenate([[0], np.cumsum(m * m)])


def unpack(orb_ptr, pack_ptr, eps, coeff):
    """Device results -> per-molecule (eps [m], C [m, m] with the orbitals as columns) on the host."""
    eps, coeff = eps.cpu().numpy(), coeff.cpu().numpy()
    out = []
    for b in range(len(orb_ptr) - 1):
        m = int(orb_ptr[b + 1] - orb_ptr[b])
        out.append((eps[orb_ptr[b]:orb_ptr[b + 1]].copy(), coeff[pack_ptr[b]:pack_ptr[b + 1]].reshape(m, m).T.copy()))
    return out


def py_solve(Hs, Ss, dtype=np.float64, poison=None):
    from nabladft_amd.orbitals import BatchedOrbitals
    op, pp = ptrs(Hs)
    orb = BatchedOrbitals(op, DEV).solve(dev(pack(Hs, dtype, poison)), None if Ss is None else dev(pack(Ss, dtype, poison)))
    return orb, unpack(op, pp, orb.energies, orb.coefficients)


class AbiState:
    """The C ABI with nothing of nabladft_amd.orbitals in between: one torch buffer, raw calls."""

    def __init__(self, orb_ptr):
        from nabladft_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        self.op = np.ascontiguousarray(np.asarray(orb_ptr, dtype=np.int32))
        m = np.diff(self.op).astype(np.int64)
        self.dims = (len(m), int(self.op[-1]), int((m * m).sum()))
        nbytes = self.lib.nq_orb_state_bytes(*self.dims)
        assert nbytes > 0
        self.off = (C.c_size_t * 11)()
        assert self.lib.nq_orb_state_layout(*self.dims, self.off) == 0
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.plan = (C.c_int32 * 2)()
        rc = self.lib.nq_orb_init(_lib.ptr(self.buf), nbytes, self.op.ctypes.data_as(C.c_void_p), *self.dims, self.plan, _lib.stream_ptr())
        assert rc == 0, self.lib.nq_last_error()

    def part(self, i, dtype, count):
        size = torch.empty(0, dtype=dtype).element_size()
        return self.buf[self.off[i]:self.off[i] + count * size].view(dtype)

    header = property(lambda self: self.part(0, torch.int32, 16))
    status = property(lambda self: self.part(4, torch.int32, self.dims[0]))
    info = property(lambda self: self.part(5, torch.int32, self.dims[0]))
    iters = property(lambda self: self.part(6, torch.int32, self.dims[0]))
    eps = property(lambda self: self.part(7, torch.float64, self.dims[1]))
    coeff = property(lambda self: self.part(8, torch.float64, self.dims[2]))

    def solve(self, H, S=None, dims=None):
        f64 = lambda t: int(t is not None and t.dtype == torch.float64)
        return self.lib.nq_orb_solve(self.L.ptr(self.buf), *(dims or self.dims), self.L.ptr(H), f64(H), self.L.ptr(S), f64(S), self.L.stream_ptr())


def abi_solve(Hs, Ss, dtype=np.float64):
    op, pp = ptrs(Hs)
    st = AbiState(op)
    assert st.solve(dev(pack(Hs, dtype)), None if Ss is None else dev(pack(Ss, dtype))) == 0
    return st, unpack(op, pp, st.eps, st.coeff)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def seed_of(m, i):
    return 2000 + 7 * m + i


@functools.lru_cache(maxsize=None)
def general_batch():
    """Every (m, kappa0) of the issue's table in shuffled order -> (Hs, Ss)."""
    cases = [(m, k0, seed_of(m, i)) for m in R.SIZES for i, k0 in enumerate(R.KAPPAS)]
    order = np.random.Generator(np.random.PCG64(17)).permutation(len(cases))
    pairs = [R.case(*cases[i]) for i in order]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@functools.lru_cache(maxsize=None)
def db_problems():
    from nabladft_amd.data import HamiltonianDatabase
    db = HamiltonianDatabase(os.path.join(GOLDEN, "hamiltonian_db_6.db"))
    sym = lambda a: np.tril(a.astype(np.float64)) + np.tril(a.astype(np.float64), -1).T
    return [(sym(db[i][4]), sym(db[i][5]), db[i][0]) for i in range(len(db))]


def check_general(tag, Hs, Ss, sols, status, iters):
    worst = np.zeros(3)
    for b, (H, S) in enumerate(zip(Hs, Ss)):
        eps, Cm = sols[b]
        m = H.shape[0]
        fig = np.array(R.errors(H, S, eps, Cm))
        worst = np.maximum(worst, fig)
        print(f"orbitals_parity {tag} b={b} m={m} e_val {fig[0]:.3f} e_res {fig[1]:.3f} e_orth {fig[2]:.3f} iters {int(iters[b])}")
        assert np.all(fig <= BOUND), (tag, b, m, fig)
        assert np.all(np.diff(eps) >= 0.0), (tag, b)
        assert status[b] == 0 and 0 <= iters[b] <= 60 * m, (tag, b, status[b], iters[b])
        assert np.array_equal(R.sign_fixed(Cm), Cm), (tag, b)
    print(f"orbitals_parity {tag} worst e_val {worst[0]:.3f} e_res {worst[1]:.3f} e_orth {worst[2]:.3f}")


# ---- 1. generalized problem -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_generalized_problem(dtype):
    """One batch with every (m, kappa0), float64 input; the same batch as float32 input against ``solve`` of the float32-rounded matrices.  Through the
    Python classes (strict upper triangles poisoned: only j <= i is read) and through the raw C ABI, which must agree bit for bit."""
    Hs, Ss = general_batch()
    dt = np.dtype(dtype).type
    orb, sols = py_solve(Hs, Ss, dt, poison=1e30)
    if dtype == "float32":
        Hs, Ss = [h.astype(np.float32).astype(np.float64) for h in Hs], [s.astype(np.float32).astype(np.float64) for s in Ss]
    orb.check()
    check_general(f"general {dtype}", Hs, Ss, sols, orb.status.cpu().numpy(), orb.iters.cpu().numpy())
    st, sols_abi = abi_solve(Hs, Ss, dt)
    for (e1, c1), (e2, c2) in zip(sols, sols_abi):
        assert same_bits(e1, e2) and same_bits(c1, c2)
    eps_list, c_list = orb.per_molecule()
    assert all(same_bits(e.cpu().numpy(), s[0]) and same_bits(c.cpu().numpy(), s[1]) for e, c, s in zip(eps_list, c_list, sols))


# ---- 2. standard problem --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zero", "diagonal", "clustered"])
def test_standard_problem(kind):
    sizes = [1, 2, 3, 5, 64, 65, 257]
    As = [R.standard(kind, m, 300 + m) for m in sizes]
    orb, sols = py_solve(As, None, poison=1e30)
    orb.check()
    status, iters = orb.status.cpu().numpy(), orb.iters.cpu().numpy()
    for b, A in enumerate(As):
        w, V = sols[b]
        fig = vib_ref.eig_errors(A, w, V)
        print(f"orbitals_parity standard {kind} m={A.shape[0]} e_val {fig[0]:.3f} e_res {fig[1]:.3f} e_orth {fig[2]:.3f} iters {int(iters[b])}")
        assert max(fig) <= BOUND, (kind, A.shape[0], fig)
        assert status[b] == 0 and np.all(np.diff(w) >= 0.0)
        if kind in ("zero", "diagonal"):
            assert iters[b] == 0
            assert same_bits(w, np.sort(np.diag(A)))
            assert np.array_equal(np.abs(V).sum(0), np.ones(A.shape[0])) and np.array_equal(np.abs(V).sum(1), np.ones(A.shape[0]))   # a permutation matrix
            assert np.array_equal(A @ V, V * w[None, :])


# ---- 3. sizes that change the code path ---------------------------------------------------------------------------------------------------------------
def test_conformer_size_with_database_molecules():
    """m = 412 (a 42-atom def2-SVP conformer's size: every loop over a row takes several passes) in one batch with the six database molecules,
    five of which have a positive definite overlap."""
    probs = db_problems()
    H412, S412 = R.case(412, 1e2, seed_of(412, 1))
    Hs, Ss = [p[0] for p in probs[:3]] + [H412] + [p[0] for p in probs[3:]], [p[1] for p in probs[:3]] + [S412] + [p[1] for p in probs[3:]]
    orb, sols = py_solve(Hs, Ss, np.float64)
    status, info = orb.status.cpu().numpy(), orb.info.cpu().numpy()
    # the overlap of the database's last molecule has a negative eigenvalue (tests/test_orbitals_cpu.py): reported, not solved
    assert np.linalg.eigvalsh(Ss[6])[0] < 0.0 and status[6] == 1 and 1 <= info[6] <= 62 and np.isnan(sols[6][0]).all() and np.isnan(sols[6][1]).all()
    with pytest.raises(RuntimeError, match="molecule 6"):
        orb.check()
    check_general("conformer+db", Hs[:6], Ss[:6], sols[:6], status, orb.iters.cpu().numpy())


def test_largest_size():
    """One matrix at the cap, m = 1024: two components per thread in the QL sweeps, the matrix beyond one XCD's L2."""
    H, S = R.case(1024, 1e2, 4242)
    orb, sols = py_solve([H], [S], np.float64)
    check_general("m=1024", [H], [S], sols, orb.status.cpu().numpy(), orb.iters.cpu().numpy())


# ---- 4. bitwise ---------------------------------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_batch_independent():
    H65, S65 = R.case(65, 1e2, seed_of(65, 1))
    H257, S257 = R.case(257, 1e4, seed_of(257, 2))
    _, a = py_solve([H65], [S65])
    _, b = py_solve([H65], [S65])
    assert same_bits(a[0][0], b[0][0]) and same_bits(a[0][1], b[0][1])
    _, alone257 = py_solve([H257], [S257])
    others = [R.case(m, k0, 700 + i) for i, (m, k0) in enumerate([(5, 1.0), (24, 1e2), (63, 1e4), (64, 1.0), (3, 1e2)] * 8)]
    Hs, Ss = [o[0] for o in others], [o[1] for o in others]
    Hs.insert(7, H65), Ss.insert(7, S65)
    Hs.insert(30, H257), Ss.insert(30, S257)
    assert len(Hs) == 42
    orb, sols = py_solve(Hs, Ss)
    orb.check()
    assert same_bits(sols[7][0], a[0][0]) and same_bits(sols[7][1], a[0][1])
    assert same_bits(sols[30][0], alone257[0][0]) and same_bits(sols[30][1], alone257[0][1])
    for eps, Cm in sols:
        assert np.array_equal(R.sign_fixed(Cm), Cm)
        assert np.all(Cm[np.argmax(np.abs(Cm), axis=0), np.arange(Cm.shape[1])] > 0.0)
    # the standard problem as well
    A = R.standard("random", 65, 9)
    _, s1 = py_solve([A], None)
    _, s2 = py_solve([R.standard("random", 24, 1), A, R.standard("clustered", 64, 2)], None)
    assert same_bits(s1[0][0], s2[1][0]) and same_bits(s1[0][1], s2[1][1])


# ---- 5. handled failure ---------------------------------------------------------------------------------------------------------------------------
def test_overlap_not_positive_definite_is_reported_per_molecule():
    good = [R.case(m, 1e2, 800 + m) for m in (24, 65, 5, 63)]
    Hb, Sb = R.case(64, 1e2, 864)
    w, Q = np.linalg.eigh(Sb)
    w[3] = -0.25
    Sb = (Q * w[None, :]) @ Q.T
    Sb = 0.5 * (Sb + Sb.T)
    Hs, Ss = [g[0] for g in good], [g[1] for g in good]
    _, clean = py_solve(Hs, Ss)
    Hs.insert(2, Hb), Ss.insert(2, Sb)
    orb, sols = py_solve(Hs, Ss)
    status, info = orb.status.cpu().numpy(), orb.info.cpu().numpy()
    print(f"orbitals_parity failure status {status.tolist()} info {info.tolist()}")
    assert status.tolist() == [0, 0, 1, 0, 0]
    assert 1 <= info[2] <= 64 and np.all(info[[0, 1, 3, 4]] == 0)
    assert np.isnan(sols[2][0]).all() and np.isnan(sols[2][1]).all()
    for got, ref in zip(sols[:2] + sols[3:], clean):
        assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])
    with pytest.raises(RuntimeError, match="molecule 2"):
        orb.check()


# ---- 6. refusals before device work -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import BatchedOrbitals, OrbitalState
    lib = _lib.load()
    with pytest.raises(_lib.NablaqError) as ei:
        BatchedOrbitals([0, 5, 1030], DEV)
    assert ei.value.code == _lib.NQ_ERR_MOL_TOO_LARGE
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    plan = (C.c_int32 * 2)()
    big = np.array([0, 5, 1030], dtype=np.int32)
    rc = lib.nq_orb_init(_lib.ptr(buf), buf.numel(), big.ctypes.data_as(C.c_void_p), 2, 1030, 25 + 1025 * 1025, plan, _lib.stream_ptr())
    assert rc == _lib.NQ_ERR_MOL_TOO_LARGE and b"1025" in lib.nq_last_error()
    op = np.array([0, 3, 8], dtype=np.int32)                     # packs to 9 + 25 = 34
    for M, P in ((8, 35), (8, 33), (9, 34)):                     # pack_ptr / orb_ptr disagree
        rc = lib.nq_orb_init(_lib.ptr(buf), buf.numel(), op.ctypes.data_as(C.c_void_p), 2, M, P, plan, _lib.stream_ptr())
        assert rc == _lib.NQ_ERR_ARG, (M, P)
    assert int(buf.sum()) == 0                                   # none of the refused calls wrote to the device
    assert lib.nq_orb_state_bytes(0, 0, 0) == 0 and lib.nq_orb_state_bytes(2, 1, 1) == 0
    with pytest.raises(ValueError):
        BatchedOrbitals([0, 3, 8], DEV).solve(torch.zeros(33, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="MI355X only"):
        BatchedOrbitals([0, 3, 8], DEV).solve(torch.zeros(34, dtype=torch.float64))
    # a call with other dimensions than init: outputs untouched, header status set
    st = AbiState(op)
    st.eps.fill_(float("nan")), st.coeff.fill_(float("nan"))
    st.status.fill_(7)
    H = dev(pack([R.standard("random", 3, 1), R.standard("random", 5, 2)]))
    assert st.solve(torch.cat([H, H]), None, dims=(2, 8, 36)) == 0
    torch.cuda.synchronize()
    assert int(st.header[4]) == -2
    assert torch.isnan(st.eps).all() and torch.isnan(st.coeff).all() and st.status.tolist() == [7, 7]
    ost = OrbitalState(op, DEV)
    ost.header_dev[4] = -2
    with pytest.raises(RuntimeError, match="other dimensions"):
        ost.header()
    assert st.solve(H, None) == 0                                # the right dimensions still work on that state
    torch.cuda.synchronize()
    assert st.status.tolist() == [0, 0] and not torch.isnan(st.eps).any()


# ---- 7. frontier and compare ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compare_batch():
    """(target H, predicted H, S, n_occ) per molecule: the predicted matrix is the target plus symmetric noise."""
    out = []
    for m in (5, 24, 65, 141):
        for i, k0 in enumerate(R.KAPPAS):
            H, S = R.case(m, k0, seed_of(m, i))
            N = np.random.Generator(np.random.PCG64(99 + m)).normal(size=(m, m))
            out.append((H, H + 0.02 * (N + N.T), S, max(1, m // 3)))
    return out


def check_compare(tag, probs, figs, sol_p, sol_t, general=True):
    worst = np.zeros(3)
    for b, (H, Hp, S, no) in enumerate(probs):
        m = H.shape[0]
        S_ = S if general else None
        e_t, C_t = R.solve(H, S_)
        e_p, C_p = R.solve(Hp, S_)
        assert np.diff(e_t[:no + 1]).min() > 1e-3 and np.diff(e_p[:no + 1]).min() > 1e-3      # the occupied levels are separated
        ref = R.compare(e_p, C_p, e_t, C_t, S_, no)
        own = R.compare(sol_p[b][0], sol_p[b][1], sol_t[b][0], sol_t[b][1], S_, no)          # the kernel's arithmetic on the kernel's own solutions
        nH, nSi, _ = R.spectral(H, S if general else np.eye(m))
        unit = m * R.EPS * max(nH, np.linalg.norm(Hp, 2)) * nSi
        got = figs[:, b]
        d_eps = np.abs(got[[0, 1, 3, 4, 5]] - ref[[0, 1, 3, 4, 5]]).max() / unit
        d_psi = np.abs(got[[2, 6]] - ref[[2, 6]]).max()
        d_own = np.abs(got - own).max()
        worst = np.maximum(worst, [d_eps, d_psi, d_own])
        print(f"orbitals_parity compare {tag} m={m} eps figures {d_eps:.3f} u psi_sim {d_psi:.2e} own {d_own:.2e} (psi_sim_occ {ref[2]:.4f})")
        assert d_eps <= BOUND and d_psi <= 1e-10 and d_own <= 1e-12, (tag, b, d_eps, d_psi, d_own)
    print(f"orbitals_parity compare {tag} worst eps {worst[0]:.3f} u psi {worst[1]:.2e} own {worst[2]:.2e}")


@pytest.mark.parametrize("general", [True, False])
def test_frontier_and_compare(general):
    probs = compare_batch()
    Ht, Hp, Ss, no = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs], [p[3] for p in probs]
    S_arg = Ss if general else None
    Sp = dev(pack(Ss)) if general else None
    targ, sol_t = py_solve(Ht, S_arg)
    pred, sol_p = py_solve(Hp, S_arg)
    homo, lumo, gap = [t.cpu().numpy() for t in pred.frontier(no)]
    for b, (H, Hpb, S, n) in enumerate(probs):
        ref = R.frontier(R.solve(Hpb, S if general else None)[0], n)
        unit = H.shape[0] * R.EPS * np.linalg.norm(Hpb, 2) * (R.spectral(H, S)[1] if general else 1.0)
        assert np.abs(np.array([homo[b], lumo[b], gap[b]]) - np.array(ref)).max() <= BOUND * unit
        assert same_bits(np.array([homo[b], lumo[b]]), sol_p[b][0][[n - 1, n]]) and gap[b] == lumo[b] - homo[b]
    figs = pred.compare(targ, no, Sp).cpu().numpy()
    check_compare("general" if general else "standard", probs, figs, sol_p, sol_t, general)
    # a solution against itself: similarity one, no energy error; every orbital occupied: no LUMO
    full = [p[0].shape[0] for p in probs]
    self_figs = targ.compare(targ, full, Sp).cpu().numpy()
    assert np.abs(self_figs[2] - 1.0).max() <= 1e-12 and np.abs(self_figs[6] - 1.0).max() <= 1e-12
    assert np.all(self_figs[[0, 1, 3]] == 0.0) and np.isnan(self_figs[[4, 5]]).all()
    h, l, g = targ.frontier(full)
    assert torch.isnan(l).all() and torch.isnan(g).all() and not torch.isnan(h).any()
    with pytest.raises(ValueError, match="outside 1..m"):
        targ.frontier([f + 1 for f in full])


# ---- 8. OrbitalErrors -------------------------------------------------------------------------------------------------------------------------------
def test_orbital_errors_over_two_batches():
    from nabladft_amd.orbitals import OrbitalErrors
    probs = compare_batch()
    acc, rows = OrbitalErrors(), []
    for part in (probs[:5], probs[5:]):
        op, _ = ptrs([p[0] for p in part])
        # atoms that give the n_occ of the plan: n_occ - 1 helium atoms and one more
        z, ptr = [], [0]
        for p in part:
            z += [2] * p[3]
            ptr.append(len(z))
        acc.update(dev(pack([p[1] for p in part])), dev(pack([p[0] for p in part])), dev(pack([p[2] for p in part])), op, torch.tensor(z), torch.tensor(ptr))
        for H, Hp, S, no in part:
            e_t, C_t = R.solve(H, S)
            e_p, C_p = R.solve(Hp, S)
            rows.append((R.compare(e_p, C_p, e_t, C_t, S, no), H.shape[0] * R.EPS * max(np.linalg.norm(H, 2), np.linalg.norm(Hp, 2)) * R.spectral(H, S)[1]))
    got = acc.compute()
    ref = np.mean([r[0] for r in rows], axis=0)
    unit = np.mean([r[1] for r in rows])
    assert tuple(got) == R.FIGURES
    for i, name in enumerate(R.FIGURES):
        d = abs(got[name] - ref[i])
        print(f"orbitals_parity errors {name} {got[name]:.12g} ref {ref[i]:.12g}")
        assert d <= (1e-10 if name.startswith("psi") else BOUND * unit), (name, got[name], ref[i])
    acc.reset()
    with pytest.raises(RuntimeError):
        acc.compute()
    with pytest.raises(ValueError, match="open shells"):
        acc.update(dev(pack([probs[0][1]])), dev(pack([probs[0][0]])), None, [0, 5], torch.tensor([1]), torch.tensor([0, 1]))


def test_orbital_errors_reports_a_failure_in_an_earlier_batch():
    """The database's 62-orbital molecule (indefinite overlap) sits in the FIRST of two batches: ``compute()`` must raise and name it, not average the rest."""
    from nabladft_amd.orbitals import OrbitalErrors
    probs = db_problems()
    assert np.linalg.eigvalsh(probs[5][1])[0] < 0.0
    z_of = lambda zs: [int(a) for a in zs]

    def feed(acc, which):
        part = [probs[i] for i in which]
        op, _ = ptrs([p[0] for p in part])
        z = sum((z_of(p[2]) for p in part), [])
        ptr = np.concatenate([[0], np.cumsum([len(p[2]) for p in part])])
        H, S = dev(pack([p[0] for p in part])), dev(pack([p[1] for p in part]))
        acc.update(dev(pack([p[0] + 0.01 * p[1] for p in part])), H, S, op, torch.tensor(z), torch.tensor(ptr))

    acc = OrbitalErrors()
    feed(acc, [0, 5, 1])
    feed(acc, [2, 3, 4])
    with pytest.raises(RuntimeError, match=r"batch 0, predicted Hamiltonian, molecule 1: the overlap matrix is not positive definite \(Cholesky pivot \d+ of 62"):
        acc.compute()
    with pytest.raises(RuntimeError, match="batch 0"):           # still there: only reset() forgets
        acc.compute()
    acc.reset()
    assert acc._flags == [] and not hasattr(acc, "_last")          # no solver state is kept alive
    feed(acc, [0, 1])
    feed(acc, [2, 3, 4])
    got = acc.compute()
    # H + 0.01 S shifts every eigenvalue by 0.01 and keeps every orbital
    assert abs(got["eps_mae_occ"] - 0.01) < 1e-9 and abs(got["eps_mae_all"] - 0.01) < 1e-9 and abs(got["psi_sim_occ"] - 1.0) < 1e-9
    assert got["homo_abs_err"] < 0.01 + 1e-9 and got["gap_abs_err"] < 1e-9


# ---- 9. PhiSNet -------------------------------------------------------------------------------------------------------------------------------------
def test_phisnet_opt_in():
    """A small network on two database molecules.  The results are cast to the dtype of the positions (float32), which cannot carry figures measured in
    units of m 2^-52: the three figures are asserted on the float64 solution the call also returns (``results["orbitals"]``) against the returned float32
    matrices, and ``orbital_energies`` / ``orbital_coefficients`` must be exactly that solution cast and laid out as documented."""
    from nabladft_amd.data import HamiltonianDataset
    from nabladft_amd.phisnet import NeuralNetwork
    ds = HamiltonianDataset(os.path.join(GOLDEN, "hamiltonian_db_6.db"))
    torch.manual_seed(0)
    net = NeuralNetwork(max_orbitals=ds.max_orbitals * 2, order=2, num_features=32, num_basis_functions=8, num_modules=1, num_residual_pre_x=1,
                        num_residual_post_x=1, num_residual_pre_vi=1, num_residual_pre_vj=1, num_residual_post_v=1, num_residual_output=1, num_residual_pc=1,
                        num_residual_pn=1, num_residual_ii=1, num_residual_ij=1, num_residual_full_ii=1, num_residual_full_ij=1, num_residual_core_ii=1,
                        num_residual_core_ij=1, num_residual_over_ij=1, basis_functions="exp-bernstein", cutoff=8.0, activation="swish").cuda()
    with torch.no_grad():                 # a fresh network's output layers are zero (diagonal matrices, nothing to solve): give them small weights
        gen = torch.Generator(device="cuda").manual_seed(5)
        for p in net.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(0.02 * torch.randn(p.shape, generator=gen, device=p.device, dtype=p.dtype))
    b = ds.collate_fn([0, 1])
    batch = {k: (v.cuda() if torch.is_tensor(v) and k != "molecule_size" else v) for k, v in b.items()}
    assert net.calculate_orbitals is False
    with torch.no_grad():
        off = net(batch)
        net.calculate_orbitals = True
        on = net(batch)
    norb = off["full_hamiltonian"].shape[-1]
    assert tuple(off["orbital_energies"].shape) == (1, norb) and tuple(off["orbital_coefficients"].shape) == (1, norb, norb)
    assert float(off["orbital_energies"].abs().max()) == 0.0 and float(off["orbital_coefficients"].abs().max()) == 0.0 and "orbitals" not in off
    for k, v in off.items():
        if torch.is_tensor(v) and not k.startswith("orbital_"):
            assert torch.equal(v, on[k]), k
    assert on["orbital_energies"].dtype == off["orbital_energies"].dtype and tuple(on["orbital_energies"].shape) == (1, norb)
    assert tuple(on["orbital_coefficients"].shape) == (1, norb, norb) and not on["orbital_energies"].requires_grad
    orb = on["orbitals"].check()
    Hd, Sd = on["full_hamiltonian"][0].double().cpu().numpy(), on["overlap_matrix"][0].double().cpu().numpy()
    op, pp = orb.orb_ptr, orb.pack_ptr
    sols = unpack(op, pp, orb.energies, orb.coefficients)
    dense = np.zeros((norb, norb))
    Hs, Ss = [], []
    for bb in range(len(op) - 1):
        sl = slice(int(op[bb]), int(op[bb + 1]))
        sym = lambda a: np.tril(a) + np.tril(a, -1).T
        Hs.append(sym(Hd[sl, sl])), Ss.append(sym(Sd[sl, sl]))
        dense[sl, sl] = sols[bb][1]
        assert R.spectral(Hs[-1], Ss[-1])[2] <= 1e5                      # the untrained network's overlap is conditioned like the generated cases
    check_general("phisnet", Hs, Ss, sols, orb.status.cpu().numpy(), orb.iters.cpu().numpy())
    assert int(orb.iters.min()) > 0                                          # the predicted matrices are not diagonal: the solver had work to do
    dt = on["orbital_energies"].dtype
    assert torch.equal(on["orbital_energies"][0].cpu(), torch.from_numpy(np.concatenate([s[0] for s in sols])).to(dt))
    assert torch.equal(on["orbital_coefficients"][0].cpu(), torch.from_numpy(dense).to(dt))
    # the overlap head off: the standard problem
    net.calculate_overlap_matrix = False
    with torch.no_grad():
        std = net(batch)
    sols = unpack(op, pp, std["orbitals"].energies, std["orbitals"].coefficients)
    for bb, H in enumerate(Hs):
        fig = vib_ref.eig_errors(H, sols[bb][0], sols[bb][1])
        print(f"orbitals_parity phisnet standard m={H.shape[0]} e_val {fig[0]:.3f} e_res {fig[1]:.3f} e_orth {fig[2]:.3f}")
        assert max(fig) <= BOUND
