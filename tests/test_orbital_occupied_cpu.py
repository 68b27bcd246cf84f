"""CPU: the numpy restatement of the occupied levels without a full solve (tests/orbital_occupied_ref.py: pivoted Cholesky factor of the projector,
``Q Ht Q^T``, an ``n_occ x n_occ`` eigenproblem, back-transform) against ``np.linalg.eigh`` / ``scipy.linalg.eigh``; ``OccupiedEnergyLoss`` against
``OrbitalEnergyLoss(kind, "occupied")``; the public surface and the Python-side refusals.

Units: ``U_eps = m 2^-52 kappa_2(S) (eps_max - eps_min)`` for a level (at m = 1 the spread is zero: the floor ``2^-52 |eps|``), ``U_eps / sep max(1, max|c c^T|)`` for
``c c^T`` (``sep``: the distance from the level to its nearest neighbour in the whole spectrum), ``u_Q = m^(3/2) 2^-52`` for the three defects of the factor
(``Q Q^T - I``, ``Q^T Q - X``, the left-over diagonal), ``(u_Q + 2 m 2^-52) kappa_2(S)`` for ``C S C^T - I`` (``orbital_occupied_ref.csc_unit``: ``u_Q kappa_2(S)`` alone is under two ulps at m <= 2, less than the two m-term
products of the check itself round by; the restatement measured 1.06 of it there, so the unit was wrong and carries the check's own rounding now).  Bound 10 units for every case, the project's standing margin; the
restatement's own worst over the grid has to stay <= 2 units (<= 1 for ``C S C^T``), which ``test_zz_worst_figures_of_the_grid`` asserts after the grid ran and
prints in the lines that profiles/orbital_occupied_parity.txt keeps."""
import inspect

import numpy as np
import pytest
import scipy.linalg
import torch

import orbital_density_ref as DR
import orbital_frontier_ref as FR
import orbital_occupied_ref as OR
import orbital_purify_ref as PR

BOUND = 10.0
SIZES = (1, 2, 3, 5, 16, 17, 33, 64, 65, 130, 412)
WORST = {}                      # figure -> the worst over everything the grid tests saw


def occupations(m):
    return sorted({n for n in (1, m // 5, m // 2, m - 1, m) if 1 <= n <= m})


def note(**figs):
    for k, v in figs.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))          # ("pivot_times_m_min" is kept as a minimum by its own line)


def figures(res, X, Ht, n, ev, Cref, S, kap):
    """The figures of one result against the reference levels ``ev`` and vectors ``Cref`` (columns) -> dict, in units."""
    m = Ht.shape[0]
    f = res["factor"]
    Q = f["Q"]
    uq = OR.q_unit(m)
    spread = ev[-1] - ev[0]
    u = OR.level_unit(m, spread, kap) if m > 1 else 2.0 ** -52 * abs(ev[0])
    out = dict(qqt=np.abs(Q @ Q.T - np.eye(n)).max() / uq, qtq=np.abs(Q.T @ Q - X).max() / uq, left=f["defect"] / uq,
               level=np.abs(res["eps"][:n] - ev[:n]).max() / u)
    C = res["C"][:n]
    cc = 0.0
    for k in range(n):
        ref = np.outer(Cref[:, k], Cref[:, k])
        cc = max(cc, np.abs(np.outer(C[k], C[k]) - ref).max() / (u / FR.separation(ev, k) * max(1.0, np.abs(ref).max())))
    out["cct"] = cc
    Sm = np.eye(m) if S is None else S
    out["csc"] = np.abs(C @ Sm @ C.T - np.eye(n)).max() / OR.csc_unit(m, kap)
    return out


@pytest.mark.parametrize("m", SIZES)
def test_restatement_against_eigh_on_the_standard_problem(m):
    worst = {}
    for n in occupations(m):
        for seed in range(3 if m <= 130 else 1):
            rng = np.random.default_rng(1000 * m + 10 * n + seed)
            H, _ = FR.random_hamiltonian(rng, m, n, gap=0.3 if seed % 2 == 0 else 0.01)
            if m == 1:
                H = np.array([[-3.5 + seed]])                          # the generator's single level is 0: no floor to compare with
            ev, U = np.linalg.eigh(H)
            for source in ("eigh", "sp2"):
                if source == "eigh":
                    X = PR.lower_sym(U[:, :n] @ U[:, :n].T)
                else:
                    sol = PR.purify(H, n)
                    assert sol["status"] == 0
                    X = sol["X"]
                res = OR.occupied(H, X, n)
                assert res["status"] == 0 and np.isnan(res["eps"][n:]).all() and np.isnan(res["C"][n:]).all(), (m, n, seed, source)
                assert res["factor"]["min_pivot"] >= (1.0 - 1e-9) / m, (m, n, seed, source, res["factor"]["min_pivot"] * m)
                assert len(set(res["factor"]["pivots"])) == n
                fig = figures(res, X, H, n, ev, U, None, 1.0)
                assert max(fig.values()) <= BOUND, (m, n, seed, source, fig)
                note(**fig)
                WORST["pivot_times_m_min"] = min(WORST.get("pivot_times_m_min", np.inf), res["factor"]["min_pivot"] * m)
                for k, v in fig.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(f"orbital_occupied_parity restatement standard m={m}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


GENERAL = [(m, n, 0.3, kap0, 200 + m + n) for m in (2, 3, 17, 65, 130) for n in sorted({1, m // 2, m}) for kap0 in (1e2, 1e4)]


@pytest.mark.parametrize("case", GENERAL, ids=[f"m{c[0]}-n{c[1]}-k{c[3]:g}" for c in GENERAL])
def test_restatement_against_scipy_on_the_generalized_problem(case):
    m, n = case[0], case[1]
    H, S = DR.gapped_case(*case)
    ev, Cref = scipy.linalg.eigh(H, S)
    kap = float(np.linalg.cond(S))
    res, sol = OR.from_matrices(H, S, n)
    assert sol["status"] == 0 and res["status"] == 0
    Z = PR.orthogonalizer(S)
    Ht = PR.congruence(Z, PR.lower_sym(H), False)
    fig = figures(res, sol["X"], Ht, n, ev, Cref, S, kap)
    print(f"orbital_occupied_parity restatement generalized m={m} n_occ={n} kappa={kap:.3g}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(fig.items())))
    assert max(fig.values()) <= BOUND, (case, fig)
    note(**fig)
    g = np.random.default_rng(5).standard_normal(m)
    gH, gS = OR.gradients(res, g, n)
    rH = sum(g[k] * np.outer(Cref[:, k], Cref[:, k]) for k in range(n))
    rS = -sum(g[k] * ev[k] * np.outer(Cref[:, k], Cref[:, k]) for k in range(n))
    u = OR.level_unit(m, ev[-1] - ev[0], kap) / min(FR.separation(ev, k) for k in range(n))
    assert np.abs(gH - rH).max() <= BOUND * u * max(1.0, np.abs(rH).max()) and np.abs(gS - rS).max() <= BOUND * u * max(1.0, np.abs(rS).max())


def test_zz_worst_figures_of_the_grid():
    """Runs after the grid (file order): the restatement's own worst values stay <= 2 units, ``C S C^T`` <= 1 (else the unit would be wrong)."""
    if not WORST:
        pytest.skip("the grid tests did not run in this session")
    print("orbital_occupied_parity restatement worst over the grid: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    for k in ("level", "cct", "qqt", "qtq", "left"):
        assert WORST[k] <= 2.0, (k, WORST[k])
    assert WORST["csc"] <= 1.0, WORST["csc"]
    assert WORST["pivot_times_m_min"] >= 1.0 - 1e-9


def test_two_equal_occupied_levels_compare_the_sum_of_their_projectors():
    rng = np.random.default_rng(7)
    m, n = 37, 9
    lev = np.concatenate([np.sort(rng.uniform(-20.0, -0.2, n)), np.sort(rng.uniform(0.2, 2.0, m - n))])
    lev[3] = lev[4]
    Qm = np.linalg.qr(rng.standard_normal((m, m)))[0]
    H = PR.lower_sym((Qm * lev) @ Qm.T)
    ev, U = np.linalg.eigh(H)
    sol = PR.purify(H, n)
    res = OR.occupied(H, sol["X"], n)
    u = OR.level_unit(m, lev[-1] - lev[0])
    assert res["status"] == 0 and np.abs(res["eps"][:n] - ev[:n]).max() <= BOUND * u
    pair = sum(np.outer(res["C"][k], res["C"][k]) for k in (3, 4))
    ref = sum(np.outer(U[:, k], U[:, k]) for k in (3, 4))
    sep = min(lev[3] - lev[2], lev[5] - lev[4])
    assert np.abs(pair - ref).max() <= BOUND * u / sep


def test_a_matrix_that_is_not_a_projector_of_the_rank_is_status_5():
    m = 8
    half = OR.factor(0.5 * np.eye(m), 3)                               # X = I / 2 passes three pivots of 1/2 and is caught by the left-over diagonal
    assert half["status"] == OR.STATUS_NOT_A_PROJECTOR and half["diag"].max() == 0.5 and np.isnan(half["Q"]).all()
    assert OR.factor(0.5 * np.eye(m), m)["status"] == 0               # only at n_occ = m nothing is left over: Q = I / sqrt(2), which Q Q^T shows
    assert OR.factor(0.5 / (2 * m + 1) * np.eye(m), 3)["status"] == OR.STATUS_NOT_A_PROJECTOR
    res = OR.occupied(np.diag(np.arange(8.0)), 0.01 * np.eye(m), 3)
    assert res["status"] == 5 and np.isnan(res["eps"]).all() and np.isnan(res["C"]).all() and np.isnan(res["factor"]["Q"]).all()
    rng = np.random.default_rng(3)
    U = np.linalg.qr(rng.standard_normal((m, m)))[0]
    X2 = PR.lower_sym(U[:, :2] @ U[:, :2].T)                           # rank 2, asked for 3
    f = OR.factor(X2, 3)
    assert f["status"] == OR.STATUS_NOT_A_PROJECTOR and (f["pivots"] == -1).all() and np.isnan(f["min_pivot"]) and np.isnan(f["defect"])
    nanx = X2.copy()
    nanx[0, 0] = np.nan
    assert OR.factor(np.full((m, m), np.nan), 2)["status"] == OR.STATUS_NOT_A_PROJECTOR
    assert OR.factor(np.diag([np.inf] + [0.0] * 7), 1)["status"] == OR.STATUS_NOT_A_PROJECTOR


def test_a_diagonal_projector_gives_pivots_in_index_order_and_unit_rows():
    m = 11
    keep = np.array([1, 4, 5, 9])
    X = np.zeros((m, m))
    X[keep, keep] = 1.0
    f = OR.factor(X, len(keep))
    assert f["status"] == 0 and list(f["pivots"]) == list(keep) and f["min_pivot"] == 1.0 and f["defect"] == 0.0
    assert np.array_equal(f["Q"], np.eye(m)[keep])
    Ht = np.diag(np.arange(m, 0, -1.0))
    res = OR.occupied(Ht, X, len(keep))
    assert np.array_equal(res["eps"][:4], np.sort(np.diag(Ht)[keep])) and np.array_equal(np.abs(res["C"][:4]).sum(1), np.ones(4))
    full = OR.occupied(Ht, np.eye(m), m)                               # n_occ = m: X = I
    assert full["status"] == 0 and np.array_equal(full["eps"], np.arange(1.0, m + 1)) and list(full["factor"]["pivots"]) == list(range(m))
    none = OR.occupied(Ht, np.zeros((m, m)), 0)
    assert none["status"] == 0 and np.isnan(none["eps"]).all() and np.array_equal(OR.reduce(np.zeros((0, m)), Ht), np.zeros((1, 1)))
    one = OR.occupied(np.array([[-3.5]]), np.array([[1.0]]), 1)        # m = 1
    assert one["eps"][0] == -3.5 and one["C"][0, 0] == 1.0


def test_occupied_energy_loss_against_the_orbital_energy_loss(monkeypatch):
    """The losses are plain torch; ``OrbitalEnergyLoss``'s refusal of CPU tensors is switched off for this comparison."""
    from nabladft_amd import orbital_loss as OL
    monkeypatch.setattr(OL, "_require_gpu", lambda t: None)
    rng = np.random.default_rng(11)
    op = np.array([0, 4, 9, 12, 13])
    n_occ = np.array([2, 5, 1, 1])
    full_p, full_t = rng.standard_normal(13), rng.standard_normal(13)
    k = np.arange(13) - np.repeat(op[:-1], np.diff(op))
    virt = k >= np.repeat(n_occ, np.diff(op))
    for kind in ("mae", "mse"):
        ep = torch.from_numpy(np.where(virt, np.nan, full_p)).requires_grad_(True)
        et = torch.from_numpy(np.where(virt, np.nan, full_t))
        a = OL.OccupiedEnergyLoss(kind)(ep, et, n_occ, op)
        b = OL.OrbitalEnergyLoss(kind, "occupied")(torch.from_numpy(full_p), torch.from_numpy(full_t), n_occ, op)       # the virtual slots filled
        assert abs(float(a.detach()) - float(b)) <= 4 * 2.0 ** -52 * abs(float(b)), kind
        a.backward()
        assert bool(torch.isfinite(ep.grad).all()) and bool((ep.grad[torch.from_numpy(virt)] == 0).all()) and bool((ep.grad[torch.from_numpy(~virt)] != 0).all())
    with pytest.raises(ValueError, match="kind"):
        OL.OccupiedEnergyLoss("huber")
    with pytest.raises(ValueError, match="entries"):
        OL.OccupiedEnergyLoss()(torch.zeros(12), torch.zeros(13), n_occ, op)
    with pytest.raises(ValueError, match="outside 1..m"):
        OL.OccupiedEnergyLoss()(torch.zeros(13), torch.zeros(13), [0, 5, 1, 1], op)
    assert OL.OccupiedEnergyLoss.packed is True


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib, orbital_loss as OL, orbitals as O
    for name in ("purified_occupied_energies", "OccupiedEnergyLoss", "QHNetPurifiedOrbitalLightning"):
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    for name in ("OccupiedOrbitals", "PurifiedOrbitalErrors"):
        assert getattr(nq, name) is getattr(O, name) and name in nq.__all__ and name in O.__all__, name
    sig = inspect.signature(OL.purified_occupied_energies).parameters
    assert list(sig) == ["H_packed", "S_packed", "plan_or_orb_ptr", "n_occ", "orthogonalizer", "max_iter", "solution", "return_solution"]
    assert sig["max_iter"].default == 100 and sig["solution"].default is None and sig["return_solution"].default is False
    sig = inspect.signature(O.BatchedPurification.occupied).parameters
    assert list(sig) == ["self", "transform"] and sig["transform"].default is None
    sig = inspect.signature(OL.OccupiedEnergyLoss.__init__).parameters
    assert list(sig) == ["self", "kind", "charge"] and sig["kind"].default == "mae" and sig["charge"].default == 0
    for name in ("energies", "coefficients", "weighted_gram", "density", "compare", "check"):
        assert hasattr(O.OccupiedOrbitals, name), name
    for name in ("frontier", "resp_project", "density_response", "fermi", "smeared_density", "solve"):       # occupied levels only
        assert not hasattr(O.OccupiedOrbitals, name), name
    assert O.OCCUPIED_FIGURES == ("eps_mae_occ", "similarity", "similarity_min", "homo_abs_err")
    assert inspect.signature(O.PurifiedOrbitalErrors.update) == inspect.signature(O.OrbitalErrors.update)
    assert inspect.signature(O.PurifiedOrbitalErrors.__init__).parameters["charge"].default == 0
    assert issubclass(OL.QHNetPurifiedOrbitalLightning, OL.QHNetPurifiedFrontierLightning)
    assert OL.QHNetPurifiedOrbitalLightning.KEYS == OL.QHNetPurifiedFrontierLightning.KEYS + ("occupied_energies",)
    assert "occupied_energies" not in OL.QHNetPurifiedFrontierLightning.KEYS                                # the parent is unchanged
    assert inspect.signature(OL.QHNetPurifiedOrbitalLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    lib = _lib.load()
    for sym in ("nq_orb_occ_factor", "nq_orb_occ_reduce", "nq_orb_occ_back"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert lib.nq_abi_version() == 17 and _lib.ABI_VERSION == 17


def test_python_side_refusals():
    import nabladft_amd as nq
    from nabladft_amd import orbitals as O
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.purified_occupied_energies(torch.zeros(4, requires_grad=True), None, [0, 2], [1])
    pur = O.BatchedPurification.__new__(O.BatchedPurification)       # no device: the order of the calls is checked before any launch
    pur._max_iter = None
    with pytest.raises(RuntimeError, match="purify\\(\\) first"):
        pur.occupied()
    with pytest.raises(RuntimeError, match="before any update"):
        O.PurifiedOrbitalErrors().compute()
    with pytest.raises(RuntimeError, match="MI355X only"):
        O.PurifiedOrbitalErrors().update(torch.zeros(4), torch.zeros(4), None, [0, 2], [1], [0, 1])
    occ = O.OccupiedOrbitals.__new__(O.OccupiedOrbitals)            # compare() refuses anything but another OccupiedOrbitals before it touches a device
    with pytest.raises(TypeError, match="OccupiedOrbitals"):
        occ.compare(object())


class _Hp:
    def __init__(self, losses, coefs):
        self.losses, self.loss_coefs = losses, coefs


def test_the_task_still_refuses_orbital_energies():
    from nabladft_amd import orbital_loss as OL
    task = OL.QHNetPurifiedOrbitalLightning.__new__(OL.QHNetPurifiedOrbitalLightning)
    losses = {"hamiltonian": OL.OccupiedEnergyLoss(), "orbital_energies": OL.OrbitalEnergyLoss(), "occupied_energies": OL.OccupiedEnergyLoss()}
    object.__setattr__(task, "_hp", _Hp(losses, {"hamiltonian": 1.0, "orbital_energies": 1.0, "occupied_energies": 1.0}))
    type(task).hparams = property(lambda self: self._hp)
    try:
        task._packed = lambda: True
        with pytest.raises(ValueError, match="occupied orbital energies only"):
            task._evaluate(None)
        task._hp.loss_coefs["occupied_energies"] = 0.0             # the parent's step and the parent's refusal
        with pytest.raises(ValueError, match="no orbital energies"):
            task._evaluate(None)
    finally:
        del type(task).hparams
