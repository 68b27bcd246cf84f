"""CPU: the numpy restatement of the frontier levels without a solve (tests/orbital_frontier_ref.py: SP2 projector, projected Lanczos recurrence with full
reorthogonalisation, Rayleigh quotient) against ``np.linalg.eigh`` (yardstick 1) and, for the generalized problem and the gradients ``c c^T`` / ``-eps c c^T``,
against ``torch.linalg`` autograd (yardstick 2: cholesky -> ``eigvalsh``); ``FrontierLoss`` against ``OrbitalEnergyLoss("mae", "frontier")``; the public surface
and the host-side refusals of ``nq_orb_front_*``.

Units: ``U_eps = m 2^-52 kappa_2(S) (eps_max - eps_min)`` for a level, ``U_g = U_eps / sep max|g c c^T|`` for a gradient (``sep``: the distance from the level
to its nearest neighbour); bound 10 units each, the project's standing margin.  Measured here: levels <= 0.49 U_eps on the standard problem and <= 0.0083 on the
generalized one, ``v v^T`` <= 0.5 U_g, gradients <= 0.036 U_g, at most twice the subspace dimension in steps."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_frontier_ref as FR
import orbital_purify_ref as PR

BOUND = 10.0
SIZES = (2, 3, 4, 5, 8, 16, 17, 31, 37, 64, 65, 100, 130)
SEEDS = 6


def occupations(m):
    return sorted({n for n in (1, 2, m // 5, m // 2, m - 2, m - 1) if 1 <= n <= m - 1})


@pytest.mark.parametrize("m", SIZES)
def test_restatement_against_eigh_over_the_small_shapes(m):
    worst = np.zeros(3)
    for n in occupations(m):
        for seed in range(SEEDS):
            rng = np.random.default_rng(1000 * m + 10 * n + seed)
            H, _ = FR.random_hamiltonian(rng, m, n, gap=0.3 if seed % 2 == 0 else 0.01)
            ev, U = np.linalg.eigh(H)
            u = FR.level_unit(m, ev[-1] - ev[0])
            sol = PR.purify(H, n)
            assert sol["status"] == 0
            for which, k in ((FR.HOMO, n - 1), (FR.LUMO, n)):
                s = FR.side(H, sol["X"], sol["e_min"], sol["e_max"], n, which)
                dim = n if which == FR.HOMO else m - n
                assert s["conv"] == 1 and s["iters"] <= min(m, 2 * dim), (m, n, seed, which, s["iters"])
                fig = [abs(s["eps"] - ev[k]) / u, np.abs(np.outer(s["vec"], s["vec"]) - np.outer(U[:, k], U[:, k])).max() / (u / FR.separation(ev, k)), s["iters"] / dim]
                worst = np.maximum(worst, fig)
                assert fig[0] <= BOUND and fig[1] <= BOUND, (m, n, seed, which, fig)
                assert abs(s["vec"] @ s["vec"] - 1.0) <= 8 * 2.0 ** -52
    print(f"orbital_frontier_parity restatement m={m}: level {worst[0]:.3g} U_eps, v v^T {worst[1]:.3g} U_g, steps / dimension {worst[2]:.3g}")


def autograd_frontier(H, S, n, g):
    Ht, St = torch.tensor(H, requires_grad=True), torch.tensor(S, requires_grad=True)
    L = torch.linalg.cholesky(St)
    Y = torch.linalg.solve_triangular(L, Ht, upper=False)
    A = torch.linalg.solve_triangular(L, Y.T, upper=False)
    e = torch.linalg.eigvalsh(0.5 * (A + A.T))
    (g[0] * e[n - 1] + g[1] * e[n]).backward()
    sym = lambda a: 0.5 * (a + a.T)
    return e.detach().numpy(), sym(Ht.grad.numpy()), sym(St.grad.numpy())


GENERAL = [c for c in DR.CASES if 1 <= c[1] < c[0]]


@pytest.mark.parametrize("case", GENERAL, ids=[f"m{c[0]}-n{c[1]}-k{c[3]:g}" for c in GENERAL])
def test_generalized_problem_and_gradients_against_torch_autograd(case):
    m, n = case[0], case[1]
    H, S = DR.gapped_case(*case)
    g = (-0.7, 1.3)
    ev, aH, aS = autograd_frontier(H, S, n, g)
    homo, lumo, sol = FR.frontier(H, S, n)
    assert sol["status"] == 0 and homo["conv"] == 1 and lumo["conv"] == 1
    kap = float(np.linalg.cond(S))
    u = FR.level_unit(m, ev[-1] - ev[0], kap)
    fig = [abs(homo["eps"] - ev[n - 1]) / u, abs(lumo["eps"] - ev[n]) / u]
    gH, gS = FR.gradients((homo, lumo), g)
    uH = sum(u / FR.separation(ev, k) * np.abs(gg * np.outer(s["coef"], s["coef"])).max() for s, k, gg in ((homo, n - 1, g[0]), (lumo, n, g[1])))
    uS = sum(u / FR.separation(ev, k) * np.abs(gg * s["eps"] * np.outer(s["coef"], s["coef"])).max() for s, k, gg in ((homo, n - 1, g[0]), (lumo, n, g[1])))
    fig += [np.abs(gH - aH).max() / uH, np.abs(gS - aS).max() / uS]
    print(f"orbital_frontier_parity restatement generalized m={m} n_occ={n} kappa={kap:.3g}: levels {fig[0]:.3g} {fig[1]:.3g} U_eps, gH {fig[2]:.3g} gS {fig[3]:.3g} U_g, "
          f"steps {homo['iters']} / {lumo['iters']}")
    assert max(fig) <= BOUND, (case, fig)
    for s in (homo, lumo):
        assert abs(s["coef"] @ S @ s["coef"] - 1.0) <= BOUND * m * 2.0 ** -52 * kap


def test_equal_top_occupied_levels_give_the_level():
    rng = np.random.default_rng(7)
    m, n = 37, 9
    lev = np.concatenate([np.sort(rng.uniform(-20.0, -0.2, n)), np.sort(rng.uniform(0.2, 2.0, m - n))])
    lev[n - 2] = lev[n - 1]
    Q = np.linalg.qr(rng.standard_normal((m, m)))[0]
    H = PR.lower_sym((Q * lev) @ Q.T)
    homo, lumo, sol = FR.frontier(H, None, n)
    u = FR.level_unit(m, lev[-1] - lev[0])
    assert homo["conv"] == 1 and abs(homo["eps"] - lev[n - 1]) <= BOUND * u and abs(lumo["eps"] - lev[n]) <= BOUND * u


def test_absent_levels_dimension_one_and_exhaustion():
    rng = np.random.default_rng(9)
    H, _ = FR.random_hamiltonian(rng, 5, 2)
    ev = np.linalg.eigvalsh(H)
    for n, absent in ((0, FR.HOMO), (5, FR.LUMO)):
        sol = PR.purify(H, n)
        s = FR.side(H, sol["X"], sol["e_min"], sol["e_max"], n, absent)
        assert s["conv"] == -1 and np.isnan(s["eps"]) and np.isnan(s["vec"]).all() and s["iters"] == 0
        t = FR.side(H, sol["X"], sol["e_min"], sol["e_max"], n, 1 - absent)       # the whole space: m steps
        assert t["conv"] == 1 and t["iters"] <= 5 and abs(t["eps"] - (ev[0] if n == 0 else ev[-1])) <= BOUND * FR.level_unit(5, ev[-1] - ev[0])
    one = FR.side(np.array([[-3.5]]), np.array([[1.0]]), -3.5, -3.5, 1, FR.HOMO)   # m = 1: beta vanishes at the first step
    assert one["conv"] == 1 and one["iters"] == 1 and one["eps"] == -3.5 and one["vec"][0] == 1.0
    sol = PR.purify(H, 1)
    s = FR.side(H, sol["X"], sol["e_min"], sol["e_max"], 1, FR.HOMO)               # subspace dimension 1
    assert s["conv"] == 1 and s["iters"] <= 2
    big, _ = FR.random_hamiltonian(rng, 130, 26)
    sol = PR.purify(big, 26)
    s = FR.side(big, sol["X"], sol["e_min"], sol["e_max"], 26, FR.LUMO, k_max=8)
    assert s["conv"] == 0 and s["iters"] == 8 and np.isnan(s["eps"]) and np.isnan(s["coef"]).all()


def test_start_vector():
    r = FR.start_vector(1024)
    assert np.all(r >= 0.5) and np.all(r < 1.5) and len(np.unique(r)) == 1024 and r[0] == 0.5 + 12345 / 2.0 ** 32
    assert r[1] == 0.5 + ((2654435761 + 12345) % 2 ** 32) / 2.0 ** 32


def test_frontier_loss_against_the_orbital_energy_loss(monkeypatch):
    """The losses are plain torch; their refusal of CPU tensors is switched off for this comparison."""
    from nabladft_amd import orbital_loss as OL
    monkeypatch.setattr(OL, "_require_gpu", lambda t: None)
    rng = np.random.default_rng(11)
    op = np.array([0, 4, 9, 12, 13])
    n_occ = np.array([2, 5, 1, 1])                                     # the second and the last molecule have no LUMO
    ep, et = torch.from_numpy(rng.standard_normal(13)), torch.from_numpy(rng.standard_normal(13))
    nan = float("nan")
    pick = lambda e: torch.stack((torch.stack([e[int(op[b] + n_occ[b] - 1)] for b in range(4)]),
                                  torch.stack([e[int(op[b] + n_occ[b])] if n_occ[b] < op[b + 1] - op[b] else torch.tensor(nan, dtype=torch.float64) for b in range(4)])))
    for kind in ("mae", "mse"):
        pred = pick(ep).clone().requires_grad_(True)
        a = OL.FrontierLoss(kind, "both")(pred, pick(et), n_occ, op)
        b = OL.OrbitalEnergyLoss(kind, "frontier")(ep, et, n_occ, op)
        assert abs(float(a.detach()) - float(b)) <= 4 * 2.0 ** -52 * abs(float(b)), kind
        a.backward()
        assert bool(torch.isfinite(pred.grad).all()) and float(pred.grad[1, 1]) == 0.0 and float(pred.grad[1, 3]) == 0.0
    p, t = pick(ep), pick(et)
    d = (p - t).numpy()
    has = np.array([True, False, True, False])
    assert abs(float(OL.FrontierLoss("mae", "gap")(p, t, n_occ, op)) - np.abs(d[1] - d[0])[has].sum() / 4) <= 1e-15
    assert abs(float(OL.FrontierLoss("mse", "homo")(p, t, n_occ, op)) - (d[0] ** 2).mean()) <= 1e-15
    assert abs(float(OL.FrontierLoss("mae", "lumo")(p, t, n_occ, op)) - np.abs(d[1])[has].sum() / 4) <= 1e-15
    with pytest.raises(ValueError, match="which"):
        OL.FrontierLoss("mae", "all")
    with pytest.raises(ValueError, match="kind"):
        OL.FrontierLoss("huber")
    with pytest.raises(ValueError, match="shapes"):
        OL.FrontierLoss()(p[0], t[0], n_occ, op)
    assert OL.FrontierLoss.packed is True


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib, orbital_loss as OL, orbitals as O
    for name in ("purified_frontier", "FrontierLoss", "QHNetPurifiedFrontierLightning"):
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    assert nq.FrontierLevels is O.FrontierLevels and "FrontierLevels" in O.__all__ and "FrontierLevels" in nq.__all__
    assert O.FrontierLevels._fields == ("homo", "lumo", "gap", "coeff", "vectors", "iterations", "residual", "converged")
    sig = inspect.signature(OL.purified_frontier).parameters
    assert list(sig) == ["H_packed", "S_packed", "plan_or_orb_ptr", "n_occ", "orthogonalizer", "max_iter", "k_max", "tol", "solution", "return_solution"]
    assert sig["max_iter"].default == 100 and sig["k_max"].default == 256 and sig["tol"].default == 2.0 ** -44 and sig["solution"].default is None
    sig = inspect.signature(O.BatchedPurification.frontier).parameters
    assert list(sig) == ["self", "k_max", "tol", "transform"] and sig["k_max"].default == 256 and sig["tol"].default == 2.0 ** -44 and sig["transform"].default is None
    sig = inspect.signature(O.BatchedPurification.frontier_gradients).parameters
    assert list(sig) == ["self", "levels", "g_homo", "g_lumo", "overlap"] and sig["overlap"].default is True
    assert list(inspect.signature(O.BatchedPurification.frontier_check).parameters) == ["self", "levels"]
    sig = inspect.signature(OL.FrontierLoss.__init__).parameters
    assert list(sig) == ["self", "kind", "which", "charge"] and sig["kind"].default == "mae" and sig["which"].default == "gap" and sig["charge"].default == 0
    assert issubclass(OL.QHNetPurifiedFrontierLightning, OL.QHNetPurifiedDensityLightning) and "frontier" in OL.QHNetPurifiedFrontierLightning.KEYS
    assert inspect.signature(OL.QHNetPurifiedFrontierLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    assert OL.QHNetPurifiedDensityLightning.KEYS == OL.QHNetDensityLightning.KEYS              # the parent is unchanged
    lib = _lib.load()
    for sym in ("nq_orb_front_lanczos", "nq_orb_front_gram"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert lib.nq_abi_version() == 17 and _lib.ABI_VERSION == 17
    assert "other than HOMO and LUMO" in " ".join(O.__doc__.split())


def test_cpu_tensors_are_refused():
    import nabladft_amd as nq
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.purified_frontier(torch.zeros(4, requires_grad=True), None, [0, 2], [1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.FrontierLoss()(torch.zeros(2, 1), torch.zeros(2, 1), [1], [0, 2])


def test_host_side_argument_checks():
    """Both entry points check their arguments on the host before any device work: no GPU is needed to be refused."""
    from nabladft_amd import _lib
    lib = _lib.load()
    B, M, P = 2, 5, 13
    buf = (C.c_double * 256)()
    a = [C.c_void_p(C.addressof(buf) + 64 * k) for k in range(16)]
    err = lambda: lib.nq_last_error().decode()
    lz = lambda **kw: lib.nq_orb_front_lanczos(*[kw.get(k, v) for k, v in (("state", a[0]), ("B", B), ("M", M), ("P", P), ("Ht", a[1]), ("X", a[2]), ("shift", a[3]),
                                                                         ("n_occ", a[4]), ("W", a[5]), ("k_max", 256), ("tol", 2.0 ** -44), ("V", a[6]), ("vptr", a[7]),
                                                                         ("eps", a[8]), ("vec", a[9]), ("coef", a[10]), ("iters", a[11]), ("res", a[12]),
                                                                         ("conv", a[13]), ("stream", None))])
    for name in ("state", "Ht", "X", "shift", "V", "vptr", "eps", "vec", "coef", "iters", "res", "conv"):
        assert lz(**{name: None}) == _lib.NQ_ERR_ARG and "null" in err(), name
    assert lz(n_occ=None) == _lib.NQ_ERR_ARG and "n_occ" in err()
    for k in (0, -1, 1025):
        assert lz(k_max=k) == _lib.NQ_ERR_ARG and "k_max" in err()
    for t in (0.0, -1e-3, 1.0, float("nan")):
        assert lz(tol=t) == _lib.NQ_ERR_ARG and "tol" in err()
    assert lz(vec=a[10]) == _lib.NQ_ERR_ARG and "different arrays" in err()
    assert lz(V=a[1]) == _lib.NQ_ERR_ARG and "different arrays" in err()
    assert lz(B=0) == _lib.NQ_ERR_ARG and "empty batch" in err()
    assert lz(P=3) == _lib.NQ_ERR_ARG and "does not fit" in err()
    assert lz(B=2 ** 30, M=2 ** 30, P=2 ** 30) == _lib.NQ_ERR_ARG and "exceed the grid" in err()
    gr = lambda **kw: lib.nq_orb_front_gram(*[kw.get(k, v) for k, v in (("state", a[0]), ("B", B), ("M", M), ("P", P), ("g", a[1]), ("eps", a[2]), ("coef", a[3]),
                                                                      ("conv", a[4]), ("gH", a[5]), ("gS", a[6]), ("stream", None))])
    for name in ("state", "g", "coef", "conv", "gH"):
        assert gr(**{name: None}) == _lib.NQ_ERR_ARG and "null" in err(), name
    assert gr(eps=None) == _lib.NQ_ERR_ARG and "second output" in err()
    assert gr(gS=a[5]) == _lib.NQ_ERR_ARG and "different arrays" in err()
    assert gr(gH=a[3]) == _lib.NQ_ERR_ARG and "different arrays" in err()
    assert gr(M=1) == _lib.NQ_ERR_ARG
    assert not any(buf)
