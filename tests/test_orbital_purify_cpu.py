"""CPU: the numpy restatement of the purification route (tests/orbital_purify_ref.py) against the float64 yardsticks of the solver route
(tests/orbital_density_ref.py: ``closed_form`` and ``autograd``), its failure and trivial cases, and the public surface and host-side refusals of
``BatchedPurification`` / ``purified_density_matrix`` / ``QHNetPurifiedDensityLightning`` / ``nq_orb_pur_*``.

Bounds: D within 10 U_D (``orbital_purify_ref.density_unit``), gradients within 10 ``orbital_density_ref.units``: the project's standing margin for these
units.  Measured here: D <= 0.26 (worst at m = 2; <= 0.031 for m >= 17), gH <= 0.71 (m = 3), gS <= 0.095; 0..40 iterations."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_purify_ref as PR

BOUND = 10.0


@pytest.mark.parametrize("standard", [False, True])
def test_restatement_against_closed_form_and_autograd(standard):
    for case in DR.CASES:
        m, n = case[0], case[1]
        H, S = DR.gapped_case(*case, standard=standard)
        G, T = DR.upstream(m, case[4])
        loss = DR.quadratic_loss(G, T, with_eps=False)
        eps, D, gH, gS = DR.closed_form(H, S, n, loss)
        _, Da, aH, aS = DR.autograd(H, S, n, loss)
        Dp, pH, pS, sol = PR.density_and_gradients(H, S, n, G + (D - T))          # dL/dD at the reference density
        assert sol["status"] == 0 and sol["iters"] <= 60 and (sol["kind"] == 0) == (n < m and m > 1)
        uD = PR.density_unit(H, S, n, eps, D)
        uH, uS = DR.units(H, S, n, eps, gH, gS)
        assert np.array_equal(Dp, Dp.T) and np.array_equal(pH, pH.T)
        assert np.abs(Dp - D).max() <= BOUND * uD and np.abs(Dp - Da).max() <= BOUND * uD, (case, standard)
        if n == m:
            assert np.all(pH == 0.0)                                 # X = I whatever H is: exactly zero, where the references leave their rounding
        else:
            assert np.abs(pH - gH).max() <= BOUND * uH and np.abs(pH - aH).max() <= BOUND * uH, (case, standard)
        if S is not None:
            assert np.abs(pS - gS).max() <= BOUND * uS and np.abs(pS - aS).max() <= BOUND * uS, (case, standard)
            assert abs((Dp * S).sum() - 2.0 * n) <= BOUND * m * 2.0 ** -52 * np.linalg.cond(S) * 2.0 * n
        else:
            assert pS is None and abs(np.trace(Dp) - 2.0 * n) <= 64 * 2.0 ** -52 * n
        if sol["kind"] == 0:
            t, t2 = sol["traces"][-1]
            assert abs(t - n) <= 16 * 2.0 ** -52 * n and sol["log"][-1] == PR.STOPPED and all(e in (1, 2) for e in sol["log"][:-1])


def test_a_gapless_spectrum_does_not_converge():
    rng = np.random.Generator(np.random.PCG64(5))
    m, n = 33, 11
    lev = np.sort(rng.uniform(-5.0, 5.0, size=m))
    lev[n] = lev[n - 1]                                              # two equal levels across the Fermi level
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    A = (Q * lev[None, :]) @ Q.T
    D, gH, gS, sol = PR.density_and_gradients(0.5 * (A + A.T), None, n, rng.normal(size=(m, m)))
    assert sol["status"] == 4 and sol["iters"] == 100 and np.isnan(D).all() and gH is None
    # with the gap open by 1e-3 the same spectrum converges
    lev[n:] += 1e-3
    A = (Q * lev[None, :]) @ Q.T
    sol = PR.density_and_gradients(0.5 * (A + A.T), None, n)[3]
    assert sol["status"] == 0 and sol["iters"] < 100


def test_trivial_cases():
    H, S = DR.gapped_case(17, 5, 0.3, 1e2, 3)
    G = np.random.Generator(np.random.PCG64(1)).normal(size=(17, 17))
    D, gH, gS, sol = PR.density_and_gradients(H, S, 0, G)
    assert sol["kind"] == 1 and sol["iters"] == 0 and np.all(D == 0.0) and np.all(gH == 0.0) and np.all(gS == 0.0)
    D, gH, gS, sol = PR.density_and_gradients(H, S, 17, G)
    assert sol["kind"] == 2 and sol["iters"] == 0 and np.all(gH == 0.0)
    assert np.abs(D - 2.0 * np.linalg.inv(S)).max() <= 17 * 2.0 ** -52 * np.linalg.cond(S) * np.abs(D).max()        # D = 2 S^-1
    Si = np.linalg.inv(S)
    assert np.abs(gS + 2.0 * Si @ (0.5 * (G + G.T)) @ Si).max() <= 1e-9 * np.abs(gS).max()                         # and its derivative
    D, gH, gS, sol = PR.density_and_gradients(3.0 * np.eye(4), None, 2, np.ones((4, 4)))                             # e_max = e_min: X = I
    assert sol["kind"] == 2 and np.array_equal(D, 2.0 * np.eye(4)) and np.all(gH == 0.0)


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib, orbital_loss as OL, orbitals as O
    assert nq.BatchedPurification is O.BatchedPurification and nq.purified_density_matrix is OL.purified_density_matrix
    assert nq.QHNetPurifiedDensityLightning is OL.QHNetPurifiedDensityLightning
    for name in ("BatchedPurification", "purified_density_matrix", "QHNetPurifiedDensityLightning"):
        assert name in nq.__all__
    assert "BatchedPurification" in O.__all__ and "Orthogonalizer" in O.__all__ and "purified_density_matrix" in OL.__all__
    sig = inspect.signature(OL.purified_density_matrix).parameters
    assert list(sig) == ["H_packed", "S_packed", "plan_or_orb_ptr", "n_occ", "orthogonalizer", "max_iter", "return_solution"]
    assert sig["orthogonalizer"].default is None and sig["max_iter"].default == 100 and sig["return_solution"].default is False
    sig = inspect.signature(O.BatchedPurification.purify).parameters
    assert list(sig)[:4] == ["self", "H_packed", "n_occ", "max_iter"] and sig["max_iter"].default == 100
    sig = inspect.signature(O.BatchedPurification.response).parameters
    assert list(sig) == ["self", "G", "overlap"] and sig["overlap"].default is True
    assert list(inspect.signature(O.BatchedPurification.orthogonalize).parameters) == ["self", "S_packed"]
    for name in ("density", "check", "congruence", "gemm", "prepare", "step", "response_start", "response_step", "populations", "populations_backward"):
        assert callable(getattr(O.BatchedPurification, name)), name
    assert isinstance(O.BatchedPurification.iterations, property)
    assert issubclass(OL.QHNetPurifiedDensityLightning, OL.QHNetDensityLightning) and OL.QHNetPurifiedDensityLightning.max_iter == 100
    assert inspect.signature(OL.QHNetPurifiedDensityLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    lib = _lib.load()
    for sym in ("nq_orb_pur_orthogonalizer", "nq_orb_pur_congruence", "nq_orb_pur_gemm", "nq_orb_pur_init", "nq_orb_pur_step", "nq_orb_pur_run",
                "nq_orb_pur_response_init", "nq_orb_pur_response_step", "nq_orb_pur_response_run"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert lib.nq_abi_version() == 17
    assert "status 4" in " ".join(OL.purified_density_matrix.__doc__.split()) and "open gap" in OL.__doc__ and "open gap" in O.__doc__
    assert "did not converge" in O._failure_text(3, 4, 100, 17) and "molecule 3" in O._failure_text(3, 4, 100, 17)


def test_cpu_tensors_and_bad_arguments_are_refused():
    import nabladft_amd as nq
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.purified_density_matrix(torch.zeros(4, requires_grad=True), None, [0, 2], [1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.purified_density_matrix(torch.zeros(4), torch.zeros(4), [0, 2], [1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.BatchedPurification([0, 2], "cpu")


def test_host_side_argument_checks():
    """Every entry point checks its arguments on the host before any device work: no GPU is needed to be refused."""
    from nabladft_amd import _lib
    lib = _lib.load()
    B, M, P = 2, 5, 13
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(C.addressof(buf) + 64)
    err = lambda: lib.nq_last_error().decode()
    assert lib.nq_orb_pur_orthogonalizer(None, B, M, P, p, 1, q, None) == _lib.NQ_ERR_ARG and "null" in err()
    assert lib.nq_orb_pur_orthogonalizer(p, B, M, P, None, 1, q, None) == _lib.NQ_ERR_ARG
    assert lib.nq_orb_pur_orthogonalizer(p, B, M, P, q, 1, q, None) == _lib.NQ_ERR_ARG and "must not be S" in err()
    assert lib.nq_orb_pur_orthogonalizer(p, 0, M, P, q, 1, p, None) == _lib.NQ_ERR_ARG and "empty batch" in err()
    assert lib.nq_orb_pur_congruence(p, B, M, P, q, 0, p, 1, 0, 1.0, None, q, None) == _lib.NQ_ERR_ARG and "tmp" in err()
    assert lib.nq_orb_pur_congruence(p, B, M, P, None, 0, q, 1, 0, 1.0, None, q, None) == _lib.NQ_ERR_ARG and "different arrays" in err()
    assert lib.nq_orb_pur_gemm(p, B, M, P, q, q, None, 1.0, 0.0, q, None) == _lib.NQ_ERR_ARG and "operand" in err()
    assert lib.nq_orb_pur_init(p, B, M, P, None, 1, None, None, 100, q, q, None) == _lib.NQ_ERR_ARG and "n_occ" in err()
    assert lib.nq_orb_pur_init(p, B, M, P, None, 1, None, q, 0, q, q, None) == _lib.NQ_ERR_ARG and "max_iter" in err()
    assert lib.nq_orb_pur_init(p, B, M, P, None, 1, None, q, 10001, q, q, None) == _lib.NQ_ERR_ARG
    assert lib.nq_orb_pur_step(p, B, M, P, 5, 5, q, q, None) == _lib.NQ_ERR_ARG and "iteration" in err()
    assert lib.nq_orb_pur_step(p, B, M, P, -1, 5, q, q, None) == _lib.NQ_ERR_ARG
    assert lib.nq_orb_pur_step(p, B, M, P, 0, 5, None, q, None) == _lib.NQ_ERR_ARG
    assert lib.nq_orb_pur_run(p, B, M, P, 5, q, None, None) == _lib.NQ_ERR_ARG
    assert lib.nq_orb_pur_run(p, B, M, 3, 5, q, q, None) == _lib.NQ_ERR_ARG and "does not fit" in err()
    assert lib.nq_orb_pur_response_init(p, B, M, P, q, 5, p, q, None) == _lib.NQ_ERR_ARG and "must not be Gt" in err()
    assert lib.nq_orb_pur_response_step(p, B, M, P, 0, 5, q, None, q, None) == _lib.NQ_ERR_ARG and "second output" in err()
    assert lib.nq_orb_pur_response_run(p, B, M, P, 5, q, None, q, None) == _lib.NQ_ERR_ARG and "second output" in err()
    assert lib.nq_orb_pur_response_run(p, B, M, P, 5, q, q, q, None) == _lib.NQ_ERR_ARG and "must not be X1" in err()
