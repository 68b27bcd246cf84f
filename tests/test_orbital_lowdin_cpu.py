"""CPU: the numpy restatement of the Löwdin analysis (tests/orbital_lowdin_ref.py) against known answers, ``scipy.linalg.sqrtm`` and torch autograd, the
degenerate cases the closed form exists for, the sum rules, and the public surface of the feature.  No GPU.

Bounds.  With E = 2^-52, m orbitals and kappa = s_max / s_min: ``eigh`` returns U and s with |U diag(s) U^T - S| <= c m E |S| and U^T U = I to c m E, so
A A = S holds to c m E s_max, A A^- = I to c m E sqrt(kappa), and the Sylvester residual A Z + Z A - g to c m E kappa^(1/2) |g| (Z carries 1 / (a_i + a_j) <=
1 / (2 a_min), A carries a_max).  c = 16 leaves room for the products that form the residuals themselves."""
import inspect

import numpy as np
import pytest
import scipy.linalg
import torch

import orbital_bond_ref as BR
import orbital_density_ref as DR
import orbital_lowdin_ref as LR

E = 2.0 ** -52
C = 16.0


def spd(m, kappa0, seed):
    return DR.overlap(m, kappa0, np.random.Generator(np.random.PCG64(seed)))


def test_identity_overlap():
    m = 7
    A, Ai, s, Uv = LR.functions(np.eye(m))
    assert np.array_equal(A, np.eye(m)) and np.array_equal(Ai, np.eye(m)) and np.array_equal(s, np.ones(m))
    a, ia, cond, info = LR.weights(s)
    assert np.array_equal(a, np.ones(m)) and np.array_equal(ia, np.ones(m)) and cond == 1.0 and info == 0
    rng = np.random.Generator(np.random.PCG64(1))
    D = LR.sym(rng.normal(size=(m, m)))
    DL, Y = LR.congruence(A, D)
    assert np.array_equal(DL, D) and np.array_equal(Y, D)
    assert LR.weights(np.array([1.0, -0.5]))[3] == 1 and LR.weights(np.array([1.0, np.inf]))[3] == 1 and np.isnan(LR.weights(np.array([0.0, 1.0]))[0]).all()


def test_two_by_two_by_hand():
    """S = [[1, t], [t, 1]]: levels 1 -+ t with vectors (1, -+1) / sqrt 2, so A = 1/2 [[p + q, p - q], [p - q, p + q]], p = sqrt(1 + t), q = sqrt(1 - t)."""
    t = 0.36
    S = np.array([[1.0, t], [t, 1.0]])
    p, q = np.sqrt(1.0 + t), np.sqrt(1.0 - t)
    A, Ai, s, Uv = LR.functions(S)
    assert np.allclose(s, [1.0 - t, 1.0 + t], rtol=0, atol=4 * E)
    assert np.allclose(A, 0.5 * np.array([[p + q, p - q], [p - q, p + q]]), rtol=0, atol=8 * E)
    assert np.allclose(Ai, 0.5 * np.array([[1 / p + 1 / q, 1 / p - 1 / q], [1 / p - 1 / q, 1 / p + 1 / q]]), rtol=0, atol=8 * E)
    # dL/dS for L = A_01: d(p - q)/2 / dt = 1/4 (1/p + 1/q), spread over S_01 and S_10
    g = np.array([[0.0, 1.0], [0.0, 0.0]])
    gS = LR.matfun_response(g, s, Uv, 0)
    assert abs(2.0 * gS[0, 1] - 0.25 * (1 / p + 1 / q)) <= 16 * E and np.array_equal(gS, gS.T)
    # the closed-shell density of one orbital (1, 1) / sqrt(2 (1 + t)): Löwdin populations 1 and 1, W_01 = 1
    c = np.array([1.0, 1.0]) / np.sqrt(2.0 * (1.0 + t))
    DL, qpop, W, V = LR.lowdin(2.0 * np.outer(c, c), S, np.array([0, 1, 2]))
    assert np.allclose(qpop, [1.0, 1.0], rtol=0, atol=16 * E) and np.allclose(W, np.ones((2, 2)), rtol=0, atol=32 * E) and np.allclose(V, [1.0, 1.0], rtol=0, atol=32 * E)


@pytest.mark.parametrize("m,kappa0", [(1, 1.0), (3, 1e2), (17, 1e2), (65, 1e4)])
def test_identities_within_condition_scaled_bounds(m, kappa0):
    S = spd(m, kappa0, 10 + m) if m > 1 else np.array([[2.5]])
    A, Ai, s, Uv = LR.functions(S)
    kap, smax = s.max() / s.min(), s.max()
    assert np.array_equal(A, A.T) and np.array_equal(Ai, Ai.T)
    assert np.abs(A @ A - S).max() <= C * m * E * smax
    assert np.abs(A @ Ai - np.eye(m)).max() <= C * m * E * np.sqrt(kap)
    rng = np.random.Generator(np.random.PCG64(20 + m))
    g = rng.normal(size=(m, m))
    Z = LR.matfun_response(g, s, Uv, 0)
    assert np.abs(A @ Z + Z @ A - LR.sym(g)).max() <= C * m * E * np.sqrt(kap) * np.abs(g).max() * np.sqrt(m)
    # the A^- form: from A^- A = I, dA^- = -A^- dA A^-, so its response is the A response of -A^- g A^-
    Zi = LR.matfun_response(g, s, Uv, 1)
    Zr = LR.matfun_response(-Ai @ LR.sym(g) @ Ai, s, Uv, 0)
    assert np.abs(Zi - Zr).max() <= C * m * E * kap * max(np.abs(Zi).max(), np.finfo(float).tiny)


@pytest.mark.parametrize("m,kappa0", [(3, 1e2), (17, 1e2), (65, 1e4)])
def test_against_scipy_sqrtm(m, kappa0):
    S = spd(m, kappa0, 30 + m)
    A, Ai, s, Uv = LR.functions(S)
    R = np.real(scipy.linalg.sqrtm(S))
    kap = s.max() / s.min()
    assert np.abs(A - R).max() <= C * m * E * np.sqrt(kap) * np.sqrt(s.max())
    assert np.abs(Ai - np.linalg.inv(R)).max() <= C * m * E * kap / np.sqrt(s.min())


@pytest.mark.parametrize("m", [2, 9, 17])
def test_closed_forms_against_torch_autograd_on_gapped_levels(m):
    rng = np.random.Generator(np.random.PCG64(40 + m))
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    s0 = np.linspace(0.2, 1.7, m)                                # well separated levels
    S = LR.sym((Q * s0[None, :]) @ Q.T)
    M, G0 = LR.sym(rng.normal(size=(m, m))), LR.sym(rng.normal(size=(m, m)))
    A, Ai, s, Uv = LR.functions(S)
    assert LR.min_relative_gap(s) > m * 2.0 ** -40
    for kind, X in ((0, A), (1, Ai)):
        St, Mt = torch.tensor(S, requires_grad=True), torch.tensor(M, requires_grad=True)
        Xt = LR.torch_functions(St)[kind]
        ML = Xt @ Mt @ Xt
        (torch.from_numpy(G0) * ML).sum().backward()
        MLn, Y = LR.congruence(X, M)
        scale = np.abs(X).max() ** 2 * np.abs(M).max() * m * m
        assert np.abs(MLn - ML.detach().numpy()).max() <= C * m * E * (s.max() / s.min()) * scale
        gM, gX = LR.congruence_backward(G0, X, Y)
        gS = LR.matfun_response(gX, s, Uv, kind)
        ref_M, ref_S = LR.sym(Mt.grad.numpy()), LR.sym(St.grad.numpy())
        gap = 1.0 / LR.min_relative_gap(s)                       # what the backward of eigh divides by
        assert np.abs(gM - ref_M).max() <= C * m * E * (s.max() / s.min()) * scale
        assert np.abs(gS - ref_S).max() <= C * m * E * gap * (s.max() / s.min()) ** 2 * max(np.abs(ref_S).max(), 1.0), (kind, float(np.abs(gS - ref_S).max()))


def degenerate_overlaps():
    m = 6
    rng = np.random.Generator(np.random.PCG64(50))
    blk = spd(3, 10.0, 51)
    two = np.zeros((m, m))
    two[:3, :3] = blk
    two[3:, 3:] = blk                                            # two identical atoms far apart: every level twice
    return [("identity", np.eye(m)), ("two identical atoms", two)], rng


def test_degenerate_levels_are_finite_where_eigh_backward_is_not():
    cases, rng = degenerate_overlaps()
    for name, S in cases:
        m = S.shape[0]
        g = rng.normal(size=(m, m))
        s, Uv = LR.decompose(S)
        for kind in (0, 1):
            gS = LR.matfun_response(g, s, Uv, kind)
            assert np.isfinite(gS).all(), (name, kind)
            if name == "identity":                               # K = 1/2 (kind 0), -1/2 (kind 1) everywhere
                assert np.abs(gS - (0.5 if kind == 0 else -0.5) * LR.sym(g)).max() <= C * m * E * np.abs(g).max()
            else:                                                # block-diagonal S: the diagonal blocks of the gradient are those of one atom alone
                sb, Ub = LR.decompose(S[:3, :3])
                ref = LR.matfun_response(g[:3, :3], sb, Ub, kind)
                assert np.abs(gS[:3, :3] - ref).max() <= C * m * E * (s.max() / s.min()) ** 2 * max(np.abs(ref).max(), 1.0)
            St = torch.tensor(S, requires_grad=True)
            (torch.from_numpy(g) * LR.torch_functions(St)[kind]).sum().backward()
            assert not np.isfinite(St.grad.numpy()).all(), (name, kind)      # the route that divides by differences of levels


@pytest.mark.parametrize("case", [c for c in DR.CASES if c[0] > 1][:6])
def test_sum_rules_on_idempotent_densities(case):
    m, n_occ = case[0], case[1]
    H, S = DR.gapped_case(*case)
    L = np.linalg.cholesky(S)
    w, Y = np.linalg.eigh(np.linalg.solve(L, np.linalg.solve(L, H).T).T)
    Cc = np.linalg.solve(L.T, Y)
    D = 2.0 * Cc[:, :n_occ] @ Cc[:, :n_occ].T
    sizes = [1] * m if m <= 3 else [5, 12] if m == 17 else [32, 14, 5, 14] + [1] * (m - 65) if m == 65 else [32, 14, 5, 32, 1, 14, 32]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    assert ptr[-1] == m
    DL, q, W, V = LR.lowdin(D, S, ptr)
    kap = np.linalg.cond(S)
    tol = C * m * E * kap * 2.0 * n_occ
    assert abs(q.sum() - np.trace(D @ S)) <= tol and abs(q.sum() - 2.0 * n_occ) <= tol
    assert np.abs(W.sum(1) - 2.0 * q).max() <= tol and np.array_equal(W, W.T)
    assert np.abs((DL * DL).sum(1) - 2.0 * np.diag(DL)).max() <= tol
    # the Löwdin Hamiltonian has the generalised levels
    Ai = LR.functions(S)[1]
    HL = LR.congruence(Ai, H)[0]
    assert np.abs(np.linalg.eigvalsh(HL) - w).max() <= C * m * E * kap * np.abs(w).max()


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd import orbital_loss as OL
    from nabladft_amd import orbitals as O
    names = ("lowdin_basis", "lowdin_density", "lowdin_hamiltonian", "lowdin_populations", "lowdin_charges", "lowdin_bond_orders", "LowdinChargeLoss",
             "QHNetLowdinLightning", "LowdinBasis")
    for name in names:
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    assert nq.LowdinBasis is O.LowdinBasis and "LowdinBasis" in O.__all__
    assert list(inspect.signature(OL.lowdin_basis).parameters) == ["S_packed", "plan_or_orb_ptr"]
    assert list(inspect.signature(OL.lowdin_density).parameters) == ["D", "basis"] and list(inspect.signature(OL.lowdin_hamiltonian).parameters) == ["H", "basis"]
    assert list(inspect.signature(OL.lowdin_populations).parameters) == ["D", "plan", "basis"]
    assert list(inspect.signature(OL.lowdin_bond_orders).parameters) == ["D", "plan", "basis"] and list(inspect.signature(OL.lowdin_charges).parameters) == ["z", "atom_pop"]
    assert OL.LowdinChargeLoss.packed is True and inspect.signature(OL.LowdinChargeLoss.__init__).parameters["kind"].default == "mae"
    with pytest.raises(ValueError):
        OL.LowdinChargeLoss(kind="rmse")
    assert issubclass(OL.QHNetLowdinLightning, OL.QHNetBondOrderLightning)
    assert inspect.signature(OL.QHNetLowdinLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    assert OL.QHNetLowdinLightning.KEYS == OL.QHNetBondOrderLightning.KEYS + ("lowdin_charges", "lowdin_bond_orders")
    assert OL.QHNetBondOrderLightning.KEYS == ("orbital_energies", "density_matrix", "mulliken_charges", "bond_orders")
    for name in ("overlap_weights", "overlap_functions", "low_product", "low_symprod", "low_symmetrize", "sym_congruence", "sym_congruence_backward", "low_mo", "matfun_response"):
        assert callable(getattr(O.BatchedOrbitals, name)), name
    for name in ("low_product", "low_symprod", "low_symmetrize", "sym_congruence"):
        assert getattr(O.BatchedPurification, name) is getattr(O.BatchedOrbitals, name), name
    assert not hasattr(O.BatchedPurification, "low_mo") and not hasattr(O.BatchedPurification, "overlap_weights")     # they read eps and coeff
    for s in ("nq_orb_low_weights", "nq_orb_low_product", "nq_orb_low_symprod", "nq_orb_low_symmetrize", "nq_orb_low_mo"):
        assert s in _lib.SYMBOLS and hasattr(_lib.load(), s), s
    assert _lib.load().nq_abi_version() == 17 and _lib.ABI_VERSION == 17
    for doc in (OL.lowdin_bond_orders.__doc__, OL.__doc__):
        assert "32" in doc and "closed shells" in doc.lower() and "positive definite" in doc and "1024" in doc
    assert "decomposition" in OL.lowdin_basis.__doc__ and "positive definite" in OL.lowdin_basis.__doc__ and "cached" in OL.lowdin_basis.__doc__
    assert not hasattr(OL, "_transpose_index")                    # the upstream gradient is made symmetric on the device, not through a host-built index
    assert "lowdin_bond_orders" in OL.bond_orders.__doc__ and "no Löwdin analysis" not in OL.bond_orders.__doc__ and "Löwdin" in O.__doc__


def test_python_refusals_without_a_device():
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals, LowdinBasis
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.lowdin_basis(torch.eye(2, dtype=torch.float64).reshape(-1), [0, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        LowdinBasis.of(torch.eye(2, dtype=torch.float64).reshape(-1), [0, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.lowdin_density(torch.zeros(4, dtype=torch.float64), None)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.LowdinChargeLoss()(torch.zeros(3), torch.zeros(3), [0, 1, 3])
    with pytest.raises(ValueError, match="z has"):
        nq.lowdin_charges([1, 6], torch.zeros(3, dtype=torch.float64))
    assert nq.lowdin_charges([1, 6, 8], torch.tensor([0.5, 6.25, 8.0], dtype=torch.float64)).tolist() == [0.5, -0.25, 0.0]
    # checks that come before the state is touched
    fake = BatchedOrbitals.__new__(BatchedOrbitals)
    fake.state = None
    with pytest.raises(ValueError, match="side must be 0"):
        BatchedOrbitals.low_symprod(fake, None, None, 2)
    with pytest.raises(ValueError, match="kind must be 0"):
        BatchedOrbitals.low_mo(fake, None, 3)
    with pytest.raises(ValueError, match="neither gradient"):
        BatchedOrbitals.sym_congruence_backward(fake, None, None, None, False, False)
