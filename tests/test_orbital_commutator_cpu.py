"""CPU: the numpy restatement of the SCF-residual kernels (tests/orbital_commutator_ref.py) against known answers and torch autograd of the dense expression,
the public surface of the feature and its host-side refusals.  No GPU.

Bounds.  With E = 2^-52 and m orbitals a product of two m x m matrices carries m E |X| |Y| per entry; ``eigh`` returns orthonormal vectors to c m E, so a
density built from them commutes with its matrix to c m E |H| |D|; the Löwdin congruences carry the condition number of S as in
tests/test_orbital_lowdin_cpu.py.  c = 16 leaves room for the products that form the residuals themselves."""
import inspect

import numpy as np
import pytest
import torch

import orbital_commutator_ref as CR
import orbital_density_ref as DR
import orbital_lowdin_ref as LR

E = 2.0 ** -52
C = 16.0


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


@pytest.mark.parametrize("m", [1, 2, 9, 33])
def test_a_matrix_commutes_with_itself_and_the_structure_is_exact(m):
    rng = rng_of(100 + m)
    X, Y = LR.sym(rng.normal(size=(m, m))), LR.sym(rng.normal(size=(m, m)))
    assert not CR.product(X, X).any()
    Cm = CR.product(X, Y)
    assert np.array_equal(Cm, -Cm.T) and not np.diag(Cm).any() and not np.signbit(np.diag(Cm)).any()
    assert np.abs(Cm - (X @ Y - Y @ X)).max() <= C * m * E * np.abs(X).max() * np.abs(Y).max() * m
    # garbage above the diagonal of the symmetric operands, on and above the diagonal of the antisymmetric one, is not read
    junk = np.triu(rng.normal(size=(m, m)), 1) * 1e6
    assert np.array_equal(CR.product(np.tril(X) + junk, np.tril(Y) - junk), Cm)
    Ga = CR.antisymmetrize(rng.normal(size=(m, m)))
    Sy = CR.product(Ga, Y, 1, 2.0)
    assert np.array_equal(Sy, Sy.T) and np.array_equal(CR.product(np.tril(Ga, -1) + junk + np.diag(rng.normal(size=m)), Y, 1, 2.0), Sy)
    assert np.array_equal(Ga, -Ga.T) and not np.diag(Ga).any()
    if m == 1:
        assert Cm[0, 0] == 0.0 and Sy[0, 0] == 0.0


@pytest.mark.parametrize("m,n_occ", [(2, 1), (9, 4), (33, 12)])
def test_a_density_of_its_own_eigenvectors_is_stationary(m, n_occ):
    rng = rng_of(200 + m)
    H = LR.sym(rng.normal(size=(m, m)))
    w, V = np.linalg.eigh(H)
    D = 2.0 * V[:, :n_occ] @ V[:, :n_occ].T
    R = CR.product(H, D)
    assert np.abs(R).max() <= C * m * E * np.abs(w).max() * 2.0
    assert CR.norms(R)[1] == np.abs(R).max() and CR.norms(R)[0] == float((R * R).sum())
    # under an overlap: the generalised problem's density is stationary in the Löwdin basis
    S = DR.overlap(m, 1e2, rng)
    L = np.linalg.cholesky(S)
    wg, Yv = np.linalg.eigh(np.linalg.solve(L, np.linalg.solve(L, H).T).T)
    Cc = np.linalg.solve(L.T, Yv)
    Dg = 2.0 * Cc[:, :n_occ] @ Cc[:, :n_occ].T
    RL, HL, DL = CR.scf_residual(H, Dg, S)
    kap = np.linalg.cond(S)
    assert np.abs(RL).max() <= C * m * E * kap * np.abs(HL).max() * 2.0 * m
    # and equals S^(-1/2) (H D S - S D H) S^(-1/2)
    A, Ai = LR.functions(S)[:2]
    H2 = LR.sym(rng.normal(size=(m, m)))
    RL2 = CR.scf_residual(H2, Dg, S)[0]
    raw = Ai @ (H2 @ Dg @ S - S @ Dg @ H2) @ Ai
    assert np.abs(RL2 - raw).max() <= C * m * E * kap ** 2 * np.abs(raw).max() * m


@pytest.mark.parametrize("m,n_occ", [(2, 1), (9, 4), (33, 12), (17, 0), (17, 17)])
def test_the_norm_is_eight_times_the_occupied_virtual_block(m, n_occ):
    rng = rng_of(300 + m + n_occ)
    HL = LR.sym(rng.normal(size=(m, m)))
    Q = np.linalg.eigh(LR.sym(rng.normal(size=(m, m))))[1]         # the projector comes from ANOTHER matrix
    Qo, Qv = Q[:, :n_occ], Q[:, n_occ:]
    DL = 2.0 * Qo @ Qo.T
    sumsq = CR.norms(CR.product(HL, DL))[0]
    want = CR.ov_identity(HL, Qo, Qv)
    assert abs(sumsq - want) <= C * m * E * max(want, 1.0) * m
    if n_occ in (0, m):
        assert want == 0.0 and sumsq <= (C * m * E * np.abs(HL).max() * 2.0 * m) ** 2 * m * m


@pytest.mark.parametrize("m", [1, 3, 17])
def test_values_and_gradients_against_torch_autograd(m):
    rng = rng_of(400 + m)
    X0, Y0, G = rng.normal(size=(m, m)), rng.normal(size=(m, m)), rng.normal(size=(m, m))
    Xt, Yt = torch.tensor(X0, requires_grad=True), torch.tensor(Y0, requires_grad=True)
    Ct = CR.torch_commutator(Xt, Yt)
    (torch.from_numpy(G) * Ct).sum().backward()
    X, Y = LR.sym(X0), LR.sym(Y0)
    scale = C * m * E * max(np.abs(X).max() * np.abs(Y).max() * np.abs(G).max(), 1e-300) * m
    assert np.abs(CR.product(X, Y) - Ct.detach().numpy()).max() <= scale
    gX, gY = CR.commutator_backward(G, X, Y)
    assert np.array_equal(gX, gX.T) and np.array_equal(gY, gY.T)
    assert np.abs(gX - Xt.grad.numpy()).max() <= scale and np.abs(gY - Yt.grad.numpy()).max() <= scale
    # the symmetric part of the upstream gradient cannot reach a commutator of symmetric matrices
    g2 = CR.commutator_backward(G + 3.0 * LR.sym(rng.normal(size=(m, m))), X, Y)
    assert np.abs(g2[0] - gX).max() <= scale * 8 and np.abs(g2[1] - gY).max() <= scale * 8
    assert np.array_equal(CR.commutator_backward(CR.antisymmetrize(G), X, Y)[0], gX)


@pytest.mark.parametrize("m", [2, 9])
def test_residual_and_its_gradients_against_torch_autograd(m):
    rng = rng_of(500 + m)
    Qm = np.linalg.qr(rng.normal(size=(m, m)))[0]
    S = LR.sym((Qm * np.linspace(0.3, 1.6, m)[None, :]) @ Qm.T)    # well separated levels: the backward of eigh is a fair yardstick
    H, D, G = LR.sym(rng.normal(size=(m, m))), LR.sym(rng.normal(size=(m, m))), rng.normal(size=(m, m))
    Ht, Dt, St = (torch.tensor(a, requires_grad=True) for a in (H, D, S))
    Rt = CR.torch_scf_residual(Ht, Dt, St)
    (torch.from_numpy(G) * Rt).sum().backward()
    R, HL, DL = CR.scf_residual(H, D, S)
    A, Ai, s, Uv = LR.functions(S)
    kap, gap = s.max() / s.min(), 1.0 / LR.min_relative_gap(s)
    scale = C * m * E * kap ** 2 * m * m * max(np.abs(G).max(), 1.0) * max(np.abs(HL).max() * np.abs(DL).max(), 1.0)
    assert np.abs(R - Rt.detach().numpy()).max() <= scale
    gHL, gDL = CR.commutator_backward(G, HL, DL)
    YH, YD = LR.product(H, Ai), LR.product(D, A)
    gH, gAi = LR.congruence_backward(gHL, Ai, YH)
    gD, gA = LR.congruence_backward(gDL, A, YD)
    gS = LR.matfun_response(gAi, s, Uv, 1) + LR.matfun_response(gA, s, Uv, 0)
    assert np.abs(gH - LR.sym(Ht.grad.numpy())).max() <= scale and np.abs(gD - LR.sym(Dt.grad.numpy())).max() <= scale
    assert np.abs(gS - LR.sym(St.grad.numpy())).max() <= scale * gap * kap


def test_errors_restatement_counts_failed_molecules():
    rng = rng_of(600)
    Rs = [CR.product(LR.sym(rng.normal(size=(m, m))), LR.sym(rng.normal(size=(m, m)))) for m in (3, 5)]
    bad = np.full((4, 4), np.nan)
    out = CR.errors([Rs[0], bad, Rs[1]])
    assert out["failed"] == 1 and out["molecules"] == 2
    assert out["scf_residual_max"] == 0.5 * (np.abs(Rs[0]).max() + np.abs(Rs[1]).max())
    assert abs(out["scf_residual_rms"] - 0.5 * (np.sqrt((Rs[0] ** 2).mean()) + np.sqrt((Rs[1] ** 2).mean()))) <= 8 * E


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd import orbital_loss as OL
    from nabladft_amd import orbitals as O
    names = ("commutator", "scf_residual", "scf_residual_to_target", "ScfResidualLoss", "ScfTarget", "scf_target", "QHNetCommutatorLightning", "ScfResidualErrors")
    for name in names:
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    assert nq.ScfResidualErrors is O.ScfResidualErrors and "ScfResidualErrors" in O.__all__
    assert list(inspect.signature(OL.commutator).parameters) == ["X", "Y", "orbitals"]
    assert list(inspect.signature(OL.scf_residual).parameters) == ["H", "D", "basis"]
    assert list(inspect.signature(OL.scf_target).parameters) == ["H_target", "S", "plan", "n_occ"]
    assert OL.ScfTarget._fields == ("basis", "DL")
    assert OL.ScfResidualLoss.packed is True and issubclass(OL.ScfResidualLoss, OL._PackedMeanLoss)
    assert list(inspect.signature(OL.ScfResidualLoss.forward).parameters) == ["self", "R_pred", "R_target", "orb_ptr"]
    with pytest.raises(ValueError):
        OL.ScfResidualLoss(kind="rmse")
    assert issubclass(OL.QHNetCommutatorLightning, OL.QHNetLowdinLightning)
    assert inspect.signature(OL.QHNetCommutatorLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    assert OL.QHNetCommutatorLightning.KEYS == OL.QHNetLowdinLightning.KEYS + ("scf_residual",)
    assert OL.QHNetCommutatorLightning.CACHED == ("lowdin_inv_half", "lowdin_half", "target_density_lowdin")
    sig = inspect.signature(O.BatchedOrbitals.commutator).parameters
    assert list(sig) == ["self", "X", "Y", "x_anti", "alpha"] and sig["x_anti"].default is False and sig["alpha"].default == 1.0
    for name in ("commutator", "antisymmetrize", "commutator_norms"):
        assert callable(getattr(O.BatchedOrbitals, name)) and getattr(O.BatchedPurification, name) is getattr(O.BatchedOrbitals, name), name
    for name in ("reset", "update", "compute"):
        assert callable(getattr(O.ScfResidualErrors, name)), name
    want = {"nq_orb_comm_product": 10, "nq_orb_comm_antisymmetrize": 7, "nq_orb_comm_norms": 8}
    for s, nargs in want.items():
        assert s in _lib.SYMBOLS and hasattr(_lib.load(), s) and len(_lib.SYMBOLS[s][1]) == nargs, s
    assert _lib.load().nq_abi_version() == 17 and _lib.ABI_VERSION == 17
    doc = OL.scf_residual.__doc__
    for word in ("positive definite", "1024", "out of scope", "gap weighting", "order of the levels", "8 sum"):
        assert word in doc, word
    assert "SCF residual" in O.__doc__ and "scf_residual" in OL.__doc__


def test_python_refusals_without_a_device():
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals, LowdinBasis, ScfResidualErrors
    z4 = torch.zeros(4, dtype=torch.float64)
    fake = BatchedOrbitals.__new__(BatchedOrbitals)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.commutator(z4, z4, fake)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.scf_residual(z4, z4, None)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.scf_target(z4, z4, [0, 2], [1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.ScfResidualLoss()(z4, None, [0, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        ScfResidualErrors().update(z4, (LowdinBasis(fake, None, None, None, None), z4))
    with pytest.raises(RuntimeError, match="before any update"):
        ScfResidualErrors().compute()
    # the checks that come before the device is asked for
    with pytest.raises(TypeError, match="orbitals must be a BatchedOrbitals"):
        nq.commutator(z4, z4, object())
    with pytest.raises(TypeError, match="its basis a LowdinBasis"):
        ScfResidualErrors().update(z4, (object(), z4))
    assert LowdinBasis is nq.LowdinBasis and BatchedOrbitals is nq.BatchedOrbitals
