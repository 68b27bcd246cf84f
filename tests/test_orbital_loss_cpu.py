"""CPU: the yardstick of the orbital-energy gradients (tests/orbital_grad_ref.py) agrees with itself, and the host side of nabladft_amd.orbital_loss and of the
entry points of csrc/orbdens.hip.

The GPU test holds the device gradients to max(10, 4 x the spread of the two reference routes) units.  Ten is the bound the project holds this solver to; the
rule only keeps that meaning while the routes themselves agree to a quarter of it, which is asserted here (2.5 units) on every case the GPU test uses."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import orbital_grad_ref as G
import orbitals_ref as R

SPREAD_BOUND = 2.5         # a quarter of the GPU bound: with the 4 x rule the device is then held to the project's 10 units, not to the reference's own error


@pytest.mark.parametrize("kind", G.LOSSES)
def test_the_two_reference_routes_agree(kind):
    worst = np.zeros(2)
    for H, S in G.cases():
        m = H.shape[0]
        fH, fS, eps, gH, gS = G.spread(H, S, kind)
        worst = np.maximum(worst, [fH, fS])
        print(f"orbital_grad_parity reference {kind} m={m} gH {fH:.3f} gS {fS:.3f}")
        assert fH <= SPREAD_BOUND and fS <= SPREAD_BOUND, (kind, m, fH, fS)
        assert np.array_equal(gH, gH.T) and np.array_equal(gS, gS.T)
        assert np.abs(eps - R.solve(H, S)[0]).max() <= 10 * m * R.EPS * np.linalg.norm(H, 2) * R.spectral(H, S)[1]
    print(f"orbital_grad_parity reference {kind} worst gH {worst[0]:.3f} gS {worst[1]:.3f}")


def test_the_sign_of_the_overlap_gradient_by_finite_differences():
    """d eps_k = c_k^T (dH - eps_k dS) c_k: a central difference of the loss along a symmetric direction of S against <gS, dS>."""
    H, S = R.case(5, 1e2, 12)
    _, gH, gS = G.closed_form(H, S, "tanh")
    N = np.random.Generator(np.random.PCG64(3)).normal(size=(5, 5))
    dS = 1e-6 * (N + N.T)
    f = lambda s: float(np.tanh(0.1 * R.solve(H, s)[0]).sum())
    fd = (f(S + dS) - f(S - dS)) / 2.0
    assert abs(fd - float((gS * dS).sum())) <= 1e-6 * abs(fd)
    fdH = (float(np.tanh(0.1 * R.solve(H + dS, S)[0]).sum()) - float(np.tanh(0.1 * R.solve(H - dS, S)[0]).sum())) / 2.0
    assert abs(fdH - float((gH * dS).sum())) <= 1e-6 * abs(fdH)


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import orbital_loss as OL
    from nabladft_amd import orbitals as O
    for name in ("orbital_energies", "OrbitalEnergyLoss", "QHNetOrbitalLightning", "mulliken_charges"):
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    assert nq.mulliken_charges is O.mulliken_charges and "mulliken_charges" in O.__all__
    assert list(inspect.signature(OL.orbital_energies).parameters) == ["H_packed", "S_packed", "plan_or_orb_ptr", "return_solution"]
    assert inspect.signature(OL.orbital_energies).parameters["return_solution"].default is False
    sig = inspect.signature(OL.OrbitalEnergyLoss.__init__).parameters
    assert list(sig) == ["self", "kind", "which", "charge"] and (sig["kind"].default, sig["which"].default, sig["charge"].default) == ("mae", "occupied", 0)
    assert list(inspect.signature(OL.OrbitalEnergyLoss.forward).parameters) == ["self", "eps_pred", "eps_target", "n_occ", "orb_ptr"]
    assert OL.OrbitalEnergyLoss.packed is True
    assert list(inspect.signature(O.BatchedOrbitals.density).parameters) == ["self", "n_occ", "energy_weighted"]
    assert inspect.signature(O.BatchedOrbitals.density).parameters["energy_weighted"].default is False
    assert list(inspect.signature(O.BatchedOrbitals.populations).parameters) == ["self", "D", "plan", "S_packed", "H_packed"]
    assert list(inspect.signature(O.mulliken_charges).parameters) == ["z", "atom_pop"]
    assert issubclass(OL.QHNetOrbitalLightning, nq.QHNetLightning)
    assert inspect.signature(OL.QHNetOrbitalLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    for bad in (dict(kind="rmse"), dict(which="virtual")):
        with pytest.raises(ValueError):
            OL.OrbitalEnergyLoss(**bad)
    # the documents say what flows and what does not
    assert "No gradient flows" in O.__doc__ and "orbital_loss" in O.__doc__
    assert "torch.linalg.eigh" in OL.__doc__ and "No gradient flows through the eigenvectors" in OL.__doc__
    # Mulliken charges are plain arithmetic
    q = nq.mulliken_charges([8, 1, 1], torch.tensor([8.5, 0.75, 0.75], dtype=torch.float64))
    assert q.dtype == torch.float64 and q.tolist() == [-0.5, 0.25, 0.25]
    with pytest.raises(ValueError):
        nq.mulliken_charges([8, 1], torch.zeros(3, dtype=torch.float64))


def test_cpu_tensors_are_refused():
    import nabladft_amd as nq
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.orbital_energies(torch.zeros(4, requires_grad=True), None, [0, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.orbital_energies(torch.zeros(4), torch.zeros(4), [0, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.OrbitalEnergyLoss()(torch.zeros(2), torch.zeros(2), [1], [0, 2])


def test_phisnet_flag_exists_and_defaults_to_false():
    from nabladft_amd.phisnet import NeuralNetwork
    m = NeuralNetwork(max_orbitals=(((6, 0), (6, 1)),), order=1, num_features=32, num_basis_functions=8, num_modules=1, num_residual_pre_x=1,
                      num_residual_post_x=1, num_residual_pre_vi=1, num_residual_pre_vj=1, num_residual_post_v=1, num_residual_output=1, num_residual_pc=1,
                      num_residual_pn=1, num_residual_ii=1, num_residual_ij=1, num_residual_full_ii=1, num_residual_full_ij=1, num_residual_core_ii=1,
                      num_residual_core_ij=1, num_residual_over_ij=1, basis_functions="exp-bernstein", cutoff=8.0, activation="swish")
    assert m.orbital_gradients is False and m.calculate_orbitals is False


def test_bad_arguments_are_refused_before_any_device_work():
    """nq_orb_wgram / nq_orb_population answer NQ_ERR_ARG from their argument checks (so this runs on a host without a GPU).  Skipped where a device is
    visible: a regression must not enqueue work on host buffers of a shared GPU."""
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    from nabladft_amd import _lib
    lib = _lib.load()
    host = (C.c_double * 64)()                                 # stands in for every device array: nothing may read it
    p = C.addressof(host)
    ok = (2, 8, 34)                                            # orb_ptr [0, 3, 8]
    ARG = _lib.NQ_ERR_ARG
    assert lib.nq_orb_wgram(None, *ok, p, None, None, None, p, None, None) == ARG and b"null" in lib.nq_last_error()
    assert lib.nq_orb_wgram(p, *ok, None, None, None, None, p, None, None) == ARG
    assert lib.nq_orb_wgram(p, *ok, p, None, None, None, None, None, None) == ARG
    assert lib.nq_orb_wgram(p, *ok, p, p, None, None, p, None, None) == ARG and b"second output" in lib.nq_last_error()
    for dims in ((0, 0, 0), (2, 1, 1), (2, 8, 7), (1, 1025, 1025 * 1025), (2, 8, 8 * 1024 + 1)):
        assert lib.nq_orb_wgram(p, *dims, p, None, None, None, p, None, None) == ARG, dims
        assert lib.nq_orb_population(p, *dims, p, None, 0, None, 0, 4, p, p, p, p, None, None) == ARG, dims
    assert lib.nq_orb_population(None, *ok, p, None, 0, None, 0, 4, p, p, p, p, None, None) == ARG
    assert lib.nq_orb_population(p, *ok, None, None, 0, None, 0, 4, p, p, p, p, None, None) == ARG
    assert lib.nq_orb_population(p, *ok, p, None, 0, None, 0, 4, None, p, p, p, None, None) == ARG
    assert lib.nq_orb_population(p, *ok, p, None, 0, None, 0, 4, p, None, p, p, None, None) == ARG
    assert lib.nq_orb_population(p, *ok, p, None, 0, None, 0, 4, p, p, None, p, None, None) == ARG
    assert lib.nq_orb_population(p, *ok, p, None, 0, None, 0, 4, p, p, p, None, None, None) == ARG
    assert lib.nq_orb_population(p, *ok, p, None, 0, None, 0, 4, p, p, p, p, p, None) == ARG and b"needs H" in lib.nq_last_error()
    assert lib.nq_orb_population(p, *ok, p, None, 0, None, 0, 1, p, p, p, p, None, None) == ARG and b"atoms" in lib.nq_last_error()
    assert all(v == 0.0 for v in host)
