"""CPU: the yardstick of the Fermi-smearing gradients (tests/orbital_smearing_ref.py) agrees with itself and with finite differences, and the host side of
``smeared_solution`` / ``electron_counts`` and of the entry points of csrc/orbsmear.hip.

The GPU test holds the device gradients to max(10, 4 x the spread of the two reference routes) units.  Here the routes themselves are held to 1 unit on the
generalized problems (float64 and float32-rounded inputs) and to 2.5 units on the standard problem (S = None), the rule of tests/test_orbital_density_cpu.py.
Where levels coincide route (a), which divides by their differences, is no yardstick: its deviation is printed, the closed form is held to itself under
another permutation and to central differences of a label-invariant loss."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_smearing_ref as SR

GENERAL_BOUND = 1.0
STANDARD_BOUND = 2.5


@pytest.mark.parametrize("inputs", ["float64", "float32", "standard"])
def test_the_two_reference_routes_agree(inputs):
    worst = np.zeros(2)
    for case in SR.CASES:
        m, no, gap, k0, seed, ne, kT = case
        H, S = DR.gapped_case(m, no, gap, k0, seed, standard=inputs == "standard")
        if inputs == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        G, T, w = SR.upstream(m, seed)
        fH, fS, a = SR.spread(H, S, ne, kT, SR.full_loss(G, T, w))
        worst = np.maximum(worst, [fH, fS])
        print(f"orbital_smearing_parity reference {inputs} m={m} n_elec={ne:g} kT={kT:g} gap={gap:g} kappa0={k0:g} gH {fH:.3f} gS {fS:.3f}")
        bound = STANDARD_BOUND if inputs == "standard" else GENERAL_BOUND
        assert fH <= bound and fS <= bound, (case, fH, fS)
        assert abs(a[2].sum() - ne) <= 1e-12 * ne and 0.0 < ne < 2 * m
    print(f"orbital_smearing_parity reference {inputs} worst gH {worst[0]:.3f} gS {worst[1]:.3f}")


def test_closed_form_at_coincident_levels():
    for m, no, seed, ne, kT, kind in SR.COINCIDENT:
        H, S = SR.coincident_case(m, no, seed, kind)
        G, T, w = SR.upstream(m, seed)
        loss = SR.full_loss(G, T, w, label_invariant=True)
        b, b2 = SR.closed_form(H, S, ne, kT, loss), SR.closed_form(H, S, ne, kT, loss, seed=3)
        eps = b[0]
        assert abs(eps[no] - eps[no - 1]) <= 1e-12 and np.isfinite(b[5]).all() and np.isfinite(b[6]).all()
        if kind == "crossed":
            assert abs(eps[no]) <= 1e-12
        uH, uS = SR.units(H, S, eps, b[3], kT, b[5], b[6])
        fH, fS = np.abs(b[5] - b2[5]).max() / uH, np.abs(b[6] - b2[6]).max() / uS
        N = np.random.Generator(np.random.PCG64(4)).normal(size=(m, m))
        d = 1e-5 * (N + N.T)
        fdH, fdS = SR.finite_difference(H, S, ne, kT, loss, dH=d), SR.finite_difference(H, S, ne, kT, loss, dS=d)
        rH, rS = abs(fdH - float((b[5] * d).sum())) / abs(fdH), abs(fdS - float((b[6] * d).sum())) / abs(fdS)
        a = SR.autograd(H, S, ne, kT, loss)
        print(f"orbital_smearing_parity reference coincident {kind} m={m} kT={kT:g}: closed form vs itself gH {fH:.3g} gS {fS:.3g}; vs central differences "
              f"gH {rH:.2e} gS {rS:.2e}; autograd vs closed form gH {np.abs(a[5] - b[5]).max() / uH:.3g} units (not bounded)")
        assert fH <= GENERAL_BOUND and fS <= GENERAL_BOUND, (m, kind, fH, fS)
        assert rH <= 1e-5 and rS <= 1e-5, (m, kind, rH, rS)


def test_zero_temperature_limit_is_the_closed_shell_closed_form():
    for case in DR.CASES:
        m, no, gap, k0, seed = case
        if no == m:
            continue
        H, S = DR.gapped_case(*case)
        G, T = DR.upstream(m, seed)
        a = DR.closed_form(H, S, no, DR.quadratic_loss(G, T))
        b = SR.closed_form(H, S, 2.0 * no, gap / 200.0, SR.density_loss(G, T))
        uH, uS = DR.units(H, S, no, a[0], a[2], a[3])
        fH, fS = np.abs(a[2] - b[5]).max() / uH, np.abs(a[3] - b[6]).max() / uS
        print(f"orbital_smearing_parity reference zero-temperature limit m={m} n_occ={no} gH {fH:.3g} gS {fS:.3g}")
        assert fH <= GENERAL_BOUND and fS <= GENERAL_BOUND, (case, fH, fS)
        assert np.abs(b[2] - np.where(np.arange(m) < no, 2.0, 0.0)).max() <= 1e-40 and b[4] <= 1e-30


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd import orbital_loss as OL
    from nabladft_amd import orbitals as O
    for name in ("smeared_solution", "smeared_density_matrix", "SmearedSolution", "QHNetSmearedDensityLightning", "electron_counts"):
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    assert nq.electron_counts is O.electron_counts and "electron_counts" in O.__all__ and "FermiResult" in O.__all__ and nq.FermiResult is O.FermiResult
    sig = inspect.signature(OL.smeared_solution).parameters
    assert list(sig) == ["H_packed", "S_packed", "plan_or_orb_ptr", "n_elec", "kT", "return_solution"] and sig["return_solution"].default is False
    assert list(inspect.signature(OL.smeared_density_matrix).parameters) == list(sig)
    assert OL.SmearedSolution._fields == ("eps", "D", "occ", "mu", "entropy")
    sig = inspect.signature(O.electron_counts).parameters
    assert list(sig)[:3] == ["z", "ptr", "charge"] and sig["charge"].default == 0
    sig = inspect.signature(O.BatchedOrbitals.smeared_response).parameters
    assert list(sig) == ["self", "G", "fermi_result", "g_eps", "g_occ", "g_mu", "g_ent", "overlap"] and sig["overlap"].default is True
    assert all(sig[k].default is None for k in ("g_eps", "g_occ", "g_mu", "g_ent"))
    assert list(inspect.signature(O.BatchedOrbitals.fermi).parameters) == ["self", "n_elec", "kT"]
    sig = inspect.signature(O.BatchedOrbitals.smeared_density).parameters
    assert list(sig) == ["self", "occ", "energy_weighted"] and sig["energy_weighted"].default is False
    assert issubclass(OL.QHNetSmearedDensityLightning, OL.QHNetDensityLightning) and OL.QHNetSmearedDensityLightning.kT == 0.01
    assert inspect.signature(OL.QHNetSmearedDensityLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    assert not hasattr(OL, "electronic_free_energy_terms")
    for sym in ("nq_orb_fermi", "nq_orb_smear_mo", "nq_orb_smear_diag", "nq_orb_smear_back"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.load(), sym), sym
    assert _lib.load().nq_abi_version() == 17
    phrase = "without dividing by a difference of orbital energies"
    for doc in (OL.smeared_solution.__doc__, OL.smeared_density_matrix.__doc__, O.BatchedOrbitals.smeared_response.__doc__, OL.__doc__, O.__doc__):
        assert phrase in " ".join(doc.split()), doc[:80]
    assert "Smearing" in OL.__doc__ and "unchanged" in OL.__doc__ and "No gap regularisation" in OL.orbital_solution.__doc__


def test_cpu_tensors_are_refused_and_electron_counts_raises():
    import nabladft_amd as nq
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.smeared_solution(torch.zeros(4, requires_grad=True), None, [0, 2], 2.0, 0.01)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.smeared_density_matrix(torch.zeros(4), torch.zeros(4), [0, 2], [2.0], [0.01])
    z, ptr = [8, 1, 1, 1, 3], [0, 3, 4, 5]
    ne = nq.electron_counts(z, ptr)
    assert ne.dtype == torch.float64 and ne.tolist() == [10.0, 1.0, 3.0]                 # odd counts are fine
    assert nq.electron_counts(z, ptr, [1, 0, -1], [0, 7, 9, 14]).tolist() == [9.0, 1.0, 4.0]
    assert nq.electron_counts(z, ptr, 0.5).tolist() == [9.5, 0.5, 2.5]
    with pytest.raises(ValueError, match=r"molecule 1 has 0 electrons"):
        nq.electron_counts(z, ptr, [0, 1, 0])
    with pytest.raises(ValueError, match=r"molecule 2 has -1 electrons"):
        nq.electron_counts(z, ptr, [0, 0, 4])
    with pytest.raises(ValueError, match=r"molecule 0 has 10 electrons for m=5"):
        nq.electron_counts(z, ptr, 0, [0, 5, 9, 14])
    with pytest.raises(ValueError, match="without atoms"):
        nq.electron_counts(z, [0, 3, 3, 5])
    with pytest.raises(ValueError, match="open shells"):                                 # occupied_counts stays as it is
        nq.occupied_counts(z, ptr)


def test_bad_arguments_are_refused_before_any_device_work():
    """The entry points of csrc/orbsmear.hip answer NQ_ERR_ARG from their argument checks (so this runs on a host without a GPU).  Skipped where a device is
    visible: a regression must not enqueue work on host buffers of a shared GPU."""
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    from nabladft_amd import _lib
    lib = _lib.load()
    host = (C.c_double * 64)()
    p = C.addressof(host)
    ok = (2, 8, 34)
    ARG = _lib.NQ_ERR_ARG
    # entry point -> (number of array arguments, indices of the required ones)
    table = {"nq_orb_fermi": (7, range(7)), "nq_orb_smear_mo": (6, (0, 1, 2, 3, 5)), "nq_orb_smear_diag": (11, (0, 1, 2, 3, 4, 9)), "nq_orb_smear_back": (4, (0, 2))}
    for name, (n, required) in table.items():
        fn = getattr(lib, name)
        full = [p] * n
        assert fn(None, *ok, *full, None) == ARG and b"null" in lib.nq_last_error(), name
        for dims in ((0, 0, 0), (2, 1, 1), (2, 8, 7), (1, 1025, 1025 * 1025), (2, 8, 8 * 1024 + 1)):
            assert fn(p, *dims, *full, None) == ARG, (name, dims)
        for i in required:
            args = list(full)
            args[i] = None
            if name == "nq_orb_smear_back" and i == 2:
                args[1] = args[3] = None
            assert fn(p, *ok, *args, None) == ARG and b"null" in lib.nq_last_error(), (name, i)
    assert lib.nq_orb_smear_back(p, *ok, p, p, p, None, None) == ARG and b"second output" in lib.nq_last_error()
    assert all(v == 0.0 for v in host)
