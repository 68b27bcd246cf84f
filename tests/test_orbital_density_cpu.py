"""CPU: the yardstick of the density-matrix gradients (tests/orbital_density_ref.py) agrees with itself, and the host side of the density part of
nabladft_amd.orbital_loss and of the entry points of csrc/orbresp.hip.

The GPU test holds the device gradients to max(10, 4 x the spread of the two reference routes) units, ten being the project's bound for the solver.  Here the
routes themselves are held to 1 unit on the generalized problems the GPU test uses (float64 and float32-rounded inputs), and to 2.5 units -- a quarter of the
GPU bound, the rule of tests/test_orbital_loss_cpu.py -- on the standard problem (S = None), whose unit has no condition number in it and is a few roundings
wide at m = 3.  Where every orbital is occupied the loss carries no energy term: D = 2 S^-1 does not depend on H, the closed form's dL/dH is exactly zero,
and route (a), which divides by differences of occupied levels on the way to that zero, is no yardstick for it."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import orbital_density_ref as DR

GENERAL_BOUND = 1.0
STANDARD_BOUND = 2.5


def case_loss(case):
    m, n_occ, seed = case[0], case[1], case[4]
    G, T = DR.upstream(m, seed)
    return DR.quadratic_loss(G, T, with_eps=n_occ < m)


@pytest.mark.parametrize("inputs", ["float64", "float32", "standard"])
def test_the_two_reference_routes_agree(inputs):
    worst = np.zeros(2)
    for case in DR.CASES:
        m, n_occ = case[0], case[1]
        H, S = DR.gapped_case(*case, standard=inputs == "standard")
        if inputs == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        fH, fS, eps, D, gH, gS = DR.spread(H, S, n_occ, case_loss(case))
        bH = DR.closed_form(H, S, n_occ, case_loss(case))[2]
        if n_occ == m:
            assert np.all(bH == 0.0), case                       # the closed form: no virtual orbital, no dL/dH
            fH = 0.0
        worst = np.maximum(worst, [fH, fS])
        print(f"orbital_density_parity reference {inputs} m={m} n_occ={n_occ} kappa0={case[3]:g} gH {fH:.3f} gS {fS:.3f}")
        bound = STANDARD_BOUND if inputs == "standard" else GENERAL_BOUND
        assert fH <= bound and fS <= bound, (case, fH, fS)
        assert np.array_equal(D, D.T) or np.abs(D - D.T).max() <= 1e-12 * np.abs(D).max()
        if n_occ < m:
            assert eps[n_occ] - eps[n_occ - 1] >= 0.29           # the prescribed gap survives the construction (and the float32 rounding)
    print(f"orbital_density_parity reference {inputs} worst gH {worst[0]:.3f} gS {worst[1]:.3f}")


def test_closed_form_is_a_yardstick_where_two_occupied_levels_coincide():
    """Two equal occupied levels: route (b) is finite and agrees with itself under another permutation; route (a) is off by many orders (printed, not held
    to anything: this is where it is not a yardstick)."""
    H, S = DR.gapped_case(65, 21, 0.3, 1e2, 5, degenerate=True)
    G, T = DR.upstream(65, 5)
    loss = DR.quadratic_loss(G, T, with_eps=False)
    eps, _, gH, gS = DR.closed_form(H, S, 21, loss)
    _, _, gH2, gS2 = DR.closed_form(H, S, 21, loss, seed=3)
    assert abs(eps[1] - eps[0]) <= 1e-12 and np.isfinite(gH).all() and np.isfinite(gS).all()
    uH, uS = DR.units(H, S, 21, eps, gH, gS)
    fH, fS = np.abs(gH - gH2).max() / uH, np.abs(gS - gS2).max() / uS
    aH = np.abs(DR.autograd(H, S, 21, loss)[2] - gH).max() / uH
    print(f"orbital_density_parity reference degenerate closed form vs closed form gH {fH:.3g} gS {fS:.3g}; autograd vs closed form gH {aH:.3g}")
    assert fH <= GENERAL_BOUND and fS <= GENERAL_BOUND


def test_response_by_finite_differences():
    """The signs and factors of the closed form: a central difference of the loss along symmetric directions of H and S."""
    H, S = DR.gapped_case(6, 2, 0.3, 1e2, 3)
    G, T = DR.upstream(6, 3)
    loss = DR.quadratic_loss(G, T)
    _, _, gH, gS = DR.closed_form(H, S, 2, loss)
    N = np.random.Generator(np.random.PCG64(4)).normal(size=(6, 6))
    d = 1e-6 * (N + N.T)

    def f(h, s):
        eps, Cm = DR.R.solve(h, s)
        Dm = 2.0 * Cm[:, :2] @ Cm[:, :2].T
        return float(loss(torch.from_numpy(eps), torch.from_numpy(Dm), None, None))
    fdH, fdS = (f(H + d, S) - f(H - d, S)) / 2.0, (f(H, S + d) - f(H, S - d)) / 2.0
    assert abs(fdH - float((gH * d).sum())) <= 1e-5 * abs(fdH) and abs(fdS - float((gS * d).sum())) <= 1e-5 * abs(fdS)


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd import orbital_loss as OL
    from nabladft_amd import orbitals as O
    names = ("orbital_solution", "density_matrix", "populations", "DensityMatrixLoss", "MullikenChargeLoss", "QHNetDensityLightning")
    for name in names:
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    sig = inspect.signature(OL.orbital_solution).parameters
    assert list(sig) == ["H_packed", "S_packed", "plan_or_orb_ptr", "n_occ", "return_solution"] and sig["return_solution"].default is False
    assert list(inspect.signature(OL.density_matrix).parameters) == list(sig)
    sig = inspect.signature(OL.populations).parameters
    assert list(sig)[:4] == ["D", "plan", "S_packed", "H_packed"] and all(sig[k].default is None for k in list(sig)[2:])
    for cls in (OL.DensityMatrixLoss, OL.MullikenChargeLoss):
        assert cls.packed is True and inspect.signature(cls.__init__).parameters["kind"].default == "mae"
        with pytest.raises(ValueError):
            cls(kind="rmse")
    assert issubclass(OL.QHNetDensityLightning, OL.QHNetOrbitalLightning)
    assert inspect.signature(OL.QHNetDensityLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    assert OL.QHNetDensityLightning.KEYS == ("orbital_energies", "density_matrix", "mulliken_charges")
    for name in ("occupied_layout", "resp_project", "resp_mo", "resp_back", "syr2k", "density_response", "populations_backward"):
        assert callable(getattr(O.BatchedOrbitals, name)), name
    for sym in ("nq_orb_resp_project", "nq_orb_resp_mo", "nq_orb_resp_back", "nq_orb_syr2k", "nq_orb_population_backward"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.load(), sym), sym
    assert _lib.load().nq_abi_version() == 17
    # the documents say what is divided by and what happens at a vanishing gap
    doc = OL.orbital_solution.__doc__
    assert "No gap regularisation" in doc and "frontier" in doc and "inf / NaN" in doc
    assert "orbital_solution" in OL.__doc__ and "orbital_loss" in O.__doc__


def test_cpu_tensors_are_refused():
    import nabladft_amd as nq
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.orbital_solution(torch.zeros(4, requires_grad=True), None, [0, 2], [1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.density_matrix(torch.zeros(4), torch.zeros(4), [0, 2], [1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.populations(torch.zeros(4, dtype=torch.float64), None)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.DensityMatrixLoss()(torch.zeros(4), torch.zeros(4), [0, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.MullikenChargeLoss()(torch.zeros(2), torch.zeros(2), [0, 2])


def test_bad_arguments_are_refused_before_any_device_work():
    """The entry points of csrc/orbresp.hip answer NQ_ERR_ARG from their argument checks (so this runs on a host without a GPU).  Skipped where a device is
    visible: a regression must not enqueue work on host buffers of a shared GPU."""
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    from nabladft_amd import _lib
    lib = _lib.load()
    host = (C.c_double * 64)()                                 # stands in for every device array: nothing may read it
    p = C.addressof(host)
    ok = (2, 8, 34)                                            # orb_ptr [0, 3, 8]
    ARG = _lib.NQ_ERR_ARG
    chain = {"nq_orb_resp_project": (3, 0), "nq_orb_resp_mo": (2, 1), "nq_orb_resp_back": (2, 2), "nq_orb_syr2k": (2, 2)}   # required / optional arrays
    for name, (req, opt) in chain.items():
        fn = getattr(lib, name)
        full = [p] * (req + opt)
        if opt == 2:
            full = [p, p, p, p]                                  # in0, in1, out0, out1
        assert fn(None, *ok, p, p, 16, *full, None) == ARG and b"null" in lib.nq_last_error(), name
        assert fn(p, *ok, None, p, 16, *full, None) == ARG and b"n_occ" in lib.nq_last_error(), name
        assert fn(p, *ok, p, None, 16, *full, None) == ARG and b"occ_ptr is missing" in lib.nq_last_error(), name
        assert fn(p, *ok, p, p, -1, *full, None) == ARG and fn(p, *ok, p, p, 35, *full, None) == ARG, name
        for dims in ((0, 0, 0), (2, 1, 1), (2, 8, 7), (1, 1025, 1025 * 1025), (2, 8, 8 * 1024 + 1)):
            assert fn(p, *dims, p, p, 16, *full, None) == ARG, (name, dims)
        required = [0, 1, 2] if name == "nq_orb_resp_project" else ([0, 1] if opt == 1 else [0, 2])
        for i in required:
            args = list(full)
            args[i] = None
            assert fn(p, *ok, p, p, 16, *args, None) == ARG and b"null" in lib.nq_last_error(), (name, i)
        if opt == 2:
            assert fn(p, *ok, p, p, 16, p, p, p, None, None) == ARG and b"second output" in lib.nq_last_error(), name
    assert lib.nq_orb_resp_project(p, *ok, p, p, 16, p, p, p, None) == ARG and b"must not be G" in lib.nq_last_error()
    pb = lib.nq_orb_population_backward
    tail = (4, p, p)                                             # N, mol_ptr, atom_orb_ptr
    for dims in ((0, 0, 0), (2, 1, 1), (2, 8, 7), (1, 1025, 1025 * 1025), (2, 8, 8 * 1024 + 1)):
        assert pb(p, *dims, p, p, None, None, None, 0, None, 0, *tail, p, None, None, None) == ARG, dims
    assert pb(None, *ok, p, p, None, None, None, 0, None, 0, *tail, p, None, None, None) == ARG
    assert pb(p, *ok, p, p, None, None, None, 0, None, 0, 4, None, p, p, None, None, None) == ARG
    assert pb(p, *ok, p, p, None, None, None, 0, None, 0, 4, p, None, p, None, None, None) == ARG
    assert pb(p, *ok, p, p, None, None, None, 0, None, 0, *tail, None, None, None, None) == ARG
    assert pb(p, *ok, p, p, None, None, None, 0, p, 1, *tail, p, p, None, None) == ARG and b"need D" in lib.nq_last_error()
    assert pb(p, *ok, p, p, None, p, None, 0, None, 0, *tail, p, p, None, None) == ARG and b"needs S" in lib.nq_last_error()
    assert pb(p, *ok, p, p, p, p, None, 0, None, 0, *tail, p, None, None, None) == ARG and b"needs H" in lib.nq_last_error()
    assert pb(p, *ok, p, p, None, p, None, 0, None, 0, *tail, p, None, p, None) == ARG and b"needs H" in lib.nq_last_error()
    assert pb(p, *ok, p, p, None, None, None, 0, None, 0, 1, p, p, p, None, None, None) == ARG and b"atoms" in lib.nq_last_error()
    assert all(v == 0.0 for v in host)
