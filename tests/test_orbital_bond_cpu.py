"""CPU: the numpy restatement of the Mayer bond orders and their reverse (tests/orbital_bond_ref.py) against known answers and ``torch`` autograd, the public
surface of ``nabladft_amd.orbital_loss.bond_orders`` / ``BondOrderLoss`` / ``QHNetBondOrderLightning`` and the refusals that need no device.

Tolerances.  Known answers: a few roundings, stated at the test.  Sum rules: ``sum_B B_AB`` is a sum of ``n_A m`` products and ``sum_AB B_AB`` one of ``m^2``, so
the dot-product bound (K + 4) 2^-53 sum |terms| with that K (tests/orbital_bond_ref.py); the densities come from ``orbitals_ref.solve`` of pencils with
kappa_2(S) = 1e2, whose own departure from ``(DS)^2 = 2 DS`` is printed beside the bound.  Autograd: two float64 evaluations of the same sums in different
orders, the dot-product bound of the contraction."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import orbital_bond_ref as BR
import orbital_density_ref as DR
import orbitals_ref as R


def atoms(m, seed):
    """A partition of m orbitals into atoms of 1, 5, 14 and 32 orbitals (and a remainder) -> ptr."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ptr, o = [0], 0
    while o < m:
        o = min(m, o + int(rng.choice([1, 5, 14, 32])))
        ptr.append(o)
    return np.array(ptr)


def test_h2_in_a_minimal_basis_has_bond_order_one():
    for s in (0.0, 0.25, 0.6593, 0.9):
        S = np.array([[1.0, s], [s, 1.0]])
        c = np.ones(2) / np.sqrt(2.0 + 2.0 * s)                   # the bonding orbital, c^T S c = 1
        D = 2.0 * np.outer(c, c)
        P, B, V = BR.forward(D, S, np.array([0, 1, 2]))
        tol = 8 * 2.0 ** -52                                     # sqrt, two products and a sum per entry of P, one product per entry of B
        assert np.all(np.abs(P - 1.0) <= tol) and abs(B[0, 1] - 1.0) <= 2 * tol and B[0, 1] == B[1, 0] and np.all(np.abs(V - 1.0) <= 2 * tol)
        assert abs(B.sum() - 4.0) <= 8 * tol                     # = 2 n_elec


def test_sum_rules_of_an_idempotent_density():
    worst = 0.0
    for m, n_occ, seed in ((17, 5, 1), (65, 21, 2), (130, 43, 3), (20, 20, 4)):
        H, S = DR.gapped_case(m, n_occ, 0.3, 1e2, seed)
        eps, Cm = R.solve(H, S)
        D = 2.0 * Cm[:, :n_occ] @ Cm[:, :n_occ].T
        ptr = atoms(m, seed)
        P, B, V = BR.forward(D, S, ptr)
        a = BR.atom_of(ptr, m)
        pop = np.array([(D * S).sum(1)[a == A].sum() for A in range(len(ptr) - 1)])
        mag = np.array([(np.abs(P) * np.abs(P).T)[a == A].sum() for A in range(len(ptr) - 1)])
        sizes = np.diff(ptr)
        bound = (sizes * m + 4) * BR.U * mag
        fig = np.abs(B.sum(1) - 2.0 * pop) / bound
        total = abs(B.sum() - 4.0 * n_occ) / ((m * m + 4) * BR.U * mag.sum())
        idem = np.abs(P @ P - 2.0 * P).max() / np.abs(P).max()
        print(f"orbital_bond_parity sum rules (numpy) m={m} n_occ={n_occ} rows {fig.max():.3g} total {total:.3g} of the bound; |P^2 - 2P| / |P| {idem:.3g}")
        worst = max(worst, fig.max(), total)
        assert np.all(fig <= 1.0) and total <= 1.0, (m, fig.max(), total)
        assert np.array_equal(B, B.T)
        assert np.allclose(V, B.sum(1) - np.diag(B), rtol=0, atol=(len(ptr) + 4) * BR.U * np.abs(B).sum(1).max())
    assert worst > 0.0


def test_without_an_overlap_the_table_is_the_sum_of_squared_block_entries():
    rng = np.random.Generator(np.random.PCG64(5))
    m = 40
    D = BR.lower_sym(rng.normal(size=(m, m)))
    ptr = atoms(m, 5)
    P, B, V = BR.forward(D, None, ptr)
    assert np.array_equal(P, D)
    for A in range(len(ptr) - 1):
        for Bn in range(len(ptr) - 1):
            blk = D[ptr[A]:ptr[A + 1], ptr[Bn]:ptr[Bn + 1]]
            assert abs(B[A, Bn] - (blk ** 2).sum()) <= (blk.size + 2) * BR.U * (blk ** 2).sum()


def dense_torch(Dt, St, ptr):
    """The definitions once more, in torch on dense float64 matrices, for autograd."""
    Ds = 0.5 * (Dt + Dt.mT)
    P = Ds if St is None else Ds @ (0.5 * (St + St.mT))
    n = len(ptr) - 1
    rows = []
    for A in range(n):
        rows.append(torch.stack([(P[ptr[A]:ptr[A + 1], ptr[Bn]:ptr[Bn + 1]] * P[ptr[Bn]:ptr[Bn + 1], ptr[A]:ptr[A + 1]].mT).sum() for Bn in range(n)]))
    B = torch.stack(rows)
    return B, (B - torch.diag(torch.diag(B))).sum(1)


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("which", ["bond", "valence", "both"])
def test_reverse_against_torch_autograd(overlap, which):
    rng = np.random.Generator(np.random.PCG64(6))
    m = 37
    D = BR.lower_sym(rng.normal(size=(m, m)))
    S = BR.lower_sym(np.eye(m) + 0.1 * rng.normal(size=(m, m))) if overlap else None
    ptr = atoms(m, 6)
    n = len(ptr) - 1
    gB = rng.normal(size=(n, n)) if which != "valence" else None      # NOT symmetric
    gV = rng.normal(size=n) if which != "bond" else None
    Dt = torch.tensor(D, requires_grad=True)
    St = None if S is None else torch.tensor(S, requires_grad=True)
    B, V = dense_torch(Dt, St, ptr)
    loss = 0.0
    if gB is not None:
        loss = loss + (torch.from_numpy(gB) * B).sum()
    if gV is not None:
        loss = loss + (torch.from_numpy(gV) * V).sum()
    loss.backward()
    Pn, Bn, Vn = BR.forward(D, S, ptr)
    assert np.allclose(B.detach().numpy(), Bn, rtol=0, atol=float(BR.bond_bound(Pn, ptr).max()) * 2)
    E, gD, gS = BR.backward(D, S, ptr, gB, gV)
    ref_D = Dt.grad.numpy()
    assert np.array_equal(gD, gD.T) and np.allclose(ref_D, ref_D.T, rtol=0, atol=1e-13)
    bD = BR.backward_bound(E, np.eye(m) if S is None else S, False) + 4 * BR.U * np.abs(gD)
    assert np.all(np.abs(gD - ref_D) <= 2 * bD), float((np.abs(gD - ref_D) / bD).max())
    if S is None:
        assert gS is None
    else:
        bS = BR.backward_bound(E, D, True) + 4 * BR.U * np.abs(gS)
        assert np.all(np.abs(gS - St.grad.numpy()) <= 2 * bS), float((np.abs(gS - St.grad.numpy()) / bS).max())


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd import orbital_loss as OL
    from nabladft_amd import orbitals as O
    for name in ("bond_orders", "BondOrderLoss", "QHNetBondOrderLightning", "bond_layout", "dense_bond_orders"):
        assert getattr(nq, name) is getattr(OL, name) and name in nq.__all__ and name in OL.__all__, name
    assert nq.bond_layout is O.bond_layout and "bond_layout" in O.__all__ and "dense_bond_orders" in O.__all__
    sig = inspect.signature(OL.bond_orders).parameters
    assert list(sig) == ["D", "plan", "S_packed", "orbitals"] and sig["S_packed"].default is None and sig["orbitals"].default is None
    assert OL.BondOrderLoss.packed is True and inspect.signature(OL.BondOrderLoss.__init__).parameters["kind"].default == "mae"
    assert inspect.signature(OL.BondOrderLoss.__init__).parameters["charge"].default == 0
    with pytest.raises(ValueError):
        OL.BondOrderLoss(kind="rmse")
    assert issubclass(OL.QHNetBondOrderLightning, OL.QHNetDensityLightning)
    assert inspect.signature(OL.QHNetBondOrderLightning.__init__) == inspect.signature(nq.QHNetLightning.__init__)
    assert OL.QHNetBondOrderLightning.KEYS == ("orbital_energies", "density_matrix", "mulliken_charges", "bond_orders")
    assert OL.QHNetDensityLightning.KEYS == ("orbital_energies", "density_matrix", "mulliken_charges")
    for cls in (O.BatchedOrbitals, O.BatchedPurification):
        for name in ("bond_orders", "bond_orders_backward", "bond_product", "bond_reduce"):
            assert callable(getattr(cls, name)), name
    for sym in ("nq_orb_bond_product", "nq_orb_bond_reduce", "nq_orb_bond_backward"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.load(), sym), sym
    assert _lib.load().nq_abi_version() == 17
    doc = OL.bond_orders.__doc__
    assert "32" in doc and "Löwdin" in doc and "closed shells" in doc.lower() and "bond_orders" in OL.__doc__ and "bond_orders" in O.__doc__


def test_layout_helpers():
    import nabladft_amd as nq
    bp = nq.bond_layout([0, 2, 5, 6])
    assert bp.dtype == np.int64 and bp.tolist() == [0, 4, 13, 14]
    assert nq.bond_layout(torch.tensor([0, 3], dtype=torch.int32)).tolist() == [0, 9]
    flat = np.arange(14.0)
    assert nq.dense_bond_orders(flat, [0, 2, 5, 6], 1).tolist() == [[4.0, 5.0, 6.0], [7.0, 8.0, 9.0], [10.0, 11.0, 12.0]]
    t = nq.dense_bond_orders(torch.arange(14.0), [0, 2, 5, 6], 2)
    assert isinstance(t, torch.Tensor) and t.shape == (1, 1) and float(t) == 13.0
    with pytest.raises(ValueError):
        nq.bond_layout([0, 2, 2])                                # a molecule without atoms
    with pytest.raises(ValueError):
        nq.bond_layout([0])
    with pytest.raises(ValueError):
        nq.dense_bond_orders(flat[:13], [0, 2, 5, 6], 0)
    with pytest.raises(IndexError):
        nq.dense_bond_orders(flat, [0, 2, 5, 6], 3)


def test_cpu_tensors_are_refused():
    import nabladft_amd as nq
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.bond_orders(torch.zeros(4, dtype=torch.float64, requires_grad=True), None)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.bond_orders(torch.zeros(4, dtype=torch.float64), None, torch.zeros(4))
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.BondOrderLoss()(torch.zeros(4), torch.zeros(4), [0, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.BondOrderLoss("mse")(torch.zeros(5), torch.zeros(5), [0, 1, 3])


def test_bad_arguments_are_refused_before_any_device_work():
    """The entry points of csrc/orbbond.hip answer NQ_ERR_ARG from their argument checks (so this runs on a host without a GPU).  Skipped where a device is
    visible: a regression must not enqueue work on host buffers of a shared GPU."""
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    from nabladft_amd import _lib
    lib = _lib.load()
    host = (C.c_double * 256)()                                # stands in for every device array: nothing may read it
    p, q, r, s = (C.addressof(host) + 512 * i for i in range(4))
    ok = (2, 8, 34)                                            # orb_ptr [0, 3, 8]
    ARG = _lib.NQ_ERR_ARG
    prod, red, back = lib.nq_orb_bond_product, lib.nq_orb_bond_reduce, lib.nq_orb_bond_backward
    atoms_ok = (3, 5)                                          # N, Q: molecules of 1 and 2 atoms
    for dims in ((0, 0, 0), (2, 1, 1), (2, 8, 7), (1, 1025, 1025 * 1025), (2, 8, 8 * 1024 + 1)):
        assert prod(p, *dims, q, r, 1, s, None) == ARG, dims
        assert red(p, *dims, q, *atoms_ok, r, r, r, s, None, None) == ARG, dims
        assert back(p, *dims, q, None, r, None, None, 0, *atoms_ok, r, r, r, s, p, None, None) == ARG, dims
    assert prod(None, *ok, q, r, 1, s, None) == ARG and b"null" in lib.nq_last_error()
    assert prod(p, *ok, None, r, 1, s, None) == ARG and prod(p, *ok, q, r, 1, None, None) == ARG
    assert prod(p, *ok, q, r, 1, q, None) == ARG and b"operand" in lib.nq_last_error()
    for i in (0, 4, 7, 8, 9, 10):                              # state, P, mol_ptr, atom_orb_ptr, bond_ptr, out_bond
        args = [p, *ok, q, *atoms_ok, r, r, r, s, None, None]
        args[i] = None
        assert red(*args) == ARG and b"null" in lib.nq_last_error(), i
    for N, Q in ((1, 1), (3, 2), (3, 6), (3, -1), (5, 18)):     # fewer atoms than molecules; Q outside N .. (N - B + 1)^2 + B - 1
        assert red(p, *ok, q, N, Q, r, r, r, s, None, None) == ARG and (b"inconsistent" in lib.nq_last_error() or b"atoms for" in lib.nq_last_error()), (N, Q)
        assert back(p, *ok, q, None, r, None, None, 0, N, Q, r, r, r, s, p, None, None) == ARG, (N, Q)
    assert back(p, *ok, q, None, r, q, None, 0, *atoms_ok, r, r, r, s, None, p, None) == ARG and b"needs S" in lib.nq_last_error()
    assert back(p, *ok, q, None, r, None, r, 1, *atoms_ok, r, r, r, s, None, p, None) == ARG and b"needs D" in lib.nq_last_error()
    assert back(p, *ok, q, None, r, q, r, 1, *atoms_ok, r, r, r, s, p, None, None) == ARG and b"second input" in lib.nq_last_error()
    assert back(p, *ok, q, None, r, None, r, 1, *atoms_ok, r, r, r, s, None, None, None) == ARG and b"no output" in lib.nq_last_error()
    assert back(p, *ok, q, None, r, None, r, 1, *atoms_ok, r, r, None, s, p, None, None) == ARG and b"bond_ptr" in lib.nq_last_error()
    assert back(p, *ok, q, None, r, None, r, 1, *atoms_ok, r, r, r, None, p, None, None) == ARG and b"null" in lib.nq_last_error()
    assert back(p, *ok, q, None, r, None, r, 1, *atoms_ok, r, r, r, r, p, None, None) == ARG and b"of their own" in lib.nq_last_error()
    assert all(v == 0.0 for v in host)
