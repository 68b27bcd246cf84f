"""GPU: the bond-order kernels (csrc/orbbond.hip) through the C ABI and through ``BatchedOrbitals.bond_orders`` / ``nabladft_amd.orbital_loss.bond_orders`` /
``BondOrderLoss`` / ``QHNetBondOrderLightning``, against the numpy restatement (tests/orbital_bond_ref.py) and the float64 yardstick of the solver route
(tests/orbital_density_ref.py).

Bounds (U = 2^-53; ``orbital_bond_ref`` states them).  Product: |P - ref| <= (m + 4) U (|D||S|) per entry, reference in extended precision.  Reduce: each B_AB
within (n_A n_B + 2) U sum |P_mu,nu P_nu,mu| of the same sum on the same P; the valence within the bound of a row sum of those entries.  Reverse: E is one
sum of four numbers and one product, compared bit for bit on integers and within 4 U |E| on random data; the two gradients within (2 m + 4) U of half the sum
of the two contractions' magnitudes, on the device's own E.  Small integers make every one of these sums exact: compared bit for bit (the sign of a zero
aside).  At m = 1024 the reference is plain float64 numpy, whose own rounding shares the bound.

End to end (test 4).  The yardstick is ``orbital_density_ref.autograd`` (torch.linalg Cholesky -> eigh -> D, autograd through all of it) followed by the dense
definitions in torch.  Its own spread is measured first: the same route on a copy with the atoms reordered and the orbitals inside every atom shuffled,
mapped back.  Allowance per quantity: max(10 x that spread, the propagated bound).  The propagated bound of the table and the valences: the dot-product
bounds of the product and the reduction plus the density's own unit carried through them (|dD| <= 10 U_D, U_D = ``orbital_purify_ref.density_unit``, the
bound tests/test_orbital_purify_gpu.py holds a density to; |dP| <= |dD||S|, |dB_AB| <= sum |dP_mu,nu||P_nu,mu| + |P_mu,nu||dP_nu,mu|).  Of the gradients: ten
units of ``orbital_density_ref.units``, the bound the response chain they flow through is held to.  Float32 results are allowed their own rounding, 2^-24 per
element: of dL/dH, and for dL/dS of each of the two float32 terms autograd adds (the one ``bond_orders`` hands back for S itself and the one that arrives
through D) and of their float32 sum.  The figures are printed in units of the spread and of the allowance as ``orbital_bond_parity ...`` lines (kept in profiles/orbital_bond_parity.txt).

Sum rules (test 5).  For D = 2 C_o C_o^T with C_o^T S C_o = I + Delta: (DS)^2 = 2 DS + 4 C_o Delta C_o^T S, so sum_B B_AB - 2 pop_A is the dot-product error
of n_A m products plus twice the relative departure from idempotency times sum |P_mu,nu P_nu,mu|: 10 m 2^-52 kappa_2(S) for the solver (the bound
tests/test_orbitals_gpu.py holds C^T S C = I to), 10 U_D / max|D| for the purified density."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import orbital_bond_ref as BR
import orbital_density_ref as DR
import orbital_purify_ref as PR
import orbitals_ref as R
from test_orbital_loss_gpu import blocks, db_plan, i32
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, ptrs, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 17, 37, 63, 64, 65, 127, 128, 129, 130]         # one orbital .. across the 64- and 128-orbital tile edges
PATTERN = [32, 14, 5, 32, 1, 14, 32, 5, 1]                        # atoms of 1, 5, 14 and 32 orbitals: [51, 83) straddles 64, [98, 130) straddles 128
SENTINEL = -7.25e300
GUARD = 64
U = BR.U


def partition(m, shift=0):
    """Atom sizes of a molecule of m orbitals: the pattern from position ``shift``, the last atom cut at m."""
    out, o, k = [], 0, shift
    while o < m:
        s = min(PATTERN[k % len(PATTERN)], m - o)
        out.append(s)
        o, k = o + s, k + 1
    return out


def make_batch(ms, parts):
    """-> namespace: ``plan`` (what the launches read of a plan), ``ptr`` (per molecule: first orbital of every atom, local), ``aptr`` (atoms of every
    molecule), ``bp`` (bond_ptr), ``op`` / ``pp``."""
    assert all(sum(p) == m for p, m in zip(parts, ms))
    op = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    pp = np.concatenate([[0], np.cumsum(np.asarray(ms, dtype=np.int64) ** 2)])
    n = np.array([len(p) for p in parts], dtype=np.int64)
    aptr = np.concatenate([[0], np.cumsum(n)])
    flat = np.concatenate([[0], np.cumsum(np.concatenate(parts))]).astype(np.int64)
    plan = SimpleNamespace(B=len(ms), N=int(n.sum()), m_total=int(op[-1]), total=int(pp[-1]), mol_ptr=i32(aptr), orb_ptr=dev(flat))
    return SimpleNamespace(ms=list(ms), plan=plan, ptr=[np.concatenate([[0], np.cumsum(p)]) for p in parts], aptr=aptr,
                           bp=np.concatenate([[0], np.cumsum(n * n)]), op=op, pp=pp, N=int(n.sum()), Q=int((n * n).sum()))


def base_batch(seed=0):
    """The ragged base case in shuffled order, plus one molecule of a single atom and one of single-orbital atoms."""
    order = np.random.Generator(np.random.PCG64(100 + seed)).permutation(len(SIZES))
    ms = [SIZES[i] for i in order] + [14, 9]
    parts = [partition(m, i) for i, m in enumerate(ms[:-2])] + [[14], [1] * 9]
    return make_batch(ms, parts)


def state_of(bt):
    from nabladft_amd.orbitals import BatchedOrbitals
    return BatchedOrbitals(bt.op, DEV)


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def unguard(buf, name, written=True):
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), name
    inner = h[GUARD:-GUARD]
    assert not np.any(inner == SENTINEL) if written else np.all(inner == SENTINEL), name
    return inner.copy()


def call(name, st, *args):
    from nabladft_amd import _lib
    rc = getattr(_lib.load(), name)(_lib.ptr(st.buf), *st._dims, *args, _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()


def tables(orb, bt):
    N, Q, mol_ptr, atom_ptr, bond_ptr = orb._bond_tables(bt.plan)
    assert (N, Q) == (bt.N, bt.Q)
    return N, Q, mol_ptr, atom_ptr, bond_ptr


def raw_product(orb, D, S):
    from nabladft_amd import _lib
    buf, out = guarded(orb.state.P)
    call("nq_orb_bond_product", orb.state, _lib.ptr(D), _lib.ptr(S), int(S is not None and S.dtype == torch.float64), _lib.ptr(out))
    return unguard(buf, "P")


def raw_reduce(orb, bt, Pm, valence=True, atom_ptr=None):
    from nabladft_amd import _lib
    N, Q, mol_ptr, aptr, bond_ptr = tables(orb, bt)
    bb, bond = guarded(Q)
    bv, val = guarded(N)
    call("nq_orb_bond_reduce", orb.state, _lib.ptr(Pm), N, Q, _lib.ptr(mol_ptr), _lib.ptr(aptr if atom_ptr is None else atom_ptr), _lib.ptr(bond_ptr),
         _lib.ptr(bond), _lib.ptr(val) if valence else None)
    return unguard(bb, "bond"), unguard(bv, "valence", valence)


def raw_backward(orb, bt, gB, gV, Pm, D, S, want_d=True, want_s=True):
    """-> (E, gD or None, gS or None); an output that is not asked for is passed as NULL and its buffer must keep the sentinel."""
    from nabladft_amd import _lib
    N, Q, mol_ptr, aptr, bond_ptr = tables(orb, bt)
    P = orb.state.P
    be, E = guarded(P)
    bd, gD = guarded(P)
    bs, gS = guarded(P)
    call("nq_orb_bond_backward", orb.state, _lib.ptr(gB), _lib.ptr(gV), _lib.ptr(Pm), _lib.ptr(D) if want_s else None, _lib.ptr(S),
         int(S is not None and S.dtype == torch.float64), N, Q, _lib.ptr(mol_ptr), _lib.ptr(aptr), _lib.ptr(bond_ptr), _lib.ptr(E),
         _lib.ptr(gD) if want_d else None, _lib.ptr(gS) if want_s else None)
    d, s = unguard(bd, "gD", want_d), unguard(bs, "gS", want_s)
    return unguard(be, "E"), (d if want_d else None), (s if want_s else None)


def same_values(a, b):
    """Bit for bit, except that -0.0 and 0.0 are the same number."""
    return same_bits(np.asarray(a) + 0.0, np.asarray(b) + 0.0)


def worst_ratio(got, ref, bound):
    err = np.abs(got - ref)
    assert np.all(err[bound == 0.0] == 0.0)
    return float((err[bound > 0.0] / bound[bound > 0.0]).max()) if np.any(bound > 0.0) else 0.0


def symmetric(rng, m, integers=False):
    A = rng.integers(-3, 4, size=(m, m)).astype(np.float64) if integers else rng.normal(size=(m, m))
    return np.tril(A) + np.tril(A, -1).T


def general(rng, m, integers=False):
    return rng.integers(-3, 4, size=(m, m)).astype(np.float64) if integers else rng.normal(size=(m, m))


def ld(a):
    return np.asarray(a, dtype=np.longdouble)


def bond_blocks(flat, bt):
    n = np.diff(bt.aptr)
    return [flat[int(bt.bp[b]):int(bt.bp[b + 1])].reshape(int(n[b]), int(n[b])) for b in range(len(bt.ms))]


# ---- 1. the product ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_product_exact_placement_with_small_integers():
    """Small integers: every sum is exact, so tile offsets, the run-time operand orientation and the lower-triangle reads are compared with numpy bit for bit;
    the upper triangles of D and S hold garbage, which must not be read."""
    bt = base_batch()
    rng = np.random.Generator(np.random.PCG64(1))
    Ds, Ss = [symmetric(rng, m, True) for m in bt.ms], [symmetric(rng, m, True) for m in bt.ms]
    orb = state_of(bt)
    Dd = dev(pack(Ds, poison=1e30))
    for sdt in (np.float64, np.float32, None):
        Sd = None if sdt is None else dev(pack(Ss, sdt, poison=1e30))
        got = blocks(raw_product(orb, Dd, Sd), bt.ms)
        for b, m in enumerate(bt.ms):
            assert same_values(got[b], BR.product(Ds[b], None if sdt is None else Ss[b])), (sdt, b, m)


def test_product_bound_on_random_data():
    bt = base_batch()
    rng = np.random.Generator(np.random.PCG64(2))
    Ds, Ss = [symmetric(rng, m) for m in bt.ms], [symmetric(rng, m) for m in bt.ms]
    orb = state_of(bt)
    worst = {}
    for sdt in (np.float64, np.float32):
        S_ = [s.astype(sdt).astype(np.float64) for s in Ss]
        got = blocks(raw_product(orb, dev(pack(Ds, poison=float("nan"))), dev(pack(S_, sdt, poison=float("nan")))), bt.ms)
        w = 0.0
        for b, m in enumerate(bt.ms):
            f = worst_ratio(got[b], (ld(Ds[b]) @ ld(S_[b])).astype(np.float64), BR.product_bound(Ds[b], S_[b]))
            w = max(w, f)
            assert f <= 1.0, (sdt, b, m, f)
        worst[np.dtype(sdt).name] = w
    print("orbital_bond_parity kernels product worst error / bound: float64 S %.3f float32 S %.3f" % (worst["float64"], worst["float32"]))


# ---- 2. the reduction ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_reduce(bt, Ps, bond, val, exact):
    worst = np.zeros(2)
    Bs = bond_blocks(bond, bt)
    for b, m in enumerate(bt.ms):
        ptr = bt.ptr[b]
        got, v = Bs[b], val[int(bt.aptr[b]):int(bt.aptr[b + 1])]
        assert np.array_equal(got, got.T), (b, m)
        if exact:
            ref = BR.bond_orders(Ps[b], ptr)
            assert same_values(got, ref) and same_values(v, BR.valence(ref)), (b, m)
            continue
        Pl = ld(Ps[b])                                            # the same sums in extended precision
        ref = np.array([[float((Pl[ptr[A]:ptr[A + 1], ptr[C]:ptr[C + 1]] * Pl[ptr[C]:ptr[C + 1], ptr[A]:ptr[A + 1]].T).sum()) for C in range(len(ptr) - 1)]
                        for A in range(len(ptr) - 1)])
        f1 = worst_ratio(got, ref, BR.bond_bound(Ps[b], ptr))
        rows = (got - np.diag(np.diag(got))).astype(np.longdouble).sum(1).astype(np.float64)       # the device's own table, summed without the diagonal
        n = len(ptr) - 1
        f2 = worst_ratio(v, rows, (n + 4) * U * (np.abs(got) * (1.0 - np.eye(n))).sum(1))
        worst = np.maximum(worst, [f1, f2])
        assert f1 <= 1.0 and f2 <= 1.0, (b, m, f1, f2)
    return worst


def test_reduce_exact_and_within_the_bound():
    bt = base_batch(1)
    rng = np.random.Generator(np.random.PCG64(3))
    orb = state_of(bt)
    Pi = [general(rng, m, True) for m in bt.ms]
    bond, val = raw_reduce(orb, bt, dev(pack(Pi)))
    check_reduce(bt, Pi, bond, val, True)
    Pr = [general(rng, m) for m in bt.ms]
    bond, val = raw_reduce(orb, bt, dev(pack(Pr)))
    worst = check_reduce(bt, Pr, bond, val, False)
    bond2, _ = raw_reduce(orb, bt, dev(pack(Pr)), valence=False)        # the valences skipped: their buffer keeps the sentinel, the table is the same
    assert same_bits(bond, bond2)
    print("orbital_bond_parity kernels reduce worst error / bound: bond %.3f valence %.3f" % tuple(worst))


def test_reduce_nan_rule_for_a_bad_atom_range():
    """An atom that runs into the next molecule, and one of 33 orbitals: NaN in their rows and columns, every other entry as without them."""
    ms, parts = [40, 38, 20], [[5, 14, 1, 20], [33, 5], [14, 5, 1]]
    bt = make_batch(ms, parts)
    rng = np.random.Generator(np.random.PCG64(4))
    Ps = [general(rng, m) for m in ms]
    orb = state_of(bt)
    good, vgood = raw_reduce(orb, bt, dev(pack(Ps)))
    Bg = bond_blocks(good, bt)
    assert np.isnan(Bg[1][0, :]).all() and np.isnan(Bg[1][:, 0]).all() and np.isfinite(Bg[1][1, 1])       # the atom of 33 orbitals
    assert np.isfinite(Bg[0]).all() and np.isfinite(Bg[2]).all()
    assert np.isnan(vgood[4:6]).all() and np.isfinite(vgood[:4]).all() and np.isfinite(vgood[6:]).all()
    flat = np.concatenate([[0], np.cumsum(np.concatenate(parts))]).astype(np.int64)
    bad = flat.copy()
    bad[4] = 41                                                   # atom 3 of molecule 0 now ends one orbital inside molecule 1, whose first atom keeps 32
    got, vgot = raw_reduce(orb, bt, dev(pack(Ps)), atom_ptr=dev(bad))
    Bb = bond_blocks(got, bt)
    assert np.isnan(Bb[0][3, :]).all() and np.isnan(Bb[0][:, 3]).all() and same_bits(Bb[0][:3, :3], Bg[0][:3, :3])
    ref1 = BR.bond_orders(Ps[1], np.array([1, 33, 38]))          # molecule 1 under the shifted table: orbitals [1, 33) and [33, 38)
    assert np.all(np.abs(Bb[1] - ref1) <= BR.bond_bound(Ps[1], np.array([1, 33, 38])) * 2) and same_bits(Bb[1][1:, 1:], Bg[1][1:, 1:])
    assert same_bits(Bb[2], Bg[2]) and same_bits(vgot[6:], vgood[6:]) and np.isnan(vgot[:4]).all() and np.isfinite(vgot[4:6]).all()


# ---- 3. the reverse -----------------------------------------------------------------------------------------------------------------------------------------------------
def backward_inputs(bt, rng, integers):
    n = np.diff(bt.aptr)
    gB = [general(rng, int(k), integers) for k in n]                 # NOT symmetric
    gV = [(rng.integers(-3, 4, size=int(k)).astype(np.float64) if integers else rng.normal(size=int(k))) for k in n]
    Ps = [general(rng, m, integers) for m in bt.ms]
    Ds, Ss = [symmetric(rng, m, integers) for m in bt.ms], [symmetric(rng, m, integers) for m in bt.ms]
    return gB, gV, Ps, Ds, Ss


def check_backward(bt, E, gD, gS, gB, gV, Ps, Ds, Ss, exact):
    worst = np.zeros(3)
    Eb, gDb = blocks(E, bt.ms), blocks(gD, bt.ms)
    gSb = None if gS is None else blocks(gS, bt.ms)
    for b, m in enumerate(bt.ms):
        refE, refD, refS = BR.backward(Ds[b], None if Ss is None else Ss[b], bt.ptr[b], None if gB is None else gB[b], None if gV is None else gV[b], Ps[b])
        assert np.array_equal(gDb[b], gDb[b].T) and (gSb is None or np.array_equal(gSb[b], gSb[b].T)), (b, m)
        if exact:
            assert same_values(Eb[b], refE) and same_values(gDb[b], refD) and (gSb is None or same_values(gSb[b], refS)), (b, m)
            continue
        f0 = worst_ratio(Eb[b], refE, 4 * U * BR.upstream(np.abs(Ps[b]), bt.ptr[b], None if gB is None else np.abs(gB[b]), None if gV is None else np.abs(gV[b])))
        Ed = Eb[b]                                                # the gradients on the device's own E
        if Ss is None:
            f1 = worst_ratio(gDb[b], 0.5 * (Ed + Ed.T), 2 * U * np.abs(0.5 * (Ed + Ed.T)))
            f2 = 0.0
        else:
            Sl, Dl = BR.lower_sym(Ss[b]), BR.lower_sym(Ds[b])
            f1 = worst_ratio(gDb[b], (0.5 * (ld(Ed) @ ld(Sl) + ld(Sl) @ ld(Ed).T)).astype(np.float64), BR.backward_bound(Ed, Sl, False))
            f2 = 0.0 if gSb is None else worst_ratio(gSb[b], (0.5 * (ld(Dl) @ ld(Ed) + ld(Ed).T @ ld(Dl))).astype(np.float64), BR.backward_bound(Ed, Dl, True))
        worst = np.maximum(worst, [f0, f1, f2])
        assert f0 <= 1.0 and f1 <= 1.0 and f2 <= 1.0, (b, m, f0, f1, f2)
    return worst


def test_backward_exact_placement_with_small_integers():
    bt = base_batch(2)
    rng = np.random.Generator(np.random.PCG64(5))
    gB, gV, Ps, Ds, Ss = backward_inputs(bt, rng, True)
    orb = state_of(bt)
    args = (dev(np.concatenate([g.reshape(-1) for g in gB])), dev(np.concatenate(gV)), dev(pack(Ps)), dev(pack(Ds, poison=1e30)))
    for sdt in (np.float64, np.float32):
        E, gD, gS = raw_backward(orb, bt, *args, dev(pack(Ss, sdt, poison=1e30)))
        check_backward(bt, E, gD, gS, gB, gV, Ps, Ds, Ss, True)
    E, gD, none = raw_backward(orb, bt, args[0], None, args[2], args[3], None, want_s=False)       # no overlap: sym(E); no valence gradient
    check_backward(bt, E, gD, None, gB, None, Ps, Ds, None, True)
    E, gD, none = raw_backward(orb, bt, None, args[1], args[2], args[3], dev(pack(Ss)), want_s=False)   # the valences alone, gS skipped (its buffer keeps the sentinel)
    check_backward(bt, E, gD, None, None, gV, Ps, Ds, Ss, True)
    E, none, gS = raw_backward(orb, bt, args[0], args[1], args[2], args[3], dev(pack(Ss)), want_d=False)  # gS alone
    assert none is None
    for b, m in enumerate(bt.ms):
        assert same_values(blocks(gS, bt.ms)[b], BR.backward(Ds[b], Ss[b], bt.ptr[b], gB[b], gV[b], Ps[b])[2]), (b, m)


def test_backward_bound_on_random_data():
    bt = base_batch(3)
    rng = np.random.Generator(np.random.PCG64(6))
    gB, gV, Ps, Ds, Ss = backward_inputs(bt, rng, False)
    orb = state_of(bt)
    E, gD, gS = raw_backward(orb, bt, dev(np.concatenate([g.reshape(-1) for g in gB])), dev(np.concatenate(gV)), dev(pack(Ps)), dev(pack(Ds, poison=float("nan"))),
                             dev(pack(Ss, poison=float("nan"))))
    worst = check_backward(bt, E, gD, gS, gB, gV, Ps, Ds, Ss, False)
    print("orbital_bond_parity kernels reverse worst error / bound: E %.3f gD %.3f gS %.3f" % tuple(worst))


def test_product_and_backward_at_the_largest_size():
    """m = 1024, atoms of 32 orbitals: one product and one reverse launch.  The reference is plain float64 numpy, whose own rounding shares the bound."""
    m = 1024
    bt = make_batch([m], [[32] * 32])
    rng = np.random.Generator(np.random.PCG64(7))
    D, S = symmetric(rng, m) / m, symmetric(rng, m)
    orb = state_of(bt)
    Pm = raw_product(orb, dev(pack([D])), dev(pack([S]))).reshape(m, m)
    f0 = worst_ratio(Pm, D @ S, BR.product_bound(D, S))
    gB, gV = general(rng, 32), rng.normal(size=32)
    E, gD, gS = raw_backward(orb, bt, dev(gB.reshape(-1)), dev(gV), dev(Pm.reshape(-1)), dev(pack([D])), dev(pack([S])))
    E, gD, gS = E.reshape(m, m), gD.reshape(m, m), gS.reshape(m, m)
    assert np.array_equal(gD, gD.T) and np.array_equal(gS, gS.T)
    fE = worst_ratio(E, BR.upstream(Pm, bt.ptr[0], gB, gV), 4 * U * BR.upstream(np.abs(Pm), bt.ptr[0], np.abs(gB), np.abs(gV)))
    f1 = worst_ratio(gD, 0.5 * (E @ S + S @ E.T), BR.backward_bound(E, S, False))
    f2 = worst_ratio(gS, 0.5 * (D @ E + E.T @ D), BR.backward_bound(E, D, True))
    print(f"orbital_bond_parity kernels m=1024 worst error / bound: product {f0:.3f} E {fE:.3f} gD {f1:.3f} gS {f2:.3f}")
    assert f0 <= 1.0 and fE <= 1.0 and f1 <= 1.0 and f2 <= 1.0


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------------------------------------
def indicator(ptr, m):
    A = np.zeros((len(ptr) - 1, m))
    for a in range(len(ptr) - 1):
        A[a, ptr[a]:ptr[a + 1]] = 1.0
    return A


def bond_loss(ptr, m, W, w):
    """L = sum W o B + sum w V + 1/2 |B|^2 as a function of torch (eps, D, S, H): the dense definitions, for autograd."""
    At, Wt, wt = torch.from_numpy(indicator(ptr, m)), torch.from_numpy(W), torch.from_numpy(w)

    def loss(eps, D, S, H):
        P = D if S is None else D @ S
        B = At @ (P * P.mT) @ At.mT
        V = B.sum(1) - torch.diagonal(B)
        return (Wt * B).sum() + (wt * V).sum() + 0.5 * (B * B).sum()
    return loss


# The cases of ``orbital_density_ref.CASES`` that have a virtual orbital: m = 2, 3, 17, 65, 130 at kappa0 = 1e2 and m = 130 at 1e4, n_occ about m / 3.  With every
# orbital occupied D = 2 S^-1 and P = 2 I whatever H and S are: the table is constant, every gradient vanishes and there is nothing to compare but rounding
# noise (the sum rules below cover those densities).
CASES = [c for c in DR.CASES if c[1] < c[0]]


def unpermute(X2, index):
    """The copy's result back in the caller's order: entry ``index`` of the result is what the copy holds."""
    Z = np.empty_like(X2)
    Z[index] = X2
    return Z


@functools.lru_cache(maxsize=None)
def reference(inputs):
    """Per case of ``CASES``: the yardstick's bond table, valences and gradients, its spread under a permutation of the atoms and of the
    orbitals inside them, and the quantities the propagated bounds need."""
    out = []
    for ci, case in enumerate(CASES):
        m, n_occ = case[0], case[1]
        H, S = DR.gapped_case(*case)
        if inputs == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        sizes = partition(m, ci) if m > 32 else [1] * m if m <= 3 else partition(m, 2)       # m = 17: atoms of 5 and 12 orbitals
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        n = len(sizes)
        rng = np.random.Generator(np.random.PCG64(8000 + ci))
        W, w = rng.normal(size=(n, n)), rng.normal(size=n)
        eps, D, gH, gS = DR.autograd(H, S, n_occ, bond_loss(ptr, m, W, w))
        P, B, V = BR.forward(D, S, ptr)
        aperm = rng.permutation(n)                                # position k of the copy holds atom aperm[k], its orbitals shuffled
        perm = np.concatenate([ptr[a] + rng.permutation(sizes[a]) for a in aperm]).astype(np.int64)
        ptr2 = np.concatenate([[0], np.cumsum([sizes[a] for a in aperm])])
        ix, ax = np.ix_(perm, perm), np.ix_(aperm, aperm)
        _, D2, gH2, gS2 = DR.autograd(H[ix], S[ix], n_occ, bond_loss(ptr2, m, W[ax], w[aperm]))
        _, B2, V2 = BR.forward(D2, S[ix], ptr2)
        Bb, gHb, gSb, Vb = unpermute(B2, ax), unpermute(gH2, ix), unpermute(gS2, ix), unpermute(V2, aperm)
        spread = dict(bond=float(np.abs(B - Bb).max()), valence=float(np.abs(V - Vb).max()), gH=float(np.abs(gH - gHb).max()), gS=float(np.abs(gS - gSb).max()))
        uD = PR.density_unit(H, S, n_occ, eps, D)
        dP = BR.product_bound(D, S) + BOUND * uD * np.abs(S).sum(0)[None, :]
        Ai = indicator(ptr, m)
        pB = BR.bond_bound(P, ptr) + Ai @ (dP * np.abs(P).T + np.abs(P) * dP.T) @ Ai.T
        pV = (pB * (1.0 - np.eye(n))).sum(1) + (n + 4) * U * (np.abs(B) * (1.0 - np.eye(n))).sum(1)
        uH, uS = DR.units(H, S, n_occ, eps, gH, gS)
        direct = BR.backward(D, S, ptr, W + B, w, P)[2]            # the part of dL/dS that bond_orders itself hands back; the rest comes through D
        out.append(SimpleNamespace(case=case, H=H, S=S, ptr=ptr, sizes=sizes, W=W, w=w, eps=eps, D=D, B=B, V=V, gH=gH, gS=gS, spread=spread,
                                   f32_terms=dict(gH=np.abs(gH), gS=np.abs(direct) + np.abs(gS - direct) + np.abs(gS)),
                                   prop=dict(bond=pB, valence=pV, gH=BOUND * uH, gS=BOUND * uS)))
    return out


@pytest.mark.parametrize("inputs", ["float64", "float32"])
def test_bond_orders_end_to_end(inputs):
    import nabladft_amd as nq
    refs = reference(inputs)
    bt = make_batch([r.case[0] for r in refs], [r.sizes for r in refs])
    nos = [r.case[1] for r in refs]
    tdt = getattr(torch, inputs)
    H, S = dev(pack([r.H for r in refs]), tdt).requires_grad_(True), dev(pack([r.S for r in refs]), tdt).requires_grad_(True)
    eps, D, sol = nq.orbital_solution(H, S, bt.op, nos, return_solution=True)
    bond, val = nq.bond_orders(D, bt.plan, S, sol)
    assert bond.dtype == torch.float64 and val.dtype == torch.float64 and bond.requires_grad and val.requires_grad and bond.numel() == bt.Q and val.numel() == bt.N
    total = 0.0
    for b, r in enumerate(refs):
        Bd = nq.dense_bond_orders(bond, bt.aptr, b)
        Vd = val[int(bt.aptr[b]):int(bt.aptr[b + 1])]
        total = total + (dev(r.W) * Bd).sum() + (dev(r.w) * Vd).sum() + 0.5 * (Bd * Bd).sum()
    total.backward()
    sol.check()
    assert H.grad.dtype == tdt and S.grad.dtype == tdt and H.grad.shape == H.shape and S.grad.shape == S.shape
    out_round = 2.0 ** -24 if inputs == "float32" else 0.0
    Bs, Vs = bond_blocks(bond.detach().cpu().numpy(), bt), val.detach().cpu().numpy()
    gHs, gSs = blocks(H.grad.double().cpu().numpy(), bt.ms), blocks(S.grad.double().cpu().numpy(), bt.ms)
    tiny = np.finfo(np.float64).tiny
    for b, r in enumerate(refs):
        m, n_occ = r.case[0], r.case[1]
        got = dict(bond=Bs[b], valence=Vs[int(bt.aptr[b]):int(bt.aptr[b + 1])], gH=gHs[b], gS=gSs[b])
        ref = dict(bond=r.B, valence=r.V, gH=r.gH, gS=r.gS)
        assert np.array_equal(got["bond"], got["bond"].T) and np.array_equal(got["gH"], got["gH"].T) and np.array_equal(got["gS"], got["gS"].T)
        line = []
        for k in ("bond", "valence", "gH", "gS"):
            rounding = out_round * r.f32_terms[k] if k in ("gH", "gS") else 0.0
            err = np.maximum(np.abs(got[k] - ref[k]) - rounding, 0.0)
            allow = np.maximum(10.0 * r.spread[k], r.prop[k])
            fig = float((err / np.maximum(allow, tiny)).max())
            line.append(f"{k} {fig:.3g} of the allowance ({float(err.max()) / max(r.spread[k], tiny):.3g} spreads; allowance {float(np.max(allow)) / max(r.spread[k], tiny):.3g} spreads)")
            assert fig <= 1.0, (inputs, r.case, k, fig)
        print(f"orbital_bond_parity end-to-end {inputs} m={m} n_occ={n_occ} kappa0={r.case[3]:g} atoms={len(r.sizes)}: " + "; ".join(line))


# ---- 5. the sum rules ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_sum_rule(tag, bt, b, Dm, Sm, bond_b, pop_b, nelec_b, rel_idem):
    """sum_B B_AB against 2 pop_A, and sum_AB B_AB against 2 Tr(DS), for one molecule; ``rel_idem``: the relative departure from (DS)^2 = 2 DS the route is
    allowed.  The allowance adds the dot-product bounds of the row sums (n_A m products), of the populations (m products and n_A additions, doubled) and of P
    itself carried through the products, to 2 rel_idem sum |P_mu,nu P_nu,mu|."""
    m, ptr = bt.ms[b], bt.ptr[b]
    P, Pa = Dm @ Sm, np.abs(Dm @ Sm)
    Ai = indicator(ptr, m)
    dP = BR.product_bound(Dm, Sm)
    mag = Ai @ (Pa * Pa.T).sum(1)
    sizes = np.diff(ptr)
    allow = ((sizes * m + 4) * U * mag + 2.0 * (m + sizes + 4) * U * (Ai @ (np.abs(Dm) * np.abs(Sm)).sum(1)) + Ai @ (dP * Pa.T + Pa * dP.T).sum(1)
             + 2.0 * rel_idem * mag)
    err = np.abs(bond_b.sum(1) - 2.0 * pop_b)
    fig = float((err / allow).max())
    total = abs(bond_b.sum() - 2.0 * nelec_b) / (allow.sum() + (len(sizes) ** 2 + m + 4) * U * (np.abs(bond_b).sum() + 2.0 * (np.abs(Dm) * np.abs(Sm)).sum()))
    print(f"orbital_bond_parity sum rule {tag} molecule {b} m={m}: worst |sum_B B_AB - 2 pop_A| / allowance {fig:.3g}, / (2 pop_A) "
          f"{float((err / np.abs(2.0 * pop_b)).max()):.3g}; |sum_AB B_AB - 2 Tr(DS)| / allowance {total:.3g}")
    assert fig <= 1.0 and total <= 1.0, (tag, b, fig, total)


def test_sum_rules_on_the_solver_and_the_purified_density():
    import nabladft_amd as nq
    refs = [r for r in reference("float64")]
    bt = make_batch([r.case[0] for r in refs], [r.sizes for r in refs])
    nos = [r.case[1] for r in refs]
    H, S = dev(pack([r.H for r in refs])), dev(pack([r.S for r in refs]))
    eps, D, sol = nq.orbital_solution(H, S, bt.op, nos, return_solution=True)
    Dp, pur = nq.purified_density_matrix(H, S, bt.op, nos, return_solution=True)
    sol.check()
    pur.check()
    for tag, dens, owner in (("solver", D, sol), ("purified", Dp, pur)):
        bond, val = nq.bond_orders(dens, bt.plan, S, owner)
        pop, nelec, _ = owner.populations(dens, bt.plan, S)
        Bs, pops, Dbs = bond_blocks(bond.cpu().numpy(), bt), pop.cpu().numpy(), blocks(dens.cpu().numpy(), bt.ms)
        nel = nelec.cpu().numpy()
        for b, r in enumerate(refs):
            m, n_occ = r.case[0], r.case[1]
            kap = float(np.linalg.cond(r.S))
            rel = BOUND * m * R.EPS * kap if tag == "solver" else BOUND * PR.density_unit(r.H, r.S, n_occ, r.eps, r.D) / np.abs(r.D).max()
            check_sum_rule(tag, bt, b, Dbs[b], r.S, Bs[b], pops[int(bt.aptr[b]):int(bt.aptr[b + 1])], nel[b], rel)


def test_sum_rules_on_the_database_molecules():
    import nabladft_amd as nq
    probs = db_problems()
    Hs, Ss = [p[0] for p in probs], [p[1] for p in probs]
    ms = [h.shape[0] for h in Hs]
    plan, per_atom = db_plan(probs)
    natoms = [len(p[2]) for p in probs]
    aptr = np.concatenate([[0], np.cumsum(natoms)])
    parts = [per_atom[int(a):int(e)] for a, e in zip(aptr[:-1], aptr[1:])]
    bt = make_batch(ms, parts)
    bt.plan = plan
    z = np.concatenate([np.asarray(p[2], dtype=np.int64) for p in probs])
    n_occ = nq.occupied_counts(z, aptr, 0, bt.op)
    Hd, Sd = dev(pack(Hs)), dev(pack(Ss, poison=1e30))
    orb = nq.BatchedOrbitals(bt.op, DEV).solve(Hd, Sd)
    assert orb.status.tolist() == [0, 0, 0, 0, 0, 1]               # the last molecule's overlap is indefinite
    D = orb.density(n_occ)
    bond, val, Pm = orb.bond_orders(D, plan, Sd)
    pop, nelec, _ = orb.populations(D, plan, Sd)
    Bs, pops, Dbs = bond_blocks(bond.cpu().numpy(), bt), pop.cpu().numpy(), blocks(D.cpu().numpy(), ms)
    vals = val.cpu().numpy()
    for b, m in enumerate(ms):
        atoms = slice(int(aptr[b]), int(aptr[b + 1]))
        if b == 5:
            assert np.isnan(Bs[b]).all() and np.isnan(vals[atoms]).all() and np.isnan(blocks(Pm.cpu().numpy(), ms)[b]).all()
            continue
        check_sum_rule("database", bt, b, Dbs[b], Ss[b], Bs[b], pops[atoms], float(nelec[b]), BOUND * m * R.EPS * float(np.linalg.cond(Ss[b])))
        assert np.array_equal(Bs[b], Bs[b].T) and np.isfinite(vals[atoms]).all()
        heavy = [i for i, zz in enumerate(probs[b][2]) if int(zz) > 1]
        print(f"orbital_bond_parity database molecule {b} m={m} atoms {natoms[b]}: largest off-diagonal bond order {float((Bs[b] - np.diag(np.diag(Bs[b]))).max()):.3f}, "
              f"valences of the heavy atoms {np.round(vals[atoms][heavy], 2).tolist()}")
    # the loss of a table against itself is zero, and its value is the mean over a molecule's entries, then over the molecules
    good = bond[:int(bt.bp[5])]
    assert float(nq.BondOrderLoss("mae")(good, good.clone(), aptr[:6])) == 0.0 and float(nq.BondOrderLoss("mse")(good, good.clone(), aptr[:6])) == 0.0
    other = good + 0.25
    assert abs(float(nq.BondOrderLoss("mae")(other, good, aptr[:6])) - 0.25) <= 1e-12 and abs(float(nq.BondOrderLoss("mse")(other, good, aptr[:6])) - 0.0625) <= 1e-12
    with pytest.raises(ValueError, match="entries"):
        nq.BondOrderLoss()(good[:-1], good[:-1], aptr[:6])


# ---- 6. run to run, the rest of the batch, a failed molecule --------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_batch_independent_and_a_failed_molecule():
    refs = reference("float64")
    pick = [2, 3, 4, 5]                                            # m = 17, 65, 130, 130 (kappa0 = 1e4)
    Hs, Ss, nos, parts = [refs[i].H for i in pick], [refs[i].S.copy() for i in pick], [refs[i].case[1] for i in pick], [refs[i].sizes for i in pick]
    ms = [h.shape[0] for h in Hs]
    rng = np.random.Generator(np.random.PCG64(9))
    w, V = np.linalg.eigh(Ss[2])
    w[3] = -0.25
    Sbad = (V * w[None, :]) @ V.T
    Sbad = 0.5 * (Sbad + Sbad.T)                                   # not positive definite: the solve fails on this molecule
    gBs = [general(rng, len(p)) for p in parts]
    gVs = [rng.normal(size=len(p)) for p in parts]

    def run(idx, bad=None):
        from nabladft_amd.orbitals import BatchedOrbitals
        bt = make_batch([ms[i] for i in idx], [parts[i] for i in idx])
        S_ = [Sbad if i == bad else Ss[i] for i in idx]
        Sd = dev(pack(S_))
        orb = BatchedOrbitals(bt.op, DEV).solve(dev(pack([Hs[i] for i in idx])), Sd)
        D = orb.density([nos[i] for i in idx])
        bond, val, Pm = orb.bond_orders(D, bt.plan, Sd)
        gD, gS = orb.bond_orders_backward(bt.plan, dev(np.concatenate([gBs[i].reshape(-1) for i in idx])), dev(np.concatenate([gVs[i] for i in idx])), Pm, D, Sd,
                                          want_s=True)
        return bt, orb.status.cpu().numpy(), [t.cpu().numpy() for t in (Pm, gD, gS)], bond.cpu().numpy(), val.cpu().numpy()
    every = list(range(len(ms)))
    bt, status, packed, bond, val = run(every)
    bt2, status2, packed2, bond2, val2 = run(every)
    assert not status.any() and all(same_bits(x, y) for x, y in zip(packed + [bond, val], packed2 + [bond2, val2]))
    for b in (0, 1, 3):                                            # alone: the same bits as inside the batch
        bta, _, pa, ba, va = run([b])
        for x, y in zip(pa, packed):
            assert same_bits(x.reshape(ms[b], ms[b]), blocks(y, ms)[b]), (b, ms[b])
        assert same_bits(ba, bond[int(bt.bp[b]):int(bt.bp[b + 1])]) and same_bits(va, val[int(bt.aptr[b]):int(bt.aptr[b + 1])])
    btf, statusf, packedf, bondf, valf = run(every, bad=2)
    assert statusf.tolist() == [0, 0, 1, 0]
    for b in every:
        own = [blocks(y, ms)[b] for y in packedf] + [bondf[int(bt.bp[b]):int(bt.bp[b + 1])], valf[int(bt.aptr[b]):int(bt.aptr[b + 1])]]
        was = [blocks(y, ms)[b] for y in packed] + [bond[int(bt.bp[b]):int(bt.bp[b + 1])], val[int(bt.aptr[b]):int(bt.aptr[b + 1])]]
        if b == 2:
            assert all(np.isnan(x).all() for x in own)
        else:
            assert all(same_bits(x, y) for x, y in zip(own, was)), b


def test_dimension_mismatch_touches_nothing_and_python_refusals():
    from nabladft_amd import _lib
    bt = make_batch([5, 3], [[2, 3], [3]])
    orb = state_of(bt)
    st = orb.state
    lib = _lib.load()
    N, Q, mol_ptr, aptr, bond_ptr = tables(orb, bt)
    big, big2 = (torch.full((40,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2))
    src = torch.ones(40, dtype=torch.float64, device=DEV)
    for fn, args in ((lib.nq_orb_bond_product, (_lib.ptr(src), None, 0, _lib.ptr(big))),
                     (lib.nq_orb_bond_reduce, (_lib.ptr(src), N, Q, _lib.ptr(mol_ptr), _lib.ptr(aptr), _lib.ptr(bond_ptr), _lib.ptr(big), _lib.ptr(big2))),
                     (lib.nq_orb_bond_backward, (None, _lib.ptr(src), _lib.ptr(src), None, None, 0, N, Q, _lib.ptr(mol_ptr), _lib.ptr(aptr), _lib.ptr(bond_ptr),
                                                 _lib.ptr(big), _lib.ptr(big2), None))):
        assert fn(_lib.ptr(st.buf), 2, 8, 36, *args, _lib.stream_ptr()) == 0, lib.nq_last_error()       # (2, 8, 36) instead of (2, 8, 34)
        torch.cuda.synchronize()
        assert int(st.header_dev[4]) == -2 and bool((big == SENTINEL).all()) and bool((big2 == SENTINEL).all())
        with pytest.raises(RuntimeError, match="other dimensions"):
            st.header()
        st.header_dev[4] = 0
    D = dev(pack([np.eye(5), np.eye(3)]))
    bond, val, Pm = orb.bond_orders(D, bt.plan)
    assert int(st.header_dev[4]) == 0 and bond.cpu().tolist() == [2.0, 0.0, 0.0, 3.0, 3.0] and val.cpu().tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="needs S_packed and D"):
        orb.bond_orders_backward(bt.plan, bond, None, Pm, D, None, want_s=True)
    with pytest.raises(ValueError, match="float64"):
        orb.bond_orders(D.float(), bt.plan)
    with pytest.raises(ValueError, match="another batch"):
        state_of(make_batch([5, 4], [[2, 3], [4]])).bond_reduce(torch.zeros(41, dtype=torch.float64, device=DEV), bt.plan)


# ---- 7. the QHNet task ------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_bond_order_task(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from nabladft_amd.orbitals import OrbitalState
    from test_qhnet_gpu import ORBITALS, load_case
    g, cfg, net, batch = load_case("small", torch.device(DEV))
    per_atom = np.array([sum(2 * l + 1 for l in ORBITALS[int(a)]) for a in g["z"]])
    ends = np.cumsum(g["sizes"])
    batch.hamiltonian, batch.overlap, o = [], [], 0
    rng = np.random.Generator(np.random.PCG64(6))
    for m in [int(per_atom[e - n:e].sum()) for n, e in zip(g["sizes"], ends)]:
        batch.hamiltonian.append(g["target"][o:o + m, o:o + m].astype(np.float32))
        A = rng.normal(size=(m, m)) * 0.1 / np.sqrt(m)
        batch.overlap.append((np.eye(m) + A + A.T).astype(np.float32))       # a well conditioned overlap
        o += m
    charge = [0, -1, 1]                                           # the fixture's molecules hold 92, 9 and 31 electrons: closed shells as anion and cation
    base = {"hamiltonian": HamiltonianLoss(), "orbital_energies": nq.OrbitalEnergyLoss("mae", "occupied", charge),
            "density_matrix": nq.DensityMatrixLoss("mse", charge), "mulliken_charges": nq.MullikenChargeLoss("mse", charge)}
    base_c = {"hamiltonian": 1.0, "orbital_energies": 0.25, "density_matrix": 0.5, "mulliken_charges": 2.0}
    losses, coefs = dict(base, bond_orders=nq.BondOrderLoss("mse", charge)), dict(base_c, bond_orders=0.75)
    make = lambda cls, ls, cs: cls("QHNet", net, None, None, ls, None, None, cs)
    solves = []
    real = OrbitalState.solve
    monkeypatch.setattr(OrbitalState, "solve", lambda self, *a, **k: (solves.append(1), real(self, *a, **k))[1])
    params = [p for p in net.parameters() if p.requires_grad]

    def step(task):
        for p in params:
            p.grad = None
        loss = task.training_step(batch, 0)
        loss.backward()
        return loss.detach(), [None if p.grad is None else p.grad.detach().clone() for p in params]
    task = make(nq.QHNetBondOrderLightning, losses, coefs)
    loss, grads = step(task)
    assert len(solves) == 2, len(solves)                           # one solve of the prediction, one of the target, for four orbital terms
    assert bool(torch.isfinite(loss)) and all(gr is None or bool(torch.isfinite(gr).all()) for gr in grads) and any(gr is not None for gr in grads)
    # the bond term by hand on what the step hands to the loss; the target is detached and a prediction against itself costs nothing
    preds, targets, _ = task._evaluate(batch)
    assert len(solves) == 4
    bp, btg = preds["bond_orders"], targets["bond_orders"]
    n = np.asarray(g["sizes"], dtype=np.int64)
    assert bp.numel() == int((n * n).sum()) and bp.requires_grad and not btg.requires_grad and bool(torch.isfinite(bp).all()) and bool(torch.isfinite(btg).all())
    term = losses["bond_orders"](bp, btg, batch.ptr)
    by_hand = np.mean([((nq.dense_bond_orders(bp.detach().cpu().numpy(), batch.ptr, b) - nq.dense_bond_orders(btg.cpu().numpy(), batch.ptr, b)) ** 2).mean() for b in range(len(n))])
    assert float(term.detach()) > 0.0 and abs(float(term.detach()) - by_hand) <= 1e-12 * by_hand
    assert float(losses["bond_orders"](bp, bp.detach().clone(), batch.ptr)) == 0.0 and float(nq.BondOrderLoss("mae")(btg, btg.clone(), batch.ptr)) == 0.0
    # the same parameters get a gradient as without the term, and the term moves the loss by its coefficient times its value
    dens = make(nq.QHNetDensityLightning, base, base_c)
    before = len(solves)
    loss_d, grads_d = step(dens)
    assert len(solves) == before + 2
    assert [gr is None for gr in grads] == [gr is None for gr in grads_d]
    print("orbital_bond_parity qhnet task loss %.9g without the bond term %.9g bond term %.6g" % (float(loss), float(loss_d), float(term.detach())))
    assert torch.allclose((loss - loss_d).double(), 0.75 * term.detach().double(), rtol=1e-4, atol=1e-6 * float(loss.abs()))
    # the coefficient at 0: QHNetDensityLightning's step, bit for bit, with the same two solves
    zero = make(nq.QHNetBondOrderLightning, losses, dict(coefs, bond_orders=0.0))
    before = len(solves)
    loss_z, grads_z = step(zero)
    assert len(solves) == before + 2
    assert loss_z.dtype == loss_d.dtype and torch.equal(loss_z, loss_d)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads_z, grads_d))
    nokey = make(nq.QHNetBondOrderLightning, base, base_c)       # without the key: the same
    loss_n, grads_n = step(nokey)
    assert torch.equal(loss_n, loss_d) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads_n, grads_d))
    with pytest.raises(ValueError, match="different charges"):
        make(nq.QHNetBondOrderLightning, dict(losses, bond_orders=nq.BondOrderLoss("mse", 0)), coefs).training_step(batch, 0)
