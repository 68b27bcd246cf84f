"""GPU: the Löwdin kernels (csrc/orblowdin.hip) through the C ABI and through ``BatchedOrbitals`` / ``LowdinBasis`` / ``nabladft_amd.orbital_loss.lowdin_*`` /
``QHNetLowdinLightning``, against the numpy restatement and the torch yardstick of tests/orbital_lowdin_ref.py.

Bounds (U = 2^-53, E = 2^-52; ``orbital_lowdin_ref`` states them).  Product: |Y - ref| <= (m + 4) U (|M||X|) per entry; symprod: (2 m + 4) U of half the sum of
the two contractions' magnitudes (the halving and alpha = 1, 2 are exact); references in extended precision.  Small integers make every sum exact: compared
bit for bit (the sign of a zero aside).  ``nq_orb_low_mo``: the bound of W = U^T T times |K|, plus 3 (kind 0) or 5 (kind 1) half-ulp roundings of |K W|: K is
a sum and a division (2 roundings) or a product, a sum, a product and a division (4), and K W one more product; the reference uses the same a = sqrt(eps)
read back from the state.  Weights: ``np.sqrt`` and one division, exactly.  At m = 1024 the reference is plain float64 numpy, whose own rounding shares the bound.

End to end.  The yardstick is ``orbital_density_ref.autograd`` (torch.linalg Cholesky -> eigh -> D) followed by ``orbital_lowdin_ref.torch_lowdin`` (eigh of S ->
U f(s) U^T -> congruence -> populations / Wiberg table / H^L), autograd through all of it.  Its own spread is measured first on a copy with the atoms
reordered and the orbitals inside every atom shuffled, mapped back.  Allowance per quantity: max(10 x that spread, the propagated bound).  The propagated
bounds: |dD| <= 10 U_D (``orbital_purify_ref.density_unit``); |dA| <= 10 m E sqrt(kappa s_max) and |dA^-| <= 10 m E kappa / sqrt(s_min) per entry (an
eigendecomposition of S to m E |S| relative, carried through f(s) and U f U^T; tests/test_orbital_lowdin_cpu.py holds the restatement to the same forms); these
and the dot-product bounds carried through Y = M X and sym(X Y), then through the diagonal sums, the squares of the table and the row sums.  Of the gradients:
ten units of ``orbital_density_ref.units``, the bound the response chain they flow through is held to.  Float32 gradients are allowed their own rounding,
2^-24 per element of each of the two float32 terms autograd adds (the one through D and the direct one) and of their float32 sum.  The figures are printed as
``orbital_lowdin_parity ...`` lines (kept in profiles/orbital_lowdin_parity.txt).

Sum rules.  With |A A - S| <= 2 x 10 m E s_max per entry (the decomposition's residual and its orthogonality, each held to 10 m E by tests/test_orbitals_gpu.py):
sum_A q_A - Tr(D S) = Tr(D (A A - S)) plus the dot-product bounds; sum_B W_AB - 2 q_A sums [A (D S D - 2 D) A + A D (A A - S) D A]_mu,mu plus those bounds, the
first term being the relative departure from idempotency the route is allowed (10 m E kappa for the solver, 10 U_D / max|D| for the purified density) times
2 (|A||D||A|)_mu,mu; eigvalsh(H^L) = eps to 10 m E kappa of the spectral width for each of the two routes."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import orbital_bond_ref as BR
import orbital_density_ref as DR
import orbital_lowdin_ref as LR
import orbital_purify_ref as PR
import orbitals_ref as R
from test_orbital_bond_gpu import (SENTINEL, bond_blocks, call, general, guarded, indicator, ld, make_batch, partition, same_values, symmetric, unguard, unpermute,
                                   worst_ratio)
from test_orbital_loss_gpu import blocks, db_plan
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 17, 64, 65, 130]                                # one orbital .. across the 64- and 128-orbital tile edges
U = LR.U
E = 2.0 ** -52
TINY = np.finfo(np.float64).tiny


def base_batch(seed=0):
    order = np.random.Generator(np.random.PCG64(300 + seed)).permutation(len(SIZES))
    ms = [SIZES[i] for i in order]
    return make_batch(ms, [partition(m, i) for i, m in enumerate(ms)])


def state_of(bt):
    from nabladft_amd.orbitals import BatchedOrbitals
    return BatchedOrbitals(bt.op, DEV)


def overlaps(ms, kappa0=1e2, seed=0):
    return [DR.overlap(m, kappa0, np.random.Generator(np.random.PCG64(500 + seed + m))) for m in ms]


def raw_product(orb, Md, Xd):
    from nabladft_amd import _lib
    buf, out = guarded(orb.state.P)
    call("nq_orb_low_product", orb.state, _lib.ptr(Md), int(Md.dtype == torch.float64), _lib.ptr(Xd), _lib.ptr(out))
    return unguard(buf, "Y")


def raw_symprod(orb, Ed, Xd, side, alpha):
    from nabladft_amd import _lib
    buf, out = guarded(orb.state.P)
    call("nq_orb_low_symprod", orb.state, _lib.ptr(Ed), _lib.ptr(Xd), side, float(alpha), _lib.ptr(out))
    return unguard(buf, "symprod")


def raw_symmetrize(orb, Gd):
    from nabladft_amd import _lib
    buf, out = guarded(orb.state.P)
    call("nq_orb_low_symmetrize", orb.state, _lib.ptr(Gd), _lib.ptr(out))
    return unguard(buf, "Gs")


def raw_mo(orb, Td, kind):
    from nabladft_amd import _lib
    buf, out = guarded(orb.state.P)
    call("nq_orb_low_mo", orb.state, kind, _lib.ptr(Td), _lib.ptr(out))
    return unguard(buf, "A")


# ---- 1. the two products ------------------------------------------------------------------------------------------------------------------------------------------------
def test_products_exact_placement_with_small_integers():
    """Small integers: every sum is exact, so tile offsets, the run-time operand orientation, the lower-triangle reads and the mirrored stores are compared
    with numpy bit for bit; the upper triangles of the symmetric operands hold garbage, which must not be read."""
    bt = base_batch()
    rng = np.random.Generator(np.random.PCG64(1))
    Ms, Xs, Es = [symmetric(rng, m, True) for m in bt.ms], [symmetric(rng, m, True) for m in bt.ms], [general(rng, m, True) for m in bt.ms]
    orb = state_of(bt)
    Xd, Ed = dev(pack(Xs, poison=1e30)), dev(pack(Es))
    for mdt in (np.float64, np.float32):
        got = blocks(raw_product(orb, dev(pack(Ms, mdt, poison=1e30)), Xd), bt.ms)
        for b, m in enumerate(bt.ms):
            assert same_values(got[b], LR.product(Ms[b], Xs[b])), (mdt, b, m)
    for side in (0, 1):
        for alpha in (1.0, 2.0):
            got = blocks(raw_symprod(orb, Ed, Xd, side, alpha), bt.ms)
            for b, m in enumerate(bt.ms):
                assert np.array_equal(got[b], got[b].T) and same_values(got[b], LR.symprod(Es[b], Xs[b], side, alpha)), (side, alpha, b, m)


def test_symmetrize_exactly_and_a_nonsymmetric_upstream_gradient():
    """(G + G^T) / 2 is one sum and one exact halving per entry: compared with numpy bit for bit on random data, every entry written (the guard), exactly
    symmetric.  Then the reverse of the congruence on a NON-symmetric G against the restatement on its symmetric part, within the bounds of the products."""
    bt = base_batch(4)
    rng = np.random.Generator(np.random.PCG64(11))
    Gs, Xs, Ms = [general(rng, m) for m in bt.ms], [symmetric(rng, m) for m in bt.ms], [symmetric(rng, m) for m in bt.ms]
    orb = state_of(bt)
    Gd, Xd = dev(pack(Gs)), dev(pack(Xs))
    got = blocks(raw_symmetrize(orb, Gd), bt.ms)
    for b, m in enumerate(bt.ms):
        assert same_bits(got[b], 0.5 * (Gs[b] + Gs[b].T)) and np.array_equal(got[b], got[b].T), (b, m)
    ML, Y = orb.sym_congruence(Xd, dev(pack(Ms)))
    gM, gX = orb.sym_congruence_backward(Gd, Xd, Y, symmetric=False)
    gM2, gX2 = orb.sym_congruence_backward(orb.low_symmetrize(Gd), Xd, Y)
    assert same_bits(gM.cpu().numpy(), gM2.cpu().numpy()) and same_bits(gX.cpu().numpy(), gX2.cpu().numpy())
    gMb, gXb, Yb = blocks(gM.cpu().numpy(), bt.ms), blocks(gX.cpu().numpy(), bt.ms), blocks(Y.cpu().numpy(), bt.ms)
    for b, m in enumerate(bt.ms):
        Gsym = LR.sym(Gs[b])
        GX = Gsym @ Xs[b]
        rM, rX = LR.congruence_backward(Gsym, Xs[b], Yb[b])
        bM = LR.symprod_bound(GX, Xs[b], 0) + 0.5 * (np.abs(Xs[b]) @ LR.product_bound(Gsym, Xs[b]) + (np.abs(Xs[b]) @ LR.product_bound(Gsym, Xs[b])).T)
        assert np.all(np.abs(gMb[b] - rM) <= 2.0 * bM) and np.all(np.abs(gXb[b] - rX) <= 2.0 * LR.symprod_bound(Yb[b], Gsym, 1, 2.0)), (b, m)


def test_products_bound_on_random_data():
    bt = base_batch(1)
    rng = np.random.Generator(np.random.PCG64(2))
    Ms, Xs, Es = [symmetric(rng, m) for m in bt.ms], [symmetric(rng, m) for m in bt.ms], [general(rng, m) for m in bt.ms]
    orb = state_of(bt)
    Xd, Ed = dev(pack(Xs, poison=float("nan"))), dev(pack(Es))
    worst = {}
    for mdt in (np.float64, np.float32):
        M_ = [x.astype(mdt).astype(np.float64) for x in Ms]
        got = blocks(raw_product(orb, dev(pack(M_, mdt, poison=float("nan"))), Xd), bt.ms)
        w = 0.0
        for b, m in enumerate(bt.ms):
            f = worst_ratio(got[b], (ld(M_[b]) @ ld(Xs[b])).astype(np.float64), LR.product_bound(M_[b], Xs[b]))
            w = max(w, f)
            assert f <= 1.0, (mdt, b, m, f)
        worst["product " + np.dtype(mdt).name] = w
    for side in (0, 1):
        alpha = 1.0 + side
        got = blocks(raw_symprod(orb, Ed, Xd, side, alpha), bt.ms)
        w = 0.0
        for b, m in enumerate(bt.ms):
            El, Xl = ld(Es[b]), ld(Xs[b])
            ref = (alpha * 0.5 * (Xl @ El + El.T @ Xl if side == 0 else El @ Xl + Xl @ El.T)).astype(np.float64)
            f = worst_ratio(got[b], ref, LR.symprod_bound(Es[b], Xs[b], side, alpha))
            w = max(w, f)
            assert f <= 1.0 and np.array_equal(got[b], got[b].T), (side, b, m, f)
        worst[f"symprod side {side}"] = w
    print("orbital_lowdin_parity kernels worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- 2. the weights and the epilogue of the matrix function's reverse --------------------------------------------------------------------------------------------------
def test_weights_exactly_and_an_indefinite_overlap():
    bt = base_batch(2)
    Ss = overlaps(bt.ms)
    orb = state_of(bt).solve(dev(pack(Ss)))
    half, inv, cond, info = orb.overlap_weights()
    s = orb.energies.cpu().numpy()
    a = np.sqrt(s)
    assert info.cpu().tolist() == [0] * len(bt.ms) and same_bits(half.cpu().numpy(), a) and same_bits(inv.cpu().numpy(), 1.0 / a)
    assert same_bits(cond.cpu().numpy(), np.array([s[o:e].max() / s[o:e].min() for o, e in zip(bt.op[:-1], bt.op[1:])]))
    A, Ai, _, _ = orb.overlap_functions()
    Ab, Aib = blocks(A.cpu().numpy(), bt.ms), blocks(Ai.cpu().numpy(), bt.ms)
    for b, m in enumerate(bt.ms):
        kap, smax = np.linalg.cond(Ss[b]), np.linalg.eigvalsh(Ss[b]).max()
        assert np.array_equal(Ab[b], Ab[b].T) and np.array_equal(Aib[b], Aib[b].T)
        # the decomposition's residual and its orthogonality, each 10 m E (s_max; carried by a_i / a_j <= sqrt(kappa) over m terms for A A^-)
        assert np.abs(Ab[b] @ Ab[b] - Ss[b]).max() <= 2.0 * BOUND * m * E * smax and np.abs(Ab[b] @ Aib[b] - np.eye(m)).max() <= 2.0 * BOUND * m * E * np.sqrt(kap * m)
    bad = bt.ms.index(17)
    w, V = np.linalg.eigh(Ss[bad])
    w[3] = -0.25
    Sbad = list(Ss)
    Sbad[bad] = LR.sym((V * w[None, :]) @ V.T)                    # indefinite: the standard solve succeeds, one level is negative
    orb2 = state_of(bt).solve(dev(pack(Sbad)))
    half2, inv2, cond2, info2 = orb2.overlap_weights()
    A2, Ai2, _, _ = orb2.overlap_functions()
    assert orb2.status.cpu().tolist() == [0] * len(bt.ms) and info2.cpu().tolist() == [int(b == bad) for b in range(len(bt.ms))]
    h1, h2, i1, i2 = half.cpu().numpy(), half2.cpu().numpy(), inv.cpu().numpy(), inv2.cpu().numpy()
    for b, m in enumerate(bt.ms):
        o, e = int(bt.op[b]), int(bt.op[b + 1])
        if b == bad:
            assert np.isnan(h2[o:e]).all() and np.isnan(i2[o:e]).all() and np.isnan(float(cond2[b]))
            assert np.isnan(blocks(A2.cpu().numpy(), bt.ms)[b]).all() and np.isnan(blocks(Ai2.cpu().numpy(), bt.ms)[b]).all()
        else:
            assert same_bits(h2[o:e], h1[o:e]) and same_bits(i2[o:e], i1[o:e]) and float(cond2[b]) == float(cond[b])
            assert same_bits(blocks(A2.cpu().numpy(), bt.ms)[b], Ab[b]) and same_bits(blocks(Ai2.cpu().numpy(), bt.ms)[b], Aib[b])
    from nabladft_amd.orbitals import LowdinBasis
    with pytest.raises(RuntimeError, match=f"molecule {bad}: the overlap matrix is not positive definite"):
        LowdinBasis(orb2, A2, Ai2, cond2, info2).check()
    g = dev(pack([general(np.random.Generator(np.random.PCG64(3)), m) for m in bt.ms]))
    for kind in (0, 1):                                           # the reverse: NaN in the flagged molecule's block only
        r1, r2 = blocks(orb.matfun_response(g, kind).cpu().numpy(), bt.ms), blocks(orb2.matfun_response(g, kind).cpu().numpy(), bt.ms)
        for b in range(len(bt.ms)):
            assert np.isnan(r2[b]).all() if b == bad else same_bits(r1[b], r2[b]), (kind, b)


def test_mo_epilogue_within_the_bound():
    bt = base_batch(3)
    Ss = overlaps(bt.ms, seed=7)
    orb = state_of(bt).solve(dev(pack(Ss)))
    s, Cts = orb.energies.cpu().numpy(), blocks(orb.coefficients.cpu().numpy(), bt.ms)
    rng = np.random.Generator(np.random.PCG64(4))
    Ts = [general(rng, m) for m in bt.ms]
    Td = dev(pack(Ts))
    worst = [0.0, 0.0]
    for kind in (0, 1):
        got = blocks(raw_mo(orb, Td, kind), bt.ms)
        for b, m in enumerate(bt.ms):
            a = np.sqrt(s[int(bt.op[b]):int(bt.op[b + 1])])
            ref = LR.kernel_K(a, kind) * (ld(Cts[b]) @ ld(Ts[b])).astype(np.float64)
            f = worst_ratio(got[b], ref, LR.mo_bound(Cts[b], Ts[b], a, kind))
            worst[kind] = max(worst[kind], f)
            # the diagonal is written by the same launch: raw_mo's guard refuses an output that keeps the sentinel anywhere, the diagonal included
            assert f <= 1.0 and np.all(np.diag(got[b]) != 0.0), (kind, b, m, f)
    print("orbital_lowdin_parity kernels mo worst error / bound: kind 0 %.3f kind 1 %.3f" % tuple(worst))


def test_products_and_mo_at_the_largest_size():
    """m = 1024: one molecule, one decomposition.  The reference is plain float64 numpy, whose own rounding shares the bound."""
    m = 1024
    bt = make_batch([m], [[32] * 32])
    rng = np.random.Generator(np.random.PCG64(5))
    S = DR.overlap(m, 1e2, rng)
    Mm, X, Em = symmetric(rng, m) / m, symmetric(rng, m), general(rng, m)
    orb = state_of(bt).solve(dev(pack([S])))
    assert orb.status.cpu().tolist() == [0]
    Y = raw_product(orb, dev(pack([Mm])), dev(pack([X]))).reshape(m, m)
    f0 = worst_ratio(Y, Mm @ X, LR.product_bound(Mm, X))
    figs = [f0]
    for side in (0, 1):
        got = raw_symprod(orb, dev(pack([Em])), dev(pack([X])), side, 1.0 + side).reshape(m, m)
        assert np.array_equal(got, got.T)
        ref = (1.0 + side) * 0.5 * (X @ Em + Em.T @ X if side == 0 else Em @ X + X @ Em.T)
        figs.append(worst_ratio(got, ref, LR.symprod_bound(Em, X, side, 1.0 + side)))
    s, Ct = orb.energies.cpu().numpy(), orb.coefficients.cpu().numpy().reshape(m, m)
    a = np.sqrt(s)
    for kind in (0, 1):
        got = raw_mo(orb, dev(pack([Em])), kind).reshape(m, m)
        figs.append(worst_ratio(got, LR.kernel_K(a, kind) * (Ct @ Em), LR.mo_bound(Ct, Em, a, kind)))
    print("orbital_lowdin_parity kernels m=1024 worst error / bound: product %.3f symprod side 0 %.3f side 1 %.3f mo kind 0 %.3f kind 1 %.3f" % tuple(figs))
    assert all(f <= 1.0 for f in figs), figs


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------------------------------------------
CASES = [c for c in DR.CASES if c[1] < c[0]]                       # with a virtual orbital: with every orbital occupied the H gradients vanish
KEYS = ("pop", "bond", "valence", "HL", "gH", "gS")


def lowdin_loss(ptr, m, wq, Wt, wv, Gh):
    """L = w_q . q + sum Wt o W + w_v . V + 1/2 |W|^2 + sum Gh o H^L + 1/2 |H^L|^2 as a function of torch (eps, D, S, H); Gh is NOT symmetric."""
    wq, Wt, wv, Gh = (torch.from_numpy(x) for x in (wq, Wt, wv, Gh))

    def loss(eps, D, S, H):
        q, W, V, HL = LR.torch_lowdin(D, S, H, ptr)
        return (wq * q).sum() + (Wt * W).sum() + (wv * V).sum() + 0.5 * (W * W).sum() + (Gh * HL).sum() + 0.5 * (HL * HL).sum()
    return loss


def values(D, S, H, ptr):
    DL, q, W, V = LR.lowdin(D, S, ptr)
    return dict(pop=q, bond=W, valence=V, HL=LR.congruence(LR.functions(S)[1], H)[0], DL=DL)


def propagated(H, S, D, ptr, n_occ, eps):
    """The bounds of the module text for q, W, V and H^L of one molecule."""
    m, n = S.shape[0], len(ptr) - 1
    A, Ai, s, _ = LR.functions(S)
    kap = s.max() / s.min()
    J = np.ones((m, m))
    dD = BOUND * PR.density_unit(H, S, n_occ, eps, D) * J
    dA, dAi = BOUND * m * E * np.sqrt(kap * s.max()) * J, BOUND * m * E * kap / np.sqrt(s.min()) * J
    out = {}
    for X, dX, Mx, dM, key in ((A, dA, D, dD, "DL"), (Ai, dAi, H, 0.0 * J, "HL")):
        Y = Mx @ X
        dY = LR.product_bound(Mx, X) + dM @ np.abs(X) + np.abs(Mx) @ dX
        t = dX @ np.abs(Y) + np.abs(X) @ dY
        out[key] = LR.symprod_bound(Y, X, 0) + 0.5 * (t + t.T)
    DL = LR.congruence(A, D)[0]
    Ai_ = indicator(ptr, m)
    out["pop"] = Ai_ @ np.diag(out["DL"]) + (np.diff(ptr) + 4) * U * (Ai_ @ np.abs(np.diag(DL)))
    out["bond"] = BR.bond_bound(DL, ptr) + Ai_ @ (2.0 * np.abs(DL) * out["DL"]) @ Ai_.T
    off = 1.0 - np.eye(n)
    out["valence"] = (out["bond"] * off).sum(1) + (n + 4) * U * (BR.bond_magnitudes(DL, ptr) * off).sum(1)
    return out


@functools.lru_cache(maxsize=None)
def reference(inputs):
    out = []
    for ci, case in enumerate(CASES):
        m, n_occ = case[0], case[1]
        H, S = DR.gapped_case(*case)
        if inputs == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        sizes = partition(m, ci) if m > 32 else [1] * m if m <= 3 else partition(m, 2)
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        n = len(sizes)
        rng = np.random.Generator(np.random.PCG64(9000 + ci))
        wq, Wt, wv, Gh = rng.normal(size=n), rng.normal(size=(n, n)), rng.normal(size=n), rng.normal(size=(m, m))
        # on the CPU first: the backward of eigh divides by the gaps of s, which must be resolved
        gap = LR.min_relative_gap(np.linalg.eigvalsh(S))
        assert gap > m * 2.0 ** -40, (case, gap)
        loss = lowdin_loss(ptr, m, wq, Wt, wv, Gh)
        eps, D, gH, gS = DR.autograd(H, S, n_occ, loss)
        _, _, gH_D, gS_D = DR.autograd(H, S, n_occ, lambda e, d, s_, h_: loss(e, d, s_.detach(), h_.detach()))        # the part that arrives through D
        val = values(D, S, H, ptr)
        aperm = rng.permutation(n)
        perm = np.concatenate([ptr[a] + rng.permutation(sizes[a]) for a in aperm]).astype(np.int64)
        ptr2 = np.concatenate([[0], np.cumsum([sizes[a] for a in aperm])])
        ix, ax = np.ix_(perm, perm), np.ix_(aperm, aperm)
        _, D2, gH2, gS2 = DR.autograd(H[ix], S[ix], n_occ, lowdin_loss(ptr2, m, wq[aperm], Wt[ax], wv[aperm], Gh[ix]))
        v2 = values(D2, S[ix], H[ix], ptr2)
        back = dict(pop=unpermute(v2["pop"], aperm), bond=unpermute(v2["bond"], ax), valence=unpermute(v2["valence"], aperm), HL=unpermute(v2["HL"], ix),
                    gH=unpermute(gH2, ix), gS=unpermute(gS2, ix))
        ref = dict(val, gH=gH, gS=gS)
        spread = {k: float(np.abs(ref[k] - back[k]).max()) for k in KEYS}
        assert all(np.isfinite(v) for v in spread.values()), (case, spread)
        uH, uS = DR.units(H, S, n_occ, eps, gH, gS)
        prop = propagated(H, S, D, ptr, n_occ, eps)
        prop.update(gH=BOUND * uH, gS=BOUND * uS)
        out.append(SimpleNamespace(case=case, H=H, S=S, ptr=ptr, sizes=sizes, w=(wq, Wt, wv, Gh), eps=eps, D=D, ref=ref, spread=spread, prop=prop, min_gap=gap,
                                   f32_terms=dict(gH=np.abs(gH_D) + np.abs(gH - gH_D) + np.abs(gH), gS=np.abs(gS_D) + np.abs(gS - gS_D) + np.abs(gS))))
    return out


@pytest.mark.parametrize("inputs", ["float64", "float32"])
def test_lowdin_end_to_end(inputs):
    import nabladft_amd as nq
    refs = reference(inputs)
    bt = make_batch([r.case[0] for r in refs], [r.sizes for r in refs])
    nos = [r.case[1] for r in refs]
    tdt = getattr(torch, inputs)
    H, S = dev(pack([r.H for r in refs]), tdt).requires_grad_(True), dev(pack([r.S for r in refs]), tdt).requires_grad_(True)
    eps, D, sol = nq.orbital_solution(H, S, bt.op, nos, return_solution=True)
    basis = nq.lowdin_basis(S, bt.op)
    pop, nelec, none = nq.lowdin_populations(D, bt.plan, basis)
    bond, val = nq.lowdin_bond_orders(D, bt.plan, basis)
    HL = nq.lowdin_hamiltonian(H, basis)
    assert none is None and all(t.dtype == torch.float64 and t.requires_grad for t in (pop, nelec, bond, val, HL, basis.half, basis.inv_half))
    assert pop.numel() == bt.N and bond.numel() == bt.Q and HL.numel() == int(bt.pp[-1]) and basis.cond.numel() == len(refs)
    total = 0.0
    for b, r in enumerate(refs):
        m = r.case[0]
        wq, Wt, wv, Gh = (dev(x) for x in r.w)
        atoms = slice(int(bt.aptr[b]), int(bt.aptr[b + 1]))
        Wd, Hd = nq.dense_bond_orders(bond, bt.aptr, b), HL[int(bt.pp[b]):int(bt.pp[b + 1])].view(m, m)
        total = total + (wq * pop[atoms]).sum() + (Wt * Wd).sum() + (wv * val[atoms]).sum() + 0.5 * (Wd * Wd).sum() + (Gh * Hd).sum() + 0.5 * (Hd * Hd).sum()
    total.backward()
    sol.check()
    basis.check()
    assert H.grad.dtype == tdt and S.grad.dtype == tdt and H.grad.shape == H.shape and S.grad.shape == S.shape
    out_round = 2.0 ** -24 if inputs == "float32" else 0.0
    Ws, pops, vals = bond_blocks(bond.detach().cpu().numpy(), bt), pop.detach().cpu().numpy(), val.detach().cpu().numpy()
    HLs, gHs, gSs = blocks(HL.detach().cpu().numpy(), bt.ms), blocks(H.grad.double().cpu().numpy(), bt.ms), blocks(S.grad.double().cpu().numpy(), bt.ms)
    conds = basis.cond.cpu().numpy()
    for b, r in enumerate(refs):
        m, n_occ = r.case[0], r.case[1]
        atoms = slice(int(bt.aptr[b]), int(bt.aptr[b + 1]))
        got = dict(pop=pops[atoms], bond=Ws[b], valence=vals[atoms], HL=HLs[b], gH=gHs[b], gS=gSs[b])
        assert all(np.array_equal(got[k], got[k].T) for k in ("bond", "HL", "gH", "gS"))
        assert abs(conds[b] - np.linalg.cond(r.S)) <= 1e-6 * conds[b]
        line = []
        for k in KEYS:
            rounding = out_round * r.f32_terms[k] if k in ("gH", "gS") else 0.0
            err = np.maximum(np.abs(got[k] - r.ref[k]) - rounding, 0.0)
            allow = np.maximum(10.0 * r.spread[k], r.prop[k])
            fig = float((err / np.maximum(allow, TINY)).max())
            line.append(f"{k} {fig:.3g} of the allowance ({float(err.max()) / max(r.spread[k], TINY):.3g} spreads; allowance {float(np.max(allow)) / max(r.spread[k], TINY):.3g} spreads)")
        print(f"orbital_lowdin_parity end-to-end {inputs} m={m} n_occ={n_occ} kappa0={r.case[3]:g} atoms={len(r.sizes)} min gap of s {r.min_gap:.2g}: " + "; ".join(line))
        for k in KEYS:
            rounding = out_round * r.f32_terms[k] if k in ("gH", "gS") else 0.0
            err = np.maximum(np.abs(got[k] - r.ref[k]) - rounding, 0.0)
            assert np.all(err <= np.maximum(10.0 * r.spread[k], r.prop[k])), (inputs, r.case, k)


# ---- 4. degenerate levels of S ------------------------------------------------------------------------------------------------------------------------------------------
def test_degenerate_levels_give_finite_gradients():
    """S = I and two identical atoms far apart (every level twice): the gradients of sum g_half o S^(1/2) + sum g_inv o S^(-1/2) are finite and equal the closed
    form, which does not depend on the basis chosen inside a degenerate level; the backward of torch.linalg.eigh is not finite there.  Allowance: 10 m E kappa^2
    of the largest entry (K varies by kappa^(3/2) over the levels, U by m E)."""
    import nabladft_amd as nq
    blk = DR.overlap(5, 10.0, np.random.Generator(np.random.PCG64(61)))
    two = np.zeros((10, 10))
    two[:5, :5] = blk
    two[5:, 5:] = blk
    Ss = [np.eye(6), two, np.eye(1), np.eye(65)]
    ms = [s.shape[0] for s in Ss]
    rng = np.random.Generator(np.random.PCG64(62))
    gh, gi = [general(rng, m) for m in ms], [general(rng, m) for m in ms]
    op = np.concatenate([[0], np.cumsum(ms)])
    exact = Ss
    for tdt in (torch.float64, torch.float32):
        Ss = exact if tdt == torch.float64 else [s.astype(np.float32).astype(np.float64) for s in exact]       # the reference sees the inputs the device sees
        S = dev(pack(Ss), tdt).requires_grad_(True)
        basis = nq.lowdin_basis(S, op)
        ((dev(pack(gh)) * basis.half).sum() + (dev(pack(gi)) * basis.inv_half).sum()).backward()
        basis.check()
        got = blocks(S.grad.double().cpu().numpy(), ms)
        assert S.grad.dtype == tdt
        for b, m in enumerate(ms):
            s, Uv = LR.decompose(Ss[b])
            r0, r1 = LR.matfun_response(gh[b], s, Uv, 0), LR.matfun_response(gi[b], s, Uv, 1)
            ref = r0 + r1
            if b != 1:
                assert np.abs(ref - 0.5 * LR.sym(gh[b] - gi[b])).max() <= 8 * E * np.abs(ref).max()       # g / 2 and -g / 2
            kap = s.max() / s.min()
            allow = BOUND * m * E * kap ** 2 * np.abs(ref).max() + (2.0 ** -24 * (np.abs(r0 + r1)) if tdt == torch.float32 else 0.0)
            assert np.isfinite(got[b]).all() and np.array_equal(got[b], got[b].T) and np.all(np.abs(got[b] - ref) <= allow), (tdt, b, float(np.abs(got[b] - ref).max()))
    for b in (0, 1):                                              # the route through eigh's backward
        St = torch.tensor(exact[b], requires_grad=True)
        A, Ai = LR.torch_functions(St)
        ((torch.from_numpy(gh[b]) * A).sum() + (torch.from_numpy(gi[b]) * Ai).sum()).backward()
        assert not np.isfinite(St.grad.numpy()).all(), b
    print("orbital_lowdin_parity degenerate levels: S = I (m = 1, 6, 65) and two identical atoms: finite, equal to the closed form; torch.linalg.eigh backward non-finite")


# ---- 5. the sum rules ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_sum_rules(tag, b, m, ptr, Dm, Sm, DL, q, W, nelec_b, rel_idem, HLm=None, eps_b=None):
    """One molecule.  With dS = |A A - S| <= 2 x 10 m E s_max per entry (the decomposition's residual and its orthogonality) and dDL the dot-product bounds of
    Y = D A and sym(A Y):  Tr(D^L) - Tr(D S) = Tr(D (A A - S)) + rounding;  (D^L D^L - 2 D^L)_mu,mu = [A (D S D - 2 D) A + A D (A A - S) D A]_mu,mu + rounding, the
    first term rel_idem x 2 (|A||D||A|)_mu,mu."""
    A = LR.functions(Sm)[0]
    kap, smax = float(np.linalg.cond(Sm)), float(np.linalg.eigvalsh(Sm).max())
    aA, aD = np.abs(A), np.abs(Dm)
    dS = 2.0 * BOUND * m * E * smax * np.ones((m, m))
    Y = Dm @ A
    t = aA @ LR.product_bound(Dm, A)
    dDL = LR.symprod_bound(Y, A, 0) + 0.5 * (t + t.T)
    Ai_ = indicator(ptr, m)
    sizes = np.diff(ptr)
    diag_mag = float(np.abs(np.diag(DL)).sum())
    allow_n = float((aD * dS).sum()) + float(np.diag(dDL).sum()) + 2.0 * (m * m + 4) * U * float((aD * np.abs(Sm)).sum()) + (m + 4) * U * diag_mag
    f_n = abs(q.sum() - nelec_b) / allow_n
    ADA = aA @ aD @ aA
    rows = (rel_idem * 2.0 * np.diag(ADA) + np.diag(aA @ aD @ dS @ aD @ aA) + (2.0 * np.abs(DL) * dDL).sum(1) + 2.0 * np.diag(dDL)
            + (m + 4) * U * ((DL * DL).sum(1) + 2.0 * np.abs(np.diag(DL))))
    allow_w = Ai_ @ rows + (sizes * m + 4) * U * (Ai_ @ (DL * DL).sum(1))
    err = np.abs(W.sum(1) - 2.0 * q)
    f_w = float((err / allow_w).max())
    line = f"orbital_lowdin_parity sum rule {tag} molecule {b} m={m}: |sum q - Tr(DS)| / allowance {f_n:.3g}; worst |sum_B W_AB - 2 q_A| / allowance {f_w:.3g}"
    f_e = 0.0
    if HLm is not None:
        f_e = float(np.abs(np.linalg.eigvalsh(HLm) - eps_b).max() / (2.0 * BOUND * m * E * kap * max(eps_b.max() - eps_b.min(), np.abs(eps_b).max())))
        line += f"; |eigvalsh(H^L) - eps| / allowance {f_e:.3g}"
    print(line)
    assert f_n <= 1.0 and f_w <= 1.0 and f_e <= 1.0 and np.array_equal(W, W.T), (tag, b, f_n, f_w, f_e)


def test_sum_rules_on_the_solver_and_the_purified_density():
    import nabladft_amd as nq
    refs = reference("float64")
    bt = make_batch([r.case[0] for r in refs], [r.sizes for r in refs])
    nos = [r.case[1] for r in refs]
    H, S = dev(pack([r.H for r in refs])), dev(pack([r.S for r in refs]))
    eps, D, sol = nq.orbital_solution(H, S, bt.op, nos, return_solution=True)
    Dp, pur = nq.purified_density_matrix(H, S, bt.op, nos, return_solution=True)
    basis = nq.lowdin_basis(S, bt.op)
    sol.check()
    pur.check()
    basis.check()
    HLs = blocks(nq.lowdin_hamiltonian(H, basis).cpu().numpy(), bt.ms)
    epsn = eps.cpu().numpy()
    for tag, dens, owner in (("solver", D, sol), ("purified", Dp, pur)):
        DLs = blocks(nq.lowdin_density(dens, basis).cpu().numpy(), bt.ms)
        pop, nel_l, _ = nq.lowdin_populations(dens, bt.plan, basis)
        bond, val = nq.lowdin_bond_orders(dens, bt.plan, basis)
        _, nelec, _ = owner.populations(dens, bt.plan, S)
        Ws, pops, Dbs = bond_blocks(bond.cpu().numpy(), bt), pop.cpu().numpy(), blocks(dens.cpu().numpy(), bt.ms)
        if tag == "purified":                                     # the layout-only launches serve a purification state alike
            DLp, Yp = pur.sym_congruence(basis.half, dens)
            assert same_bits(DLp.cpu().numpy(), nq.lowdin_density(dens, basis).cpu().numpy())
        for b, r in enumerate(refs):
            m, n_occ = r.case[0], r.case[1]
            rel = BOUND * m * R.EPS * float(np.linalg.cond(r.S)) if tag == "solver" else BOUND * PR.density_unit(r.H, r.S, n_occ, r.eps, r.D) / np.abs(r.D).max()
            atoms = slice(int(bt.aptr[b]), int(bt.aptr[b + 1]))
            check_sum_rules(tag, b, m, r.ptr, Dbs[b], r.S, DLs[b], pops[atoms], Ws[b], float(nelec[b]), rel, HLs[b] if tag == "solver" else None,
                            epsn[int(bt.op[b]):int(bt.op[b + 1])])
            assert abs(float(nel_l[b]) - pops[atoms].sum()) <= (len(r.sizes) + 4) * U * np.abs(pops[atoms]).sum() * 2


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
    basis = nq.LowdinBasis.of(Sd, bt.op)
    assert orb.status.tolist() == [0, 0, 0, 0, 0, 1] and basis.info.tolist() == [0, 0, 0, 0, 0, 1]       # the last molecule's overlap is indefinite
    D = orb.density(n_occ)
    DLs = blocks(nq.lowdin_density(D, basis).cpu().numpy(), ms)
    HLs = blocks(nq.lowdin_hamiltonian(Hd, basis).cpu().numpy(), ms)
    pop, _, _ = nq.lowdin_populations(D, plan, basis)
    bond, val = nq.lowdin_bond_orders(D, plan, basis)
    _, nelec, _ = orb.populations(D, plan, Sd)
    Ws, pops, Dbs, vals, epsn = bond_blocks(bond.cpu().numpy(), bt), pop.cpu().numpy(), blocks(D.cpu().numpy(), ms), val.cpu().numpy(), orb.energies.cpu().numpy()
    q = nq.lowdin_charges(z, pop).cpu().numpy()
    for b, m in enumerate(ms):
        atoms = slice(int(aptr[b]), int(aptr[b + 1]))
        if b == 5:
            assert np.isnan(Ws[b]).all() and np.isnan(pops[atoms]).all() and np.isnan(DLs[b]).all() and np.isnan(HLs[b]).all()
            continue
        check_sum_rules("database", b, m, bt.ptr[b], Dbs[b], Ss[b], DLs[b], pops[atoms], Ws[b], float(nelec[b]), BOUND * m * R.EPS * float(np.linalg.cond(Ss[b])),
                        HLs[b], epsn[int(bt.op[b]):int(bt.op[b + 1])])
        assert abs(q[atoms].sum()) <= 1e-9 * z[atoms].sum() and np.isfinite(vals[atoms]).all()       # neutral molecules
        heavy = [i for i, zz in enumerate(probs[b][2]) if int(zz) > 1]
        print(f"orbital_lowdin_parity database molecule {b} m={m} atoms {natoms[b]}: Löwdin charges of the heavy atoms {np.round(q[atoms][heavy], 3).tolist()}, "
              f"largest off-diagonal Wiberg index {float((Ws[b] - np.diag(np.diag(Ws[b]))).max()):.3f}")
    good = dev(q[:int(aptr[5])])
    assert float(nq.LowdinChargeLoss("mae")(good, good.clone(), aptr[:6])) == 0.0
    assert abs(float(nq.LowdinChargeLoss("mse")(good + 0.5, good, aptr[:6])) - 0.25) <= 1e-12
    with pytest.raises(ValueError, match="entries"):
        nq.LowdinChargeLoss()(good[:-1], good[:-1], aptr[:6])


# ---- 6. run to run, the rest of the batch, a failed molecule, refusals ------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_batch_independent_and_a_failed_molecule():
    refs = reference("float64")
    pick = [2, 3, 4, 5]                                            # m = 17, 65, 130, 130 (kappa0 = 1e4)
    Hs, Ss, nos, parts = [refs[i].H for i in pick], [refs[i].S for i in pick], [refs[i].case[1] for i in pick], [refs[i].sizes for i in pick]
    ms = [h.shape[0] for h in Hs]
    rng = np.random.Generator(np.random.PCG64(9))
    Gs = [symmetric(rng, m) for m in ms]
    bad_status = torch.tensor([0, 0, 2, 0], dtype=torch.int32)

    def run(idx, fail=False):
        from nabladft_amd.orbitals import BatchedOrbitals
        bt = make_batch([ms[i] for i in idx], [parts[i] for i in idx])
        Sd, Hd = dev(pack([Ss[i] for i in idx])), dev(pack([Hs[i] for i in idx]))
        orb = BatchedOrbitals(bt.op, DEV).solve(Sd)
        if fail:                                                  # as if the decomposition had not converged on molecule 2
            orb.state.status.copy_(bad_status.to(DEV))
        A, Ai, cond, info = orb.overlap_functions()
        HL, Y = orb.sym_congruence(Ai, Hd)
        G = dev(pack([Gs[i] for i in idx]))
        gM, gX = orb.sym_congruence_backward(G, Ai, Y)
        gS = orb.matfun_response(gX, 1)
        return bt, info.cpu().numpy(), [t.cpu().numpy() for t in (A, Ai, HL, Y, gM, gX, gS)]
    every = list(range(len(ms)))
    bt, info, packed = run(every)
    _, info2, packed2 = run(every)
    assert not info.any() and all(same_bits(x, y) for x, y in zip(packed, packed2))
    for b in (0, 1, 3):                                            # alone: the same bits as inside the batch
        _, _, pa = run([b])
        for x, y in zip(pa, packed):
            assert same_bits(x.reshape(ms[b], ms[b]), blocks(y, ms)[b]), (b, ms[b])
    _, infof, packedf = run(every, fail=True)
    assert infof.tolist() == [0, 0, 1, 0]
    for b in every:
        own, was = [blocks(y, ms)[b] for y in packedf], [blocks(y, ms)[b] for y in packed]
        assert all(np.isnan(x).all() for x in own) if b == 2 else all(same_bits(x, y) for x, y in zip(own, was)), b


def test_dimension_mismatch_touches_nothing_and_python_refusals():
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import BatchedPurification
    bt = make_batch([5, 3], [[2, 3], [3]])
    orb = state_of(bt)
    st = orb.state
    lib = _lib.load()
    big, big2, big3 = (torch.full((40,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(3))
    ibig = torch.full((4,), -77, dtype=torch.int32, device=DEV)
    src = torch.ones(40, dtype=torch.float64, device=DEV)
    for fn, args in ((lib.nq_orb_low_weights, (_lib.ptr(big), _lib.ptr(big2), _lib.ptr(big3), _lib.ptr(ibig))),
                     (lib.nq_orb_low_product, (_lib.ptr(src), 1, _lib.ptr(src), _lib.ptr(big))),
                     (lib.nq_orb_low_symprod, (_lib.ptr(src), _lib.ptr(src), 0, 1.0, _lib.ptr(big))),
                     (lib.nq_orb_low_symmetrize, (_lib.ptr(src), _lib.ptr(big))),
                     (lib.nq_orb_low_mo, (0, _lib.ptr(src), _lib.ptr(big)))):
        assert fn(_lib.ptr(st.buf), 2, 8, 36, *args, _lib.stream_ptr()) == 0, lib.nq_last_error()       # (2, 8, 36) instead of (2, 8, 34)
        torch.cuda.synchronize()
        assert int(st.header_dev[4]) == -2 and all(bool((t == SENTINEL).all()) for t in (big, big2, big3)) and bool((ibig == -77).all())
        with pytest.raises(RuntimeError, match="other dimensions"):
            st.header()
        st.header_dev[4] = 0
    Sd = dev(pack([np.eye(5), 4.0 * np.eye(3)]))
    basis = nq.LowdinBasis.of(Sd, bt.op).check()
    assert basis.half.cpu().tolist() == pack([np.eye(5), 2.0 * np.eye(3)]).tolist() and basis.inv_half.cpu().tolist() == pack([np.eye(5), 0.5 * np.eye(3)]).tolist()
    assert basis.cond.cpu().tolist() == [1.0, 1.0] and basis.s.cpu().tolist() == [1.0] * 5 + [4.0] * 3
    D = dev(pack([2.0 * np.eye(5), np.eye(3)]))
    pop, nelec, _ = nq.lowdin_populations(D, bt.plan, basis)
    assert pop.cpu().tolist() == [4.0, 6.0, 12.0] and nelec.cpu().tolist() == [10.0, 12.0]
    # the readers of eps and coeff refuse a purification state (header status -3), the layout-only launches do not
    pur = BatchedPurification(bt.op, DEV)
    pur.orthogonalize(Sd)
    DL, Y = pur.sym_congruence(basis.half, D)
    assert same_bits(DL.cpu().numpy(), nq.lowdin_density(D, basis).cpu().numpy()) and int(pur.state.header_dev[4]) == 0
    assert lib.nq_orb_low_mo(_lib.ptr(pur.state.buf), *pur.state._dims, 0, _lib.ptr(src[:34]), _lib.ptr(big[:34]), _lib.stream_ptr()) == 0
    assert lib.nq_orb_low_weights(_lib.ptr(pur.state.buf), *pur.state._dims, _lib.ptr(big), _lib.ptr(big2), _lib.ptr(big3), _lib.ptr(ibig), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(pur.state.header_dev[4]) == -3 and all(bool((t == SENTINEL).all()) for t in (big, big2, big3)) and bool((ibig == -77).all())
    with pytest.raises(ValueError, match="side must be 0"):
        orb.low_symprod(D, D, 2)
    with pytest.raises(ValueError, match="kind must be 0"):
        orb.matfun_response(D, 2)
    with pytest.raises(ValueError, match="float64"):
        orb.low_product(D, D.float())
    with pytest.raises(ValueError, match="entries"):
        orb.low_product(D[:-1], D)
    with pytest.raises(TypeError, match="LowdinBasis"):
        nq.lowdin_density(D, orb)
    with pytest.raises(ValueError, match="the basis packs"):
        nq.lowdin_hamiltonian(D[:-1], basis)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.lowdin_basis(Sd.cpu(), bt.op)


# ---- 7. the QHNet task ------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_lowdin_task(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd import orbital_loss as OL
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
            "density_matrix": nq.DensityMatrixLoss("mse", charge), "mulliken_charges": nq.MullikenChargeLoss("mse", charge), "bond_orders": nq.BondOrderLoss("mse", charge)}
    base_c = {"hamiltonian": 1.0, "orbital_energies": 0.25, "density_matrix": 0.5, "mulliken_charges": 2.0, "bond_orders": 0.75}
    losses = dict(base, lowdin_charges=nq.LowdinChargeLoss("mse", charge), lowdin_bond_orders=nq.BondOrderLoss("mse", charge))
    coefs = dict(base_c, lowdin_charges=1.5, lowdin_bond_orders=0.6)
    make = lambda cls, ls, cs: cls("QHNet", net, None, None, ls, None, None, cs)
    solves, bases = [], []
    real, real_basis = OrbitalState.solve, OL.lowdin_basis
    monkeypatch.setattr(OrbitalState, "solve", lambda self, *a, **k: (solves.append(1), real(self, *a, **k))[1])
    monkeypatch.setattr(OL, "lowdin_basis", lambda *a, **k: (bases.append(1), real_basis(*a, **k))[1])
    params = [p for p in net.parameters() if p.requires_grad]

    def step(task):
        for p in params:
            p.grad = None
        loss = task.training_step(batch, 0)
        loss.backward()
        return loss.detach(), [None if p.grad is None else p.grad.detach().clone() for p in params]
    task = make(nq.QHNetLowdinLightning, losses, coefs)
    loss, grads = step(task)
    assert len(bases) == 1 and len(solves) == 3, (len(bases), len(solves))      # one basis per step; prediction, target and the decomposition of S
    assert bool(torch.isfinite(loss)) and all(gr is None or bool(torch.isfinite(gr).all()) for gr in grads) and any(gr is not None for gr in grads)
    preds, targets, _ = task._evaluate(batch)
    assert len(bases) == 2 and len(solves) == 6
    n = np.asarray(g["sizes"], dtype=np.int64)
    terms = {}
    for k, count in (("lowdin_charges", int(n.sum())), ("lowdin_bond_orders", int((n * n).sum()))):
        p, t = preds[k], targets[k]
        assert p.numel() == count and p.requires_grad and not t.requires_grad and bool(torch.isfinite(p).all()) and bool(torch.isfinite(t).all())
        terms[k] = losses[k](p, t, batch.ptr).detach()
        assert float(terms[k]) > 0.0 and float(losses[k](p, p.detach().clone(), batch.ptr)) == 0.0
    qp, qt = preds["lowdin_charges"].detach().cpu().numpy(), targets["lowdin_charges"].cpu().numpy()
    by_hand = np.mean([((qp[int(a):int(e)] - qt[int(a):int(e)]) ** 2).mean() for a, e in zip(np.concatenate([[0], np.cumsum(n)])[:-1], np.cumsum(n))])
    assert abs(float(terms["lowdin_charges"]) - by_hand) <= 1e-12 * by_hand
    bp, btg = preds["lowdin_bond_orders"].detach().cpu().numpy(), targets["lowdin_bond_orders"].cpu().numpy()
    by_hand = np.mean([((nq.dense_bond_orders(bp, batch.ptr, b) - nq.dense_bond_orders(btg, batch.ptr, b)) ** 2).mean() for b in range(len(n))])
    assert abs(float(terms["lowdin_bond_orders"]) - by_hand) <= 1e-12 * by_hand
    # Löwdin charges of a neutral-by-count molecule sum to its charge, like the Mulliken ones
    # the loss is the parent's plus the two terms times their coefficients
    parent = make(nq.QHNetBondOrderLightning, base, base_c)
    before = (len(solves), len(bases))
    loss_p, grads_p = step(parent)
    assert (len(solves), len(bases)) == (before[0] + 2, before[1])
    assert [gr is None for gr in grads] == [gr is None for gr in grads_p]
    extra = 1.5 * terms["lowdin_charges"].double() + 0.6 * terms["lowdin_bond_orders"].double()
    print("orbital_lowdin_parity qhnet task loss %.9g parent %.9g lowdin charge term %.6g lowdin bond term %.6g" %
          (float(loss), float(loss_p), float(terms["lowdin_charges"]), float(terms["lowdin_bond_orders"])))
    assert torch.allclose((loss - loss_p).double(), extra, rtol=1e-4, atol=1e-6 * float(loss.abs()))
    # the coefficients at 0, or no keys: QHNetBondOrderLightning's step, bit for bit, no basis
    zero = make(nq.QHNetLowdinLightning, losses, dict(coefs, lowdin_charges=0.0, lowdin_bond_orders=0.0))
    before = (len(solves), len(bases))
    loss_z, grads_z = step(zero)
    assert (len(solves), len(bases)) == (before[0] + 2, before[1])
    assert loss_z.dtype == loss_p.dtype and torch.equal(loss_z, loss_p)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads_z, grads_p))
    nokey = make(nq.QHNetLowdinLightning, base, base_c)
    loss_n, grads_n = step(nokey)
    assert torch.equal(loss_n, loss_p) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads_n, grads_p))
    with pytest.raises(ValueError, match="different charges"):
        make(nq.QHNetLowdinLightning, dict(losses, lowdin_charges=nq.LowdinChargeLoss("mse", 0)), coefs).training_step(batch, 0)
    overlap, batch.overlap = batch.overlap, None
    with pytest.raises(ValueError, match="need batch.overlap"):
        make(nq.QHNetLowdinLightning, losses, coefs).training_step(batch, 0)
    batch.overlap = overlap
