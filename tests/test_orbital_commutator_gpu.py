"""GPU: the SCF-residual kernels (csrc/orbcomm.hip) through the C ABI and through ``BatchedOrbitals`` / ``nabladft_amd.orbital_loss.commutator`` / ``scf_residual`` /
``QHNetCommutatorLightning`` / ``ScfResidualErrors``, against the numpy restatement and the torch yardstick of tests/orbital_commutator_ref.py.

Bounds (U = 2^-53, E = 2^-52; ``orbital_commutator_ref`` states them).  Product: an entry is a sum of 2 m terms in one accumulator set, so
|C - ref| <= (2 m + 4) U |alpha| (|X||Y| + |Y||X|); references in extended precision, at m = 1024 plain float64 numpy, whose own rounding shares the bound.  Small
integers make every sum exact: compared bit for bit (the sign of a zero aside).  ``antisymmetrize`` is one difference and one exact halving: bit for bit.  Norms:
m^2 U sum R^2 against numpy's sum; the maximum exactly.

End to end.  The yardstick is ``orbital_commutator_ref.torch_scf_residual`` (``torch.linalg.eigh`` of S -> U f(s) U^T -> the two congruences -> the dense
commutator), autograd through all of it, for L = sum G o R + 1/2 |R|^2 with a NON-antisymmetric G.  Its own spread is measured first on a copy with the
orbitals shuffled, mapped back.  Allowance per quantity, as tests/test_orbital_lowdin_gpu.py has it: max(10 x that spread, a floor from the number formats).
The floors: S^(1/2) and S^(-1/2) carry the decomposition of S, m E relative to s_max, through f(s): m E sqrt(kappa) relative each, and every quantity holds two
such factors, so R, gH and gD are allowed 10 m E kappa of the magnitude of their own sums (the products taken with absolute values); gS passes through the
Daleckii-Krein form, 10 m E kappa^2 of its largest entry, the allowance of the degenerate-level test of tests/test_orbital_lowdin_gpu.py.  The figures are
printed as ``orbital_commutator_parity ...`` lines (kept in profiles/orbital_commutator_parity.txt).

The chain bound of a residual that should vanish: with dHL, dDL the bounds of the two congruences (``propagated`` of tests/test_orbital_lowdin_gpu.py, which
includes the 10 U_D of the solver's density), |R| <= product_bound(HL, DL) + dHL |DL| + |HL| dDL + |DL| dHL + dDL |HL|."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import orbital_commutator_ref as CR
import orbital_density_ref as DR
import orbital_lowdin_ref as LR
from test_orbital_bond_gpu import SENTINEL, call, general, guarded, ld, make_batch, partition, same_values, symmetric, unguard, unpermute, worst_ratio
from test_orbital_loss_gpu import blocks
from test_orbital_lowdin_gpu import propagated
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130]        # one orbital .. across the 16-, 64- and 128-orbital edges of the sub-tiles and tiles
U = CR.U
E = 2.0 ** -52
TINY = np.finfo(np.float64).tiny


def ragged(seed=0, extra=()):
    order = np.random.Generator(np.random.PCG64(700 + seed)).permutation(len(SIZES))
    ms = [SIZES[i] for i in order] + list(extra)
    return make_batch(ms, [[m] for m in ms])


def state_of(bt):
    from nabladft_amd.orbitals import BatchedOrbitals
    return BatchedOrbitals(bt.op, DEV)


def raw_product(orb, Xd, x_anti, Yd, alpha):
    from nabladft_amd import _lib
    buf, out = guarded(orb.state.P)
    call("nq_orb_comm_product", orb.state, _lib.ptr(Xd), int(x_anti), _lib.ptr(Yd), float(alpha), _lib.ptr(out))
    return unguard(buf, "C")


def raw_antisymmetrize(orb, Gd):
    from nabladft_amd import _lib
    buf, out = guarded(orb.state.P)
    call("nq_orb_comm_antisymmetrize", orb.state, _lib.ptr(Gd), _lib.ptr(out))
    return unguard(buf, "Ga")


def raw_norms(orb, Rd):
    from nabladft_amd import _lib
    B = orb.state.B
    buf, out = guarded(2 * B)
    call("nq_orb_comm_norms", orb.state, _lib.ptr(Rd), _lib.ptr(out[:B]), _lib.ptr(out[B:]))
    h = unguard(buf, "norms")
    return h[:B], h[B:]


def anti_operand(rng, m, integers=False, garbage=None):
    """An antisymmetric matrix; ``garbage``: written over the diagonal and the upper triangle, which the kernel must not read."""
    A = np.tril(general(rng, m, integers), -1)
    full = A - A.T
    if garbage is None:
        return full, full
    stored = A.copy()
    stored[np.triu_indices(m)] = garbage
    return full, stored


def structure_ok(Cb, x_anti):
    if x_anti:
        return same_bits(Cb, Cb.T)
    return same_bits(Cb + Cb.T, np.zeros_like(Cb)) and not np.diag(Cb).any() and not np.signbit(np.diag(Cb)).any()


# ---- 1. the product --------------------------------------------------------------------------------------------------------------------------------------------------
def test_product_exact_placement_with_small_integers():
    """Small integers (|entries| <= 3, at most 2 x 130 x 9 per sum): every partial sum is exact, so tile offsets, the run-time operand orientation, the signs of
    the antisymmetric operand and of the second term, and the mirrored stores are compared with numpy bit for bit.  The upper triangles of the symmetric
    operands, and the diagonal and upper triangle of the antisymmetric one, hold garbage, which must not change a bit."""
    bt = ragged()
    rng = np.random.Generator(np.random.PCG64(1))
    Xs, Ys = [symmetric(rng, m, True) for m in bt.ms], [symmetric(rng, m, True) for m in bt.ms]
    As = [anti_operand(rng, m, True, garbage=-7e29) for m in bt.ms]
    orb = state_of(bt)
    Yd, Yg = dev(pack(Ys)), dev(pack(Ys, poison=1e30))
    for x_anti in (0, 1):
        Xc = dev(pack(Xs if not x_anti else [a[0] for a in As]))
        Xg = dev(pack(Xs, poison=float("nan")) if not x_anti else pack([a[1] for a in As]))
        for alpha in (1.0, -1.0, 2.0):
            clean, dirty = raw_product(orb, Xc, x_anti, Yd, alpha), raw_product(orb, Xg, x_anti, Yg, alpha)
            assert same_bits(clean, dirty), (x_anti, alpha)
            for b, (m, got) in enumerate(zip(bt.ms, blocks(dirty, bt.ms))):
                ref = CR.product(Xs[b] if not x_anti else As[b][0], Ys[b], x_anti, alpha)
                assert same_values(got, ref) and structure_ok(got, x_anti), (x_anti, alpha, b, m)
                if m == 1:
                    assert got[0, 0] == 0.0


def test_product_bound_on_random_data_and_at_the_largest_size():
    bt = ragged(1, extra=[1024])
    rng = np.random.Generator(np.random.PCG64(2))
    Xs, Ys = [symmetric(rng, m) for m in bt.ms], [symmetric(rng, m) for m in bt.ms]
    As = [anti_operand(rng, m, garbage=float("nan")) for m in bt.ms]
    orb = state_of(bt)
    Yd = dev(pack(Ys, poison=float("nan")))
    worst = {}
    for x_anti, alpha in ((0, 1.0), (1, 1.0), (1, -1.0), (0, 2.0)):
        Xb = Xs if not x_anti else [a[0] for a in As]
        Xd = dev(pack(Xs, poison=float("nan")) if not x_anti else pack([a[1] for a in As]))
        got = blocks(raw_product(orb, Xd, x_anti, Yd, alpha), bt.ms)
        w, w1024 = 0.0, 0.0
        for b, m in enumerate(bt.ms):
            if m < 1024:
                Xl, Yl = ld(Xb[b]), ld(Ys[b])
                ref = (alpha * (Xl @ Yl - Yl @ Xl)).astype(np.float64)
            else:
                ref = alpha * (Xb[b] @ Ys[b] - Ys[b] @ Xb[b])
            f = worst_ratio(got[b], ref, CR.product_bound(Xb[b], Ys[b], x_anti, alpha))
            assert f <= 1.0 and structure_ok(got[b], x_anti), (x_anti, alpha, b, m, f)
            w, w1024 = (max(w, f), w1024) if m < 1024 else (w, f)
        worst[f"x_anti {x_anti} alpha {alpha:g}"] = (w, w1024)
    print("orbital_commutator_parity product worst error / bound (m <= 130 against extended precision; m = 1024 against float64 numpy): " +
          ", ".join(f"{k}: {v[0]:.3f}; {v[1]:.3f}" for k, v in worst.items()))


# ---- 2. the antisymmetric part and the norms ------------------------------------------------------------------------------------------------------------------------
def test_antisymmetrize_exactly_and_norms_within_the_summation_bound():
    bt = ragged(2)
    rng = np.random.Generator(np.random.PCG64(3))
    Gs = [general(rng, m) for m in bt.ms]
    orb = state_of(bt)
    Gd = dev(pack(Gs))
    got = blocks(raw_antisymmetrize(orb, Gd), bt.ms)
    for b, m in enumerate(bt.ms):
        assert same_bits(got[b], 0.5 * (Gs[b] - Gs[b].T)) and structure_ok(got[b], 0), (b, m)
    assert same_bits(orb.antisymmetrize(Gd).cpu().numpy(), pack(got))
    assert same_bits(orb.antisymmetrize(orb.antisymmetrize(Gd)).cpu().numpy(), pack(got))        # an antisymmetric matrix is its own antisymmetric part, bit for bit
    sumsq, top = raw_norms(orb, Gd)
    worst = 0.0
    for b, m in enumerate(bt.ms):
        ref = float((Gs[b] * Gs[b]).sum())
        f = abs(sumsq[b] - ref) / CR.norms_bound(Gs[b])
        worst = max(worst, f)
        assert f <= 1.0 and top[b] == np.abs(Gs[b]).max(), (b, m, f)
    s2, t2 = orb.commutator_norms(Gd)
    assert same_bits(s2.cpu().numpy(), sumsq) and same_bits(t2.cpu().numpy(), top)
    # a NaN entry is not dropped by the maximum
    Gn = [g.copy() for g in Gs]
    Gn[3][0, 0] = np.nan
    sn, tn = raw_norms(orb, dev(pack(Gn)))
    assert np.isnan(sn[3]) and np.isnan(tn[3]) and same_bits(np.delete(sn, 3), np.delete(sumsq, 3)) and same_bits(np.delete(tn, 3), np.delete(top, 3))
    bt2 = make_batch([1024], [[1024]])
    G = general(rng, 1024)
    s3, t3 = raw_norms(state_of(bt2), dev(pack([G])))
    f3 = abs(s3[0] - float((G * G).sum())) / CR.norms_bound(G)
    assert f3 <= 1.0 and t3[0] == np.abs(G).max()
    print(f"orbital_commutator_parity norms worst |sumsq - numpy| / (m^2 U sum R^2): {worst:.3g} (m <= 130), {f3:.3g} (m = 1024); the maximum is exact")


# ---- 3. run to run, the rest of the batch, a failed molecule, a dimension mismatch ---------------------------------------------------------------------------------------
def test_bitwise_reproducible_batch_independent_and_a_failed_molecule():
    ms = [17, 65, 130, 64]
    rng = np.random.Generator(np.random.PCG64(4))
    Xs, Ys, Gs = [symmetric(rng, m) for m in ms], [symmetric(rng, m) for m in ms], [general(rng, m) for m in ms]
    bad_status = torch.tensor([0, 0, 2, 0], dtype=torch.int32)

    def run(idx, fail=False):
        bt = make_batch([ms[i] for i in idx], [[ms[i]] for i in idx])
        orb = state_of(bt)
        if fail:
            orb.state.status.copy_(bad_status.to(DEV))
        Xd, Yd, Gd = (dev(pack([src[i] for i in idx])) for src in (Xs, Ys, Gs))
        Cm = orb.commutator(Xd, Yd)
        Ga = orb.antisymmetrize(Gd)
        gX, gY = orb.commutator(Ga, Yd, True, 1.0), orb.commutator(Ga, Xd, True, -1.0)
        sumsq, top = orb.commutator_norms(Cm)
        return [t.cpu().numpy() for t in (Cm, Ga, gX, gY)], [sumsq.cpu().numpy(), top.cpu().numpy()]
    every = list(range(len(ms)))
    packed, figs = run(every)
    packed2, figs2 = run(every)
    assert all(same_bits(x, y) for x, y in zip(packed + figs, packed2 + figs2))
    for b in (0, 1, 3):                                            # alone: the same bits as inside the batch
        pa, fa = run([b])
        for x, y in zip(pa, packed):
            assert same_bits(x.reshape(ms[b], ms[b]), blocks(y, ms)[b]), (b, ms[b])
        assert all(same_bits(x, y[b:b + 1]) for x, y in zip(fa, figs))
    packedf, figsf = run(every, fail=True)
    for b in every:
        own, was = [blocks(y, ms)[b] for y in packedf], [blocks(y, ms)[b] for y in packed]
        if b == 2:
            assert all(np.isnan(x).all() for x in own) and np.isnan(figsf[0][b]) and np.isnan(figsf[1][b])
        else:
            assert all(same_bits(x, y) for x, y in zip(own, was)) and figsf[0][b] == figs[0][b] and figsf[1][b] == figs[1][b], b


def test_dimension_mismatch_touches_nothing_and_python_refusals():
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import BatchedPurification
    bt = make_batch([5, 3], [[2, 3], [3]])
    orb = state_of(bt)
    st = orb.state
    lib = _lib.load()
    big, big2 = (torch.full((40,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2))
    src = torch.ones(40, dtype=torch.float64, device=DEV)
    for fn, args in ((lib.nq_orb_comm_product, (_lib.ptr(src), 0, _lib.ptr(src), 1.0, _lib.ptr(big))),
                     (lib.nq_orb_comm_product, (_lib.ptr(src), 1, _lib.ptr(src), -1.0, _lib.ptr(big))),
                     (lib.nq_orb_comm_antisymmetrize, (_lib.ptr(src), _lib.ptr(big))),
                     (lib.nq_orb_comm_norms, (_lib.ptr(src), _lib.ptr(big), _lib.ptr(big2)))):
        assert fn(_lib.ptr(st.buf), 2, 8, 36, *args, _lib.stream_ptr()) == 0, lib.nq_last_error()       # (2, 8, 36) instead of (2, 8, 34)
        torch.cuda.synchronize()
        assert int(st.header_dev[4]) == -2 and bool((big == SENTINEL).all()) and bool((big2 == SENTINEL).all())
        with pytest.raises(RuntimeError, match="other dimensions"):
            st.header()
        st.header_dev[4] = 0
    # aliased outputs and a symmetry that does not exist are refused on the host
    D = dev(pack([2.0 * np.eye(5), np.eye(3)]))
    X = dev(pack([np.diag(np.arange(5.0)), np.ones((3, 3))]))
    assert lib.nq_orb_comm_product(_lib.ptr(st.buf), *st._dims, _lib.ptr(X), 0, _lib.ptr(D), 1.0, _lib.ptr(X), _lib.stream_ptr()) != 0 and "operand" in lib.nq_last_error().decode()
    assert lib.nq_orb_comm_product(_lib.ptr(st.buf), *st._dims, _lib.ptr(X), 2, _lib.ptr(D), 1.0, _lib.ptr(big), _lib.stream_ptr()) != 0 and "neither 0" in lib.nq_last_error().decode()
    assert lib.nq_orb_comm_antisymmetrize(_lib.ptr(st.buf), *st._dims, _lib.ptr(X), _lib.ptr(X), _lib.stream_ptr()) != 0
    assert lib.nq_orb_comm_norms(_lib.ptr(st.buf), *st._dims, _lib.ptr(X), _lib.ptr(big), _lib.ptr(big), _lib.stream_ptr()) != 0 and "of their own" in lib.nq_last_error().decode()
    # the layout-only launches serve a purification state alike
    Cm = orb.commutator(X, D)
    pur = BatchedPurification(bt.op, DEV)
    pur.orthogonalize(dev(pack([np.eye(5), 4.0 * np.eye(3)])))
    assert same_bits(pur.commutator(X, D).cpu().numpy(), Cm.cpu().numpy()) and int(pur.state.header_dev[4]) == 0
    assert same_bits(nq.commutator(X, D, pur).cpu().numpy(), Cm.cpu().numpy())
    assert Cm.cpu().tolist() == [0.0] * 34                         # diagonal matrices and a multiple of the identity commute
    basis = nq.LowdinBasis.of(dev(pack([np.eye(5), 4.0 * np.eye(3)])), bt.op).check()
    with pytest.raises(ValueError, match="float64"):
        orb.commutator(D, D.float())
    with pytest.raises(ValueError, match="float64"):
        orb.antisymmetrize(D[:-1])
    with pytest.raises(ValueError, match="float64"):
        orb.commutator_norms(D.cpu())
    with pytest.raises(TypeError, match="basis must be a LowdinBasis"):
        nq.scf_residual(D, D, orb)
    with pytest.raises(ValueError, match="the basis packs"):
        nq.scf_residual(D[:-1], D, basis)
    with pytest.raises(TypeError, match="must be float64"):
        nq.commutator(D.float(), D, orb)
    with pytest.raises(ValueError, match="the batch packs"):
        nq.commutator(D[:-1], D, orb)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.scf_residual(D.cpu(), D, basis)
    with pytest.raises(ValueError, match="entries"):
        nq.ScfResidualLoss()(D[:-1], None, bt.op)
    assert float(nq.ScfResidualLoss("mse")(D, None, bt.op)) == 0.5 * (20.0 / 25.0 + 3.0 / 9.0)
    assert float(nq.ScfResidualLoss("mae")(D, D.clone(), bt.op)) == 0.0


# ---- 4. autograd of the commutator ------------------------------------------------------------------------------------------------------------------------------------
def test_commutator_autograd_against_torch(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals
    bt = ragged(3)
    rng = np.random.Generator(np.random.PCG64(5))
    Xs, Ys, Gs = [symmetric(rng, m) for m in bt.ms], [symmetric(rng, m) for m in bt.ms], [general(rng, m) for m in bt.ms]
    orb = state_of(bt)
    launches = []
    for name in ("commutator", "antisymmetrize"):
        real = getattr(BatchedOrbitals, name)
        monkeypatch.setattr(BatchedOrbitals, name, (lambda real, name: lambda self, *a, **k: (launches.append(name), real(self, *a, **k))[1])(real, name))
    X, Y = dev(pack(Xs)).requires_grad_(True), dev(pack(Ys)).requires_grad_(True)
    Gd = dev(pack(Gs))
    Cm = nq.commutator(X, Y, orb)
    assert launches == ["commutator"] and Cm.requires_grad and Cm.dtype == torch.float64 and Cm.shape == X.shape
    (Gd * Cm).sum().backward()
    assert launches == ["commutator", "antisymmetrize", "commutator", "commutator"]
    gX, gY = X.grad.clone(), Y.grad.clone()
    worst = [0.0, 0.0]
    for b, m in enumerate(bt.ms):
        Xt, Yt = torch.tensor(Xs[b], requires_grad=True), torch.tensor(Ys[b], requires_grad=True)
        (torch.from_numpy(Gs[b]) * CR.torch_commutator(Xt, Yt)).sum().backward()
        Ga = CR.antisymmetrize(Gs[b])
        for k, (got, ref, other) in enumerate(((gX, Xt.grad.numpy(), Ys[b]), (gY, Yt.grad.numpy(), Xs[b]))):
            gb = blocks(got.cpu().numpy(), bt.ms)[b]
            f = worst_ratio(gb, ref, CR.product_bound(Ga, other, 1, 1.0))
            worst[k] = max(worst[k], f)
            assert f <= 1.0 and same_bits(gb, gb.T), (k, b, m, f)
    print("orbital_commutator_parity autograd of the commutator worst error / bound against torch float64: dL/dX %.3f dL/dY %.3f" % tuple(worst))
    # the symmetric part of an upstream gradient cannot reach a commutator of symmetric matrices: G and its antisymmetric part give the same bits
    X.grad = Y.grad = None
    (orb.antisymmetrize(Gd) * nq.commutator(X, Y, orb)).sum().backward()
    assert same_bits(X.grad.cpu().numpy(), gX.cpu().numpy()) and same_bits(Y.grad.cpu().numpy(), gY.cpu().numpy())
    # a half nobody asks for is skipped; without an upstream gradient nothing is launched
    del launches[:]
    (Gd * nq.commutator(X, Y.detach(), orb)).sum().backward()
    assert launches == ["commutator", "antisymmetrize", "commutator"]
    del launches[:]
    X.grad = None
    Cm = nq.commutator(X, Y, orb)
    (2.0 * X).sum().backward()
    assert launches == ["commutator"] and bool((X.grad == 2.0).all())


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------------------------------------
KEYS = ("R", "gH", "gD", "gS")


def np_solution(H, S, n_occ):
    """-> (eps, C with the orbitals as columns, C^T S C = I, D = 2 C_o C_o^T)"""
    L = np.linalg.cholesky(S)
    w, Yv = np.linalg.eigh(LR.sym(np.linalg.solve(L, np.linalg.solve(L, H).T).T))
    Cc = np.linalg.solve(L.T, Yv)
    return w, Cc, 2.0 * Cc[:, :n_occ] @ Cc[:, :n_occ].T


def yardstick(H, D, S, G):
    Ht, Dt, St = (torch.tensor(a, requires_grad=True) for a in (H, D, S))
    Rt = CR.torch_scf_residual(Ht, Dt, St)
    ((torch.from_numpy(G) * Rt).sum() + 0.5 * (Rt * Rt).sum()).backward()
    return dict(R=Rt.detach().numpy(), gH=LR.sym(Ht.grad.numpy()), gD=LR.sym(Dt.grad.numpy()), gS=LR.sym(St.grad.numpy()))


def problems(which):
    """-> list of (tag, H_pred, S, D_target, n_occ): the prediction is the target Hamiltonian plus a symmetric perturbation of 2 % of its scale."""
    out = []
    if which == "synthetic":
        for case in [c for c in DR.CASES if c[1] < c[0]]:
            H, S = DR.gapped_case(*case)
            out.append((f"m={case[0]} n_occ={case[1]} kappa0={case[3]:g}", H, S, case[1], case[4]))
    else:
        import nabladft_amd as nq
        probs = db_problems()[:5]                                  # the sixth molecule's overlap is indefinite (tests/test_orbital_lowdin_gpu.py)
        for i, (H, S, z) in enumerate(probs):
            n_occ = int(nq.occupied_counts(np.asarray(z, dtype=np.int64), [0, len(z)], 0)[0])
            out.append((f"molecule {i} m={H.shape[0]} n_occ={n_occ}", H, S, n_occ, 800 + i))
    res = []
    for tag, H, S, n_occ, seed in out:
        rng = np.random.Generator(np.random.PCG64(seed))
        m = H.shape[0]
        Hp = H + 0.02 * np.abs(H).max() * LR.sym(rng.normal(size=(m, m)))
        res.append((tag, Hp, S, np_solution(H, S, n_occ)[2], n_occ, seed))
    return res


@functools.lru_cache(maxsize=None)
def reference(which):
    out = []
    for tag, H, S, D, n_occ, seed in problems(which):
        m = H.shape[0]
        rng = np.random.Generator(np.random.PCG64(9100 + seed))
        G = rng.normal(size=(m, m))
        s = np.linalg.eigvalsh(S)
        gap = LR.min_relative_gap(s)
        ref = yardstick(H, D, S, G)
        perm = rng.permutation(m)
        ix = np.ix_(perm, perm)
        back = {k: unpermute(v, ix) for k, v in yardstick(H[ix], D[ix], S[ix], G[ix]).items()}
        spread = {k: float(np.abs(ref[k] - back[k]).max()) for k in KEYS}
        kap = float(s.max() / s.min())
        A, Ai = LR.functions(S)[:2]
        HL, DL = LR.congruence(Ai, H)[0], LR.congruence(A, D)[0]
        Ga = np.abs(CR.antisymmetrize(G + ref["R"]))
        aH, aD, aA, aAi = np.abs(HL), np.abs(DL), np.abs(A), np.abs(Ai)
        unit = BOUND * m * E * kap
        floor = dict(R=unit * float((aH @ aD + aD @ aH).max()), gH=unit * float((aAi @ (Ga @ aD + aD @ Ga) @ aAi).max()),
                     gD=unit * float((aA @ (Ga @ aH + aH @ Ga) @ aA).max()), gS=unit * kap * float(np.abs(ref["gS"]).max()))
        out.append(SimpleNamespace(tag=tag, H=H, S=S, D=D, G=G, n_occ=n_occ, ref=ref, spread=spread, floor=floor, gap=gap, gap_ok=gap > m * 2.0 ** -40))
    return out


@pytest.mark.parametrize("which", ["synthetic", "database"])
def test_scf_residual_end_to_end(which):
    import nabladft_amd as nq
    refs = reference(which)
    if which == "synthetic":
        assert all(r.gap_ok for r in refs)                        # the backward of eigh divides by the gaps of s, which must be resolved
    ms = [r.H.shape[0] for r in refs]
    bt = make_batch(ms, [[m] for m in ms])
    H, D, S = (dev(pack([getattr(r, n) for r in refs])).requires_grad_(True) for n in "HDS")
    basis = nq.lowdin_basis(S, bt.op)
    Rm = nq.scf_residual(H, D, basis)
    assert Rm.dtype == torch.float64 and Rm.requires_grad and Rm.numel() == int(bt.pp[-1])
    Gd = dev(pack([r.G for r in refs]))
    ((Gd * Rm).sum() + 0.5 * (Rm * Rm).sum()).backward()
    basis.check()
    got_all = dict(R=blocks(Rm.detach().cpu().numpy(), ms), gH=blocks(H.grad.cpu().numpy(), ms), gD=blocks(D.grad.cpu().numpy(), ms), gS=blocks(S.grad.cpu().numpy(), ms))
    sumsq, top = basis.orbitals.commutator_norms(Rm.detach())
    for b, r in enumerate(refs):
        got = {k: got_all[k][b] for k in KEYS}
        assert structure_ok(got["R"], 0) and all(same_bits(got[k], got[k].T) for k in ("gH", "gD", "gS")), r.tag
        assert abs(float(sumsq[b]) - float((got["R"] ** 2).sum())) <= CR.norms_bound(got["R"]) and float(top[b]) == np.abs(got["R"]).max()
        keys = [k for k in KEYS if k != "gS" or r.gap_ok]
        line = []
        for k in keys:
            err, allow = float(np.abs(got[k] - r.ref[k]).max()), max(10.0 * r.spread[k], r.floor[k])
            line.append(f"{k} {err / max(allow, TINY):.3g} of the allowance ({err / max(r.spread[k], TINY):.3g} spreads; allowance {allow / max(r.spread[k], TINY):.3g} spreads)")
        skipped = "" if r.gap_ok else f"; gS not compared: the levels of S are not resolved for the backward of eigh (min gap {r.gap:.2g})"
        print(f"orbital_commutator_parity end-to-end {which} {r.tag} min gap of s {r.gap:.2g}: " + "; ".join(line) + skipped)
        for k in keys:
            assert np.isfinite(got[k]).all() and float(np.abs(got[k] - r.ref[k]).max()) <= max(10.0 * r.spread[k], r.floor[k]), (r.tag, k)
        if not r.gap_ok:
            assert np.isfinite(got["gS"]).all(), r.tag


def residual_bound(H, S, D, n_occ, eps):
    """The chain bound of the module text for R^L of one molecule -> (bound [m, m], HL, DL)."""
    m = H.shape[0]
    prop = propagated(H, S, D, np.array([0, m]), n_occ, eps)
    A, Ai = LR.functions(S)[:2]
    HL, DL = LR.congruence(Ai, H)[0], LR.congruence(A, D)[0]
    aH, aD = np.abs(HL), np.abs(DL)
    return CR.product_bound(HL, DL) + prop["HL"] @ aD + aH @ prop["DL"] + aD @ prop["HL"] + prop["DL"] @ aH, HL, DL


def test_own_density_is_stationary_and_the_occupied_virtual_identity():
    """``orbital_solution``'s own (H, D) has a residual of zero within the bound of the chain; for another H the sum of squares is 8 sum_ia h_ia^2 with
    h_ia = c_i^T H c_a over the SOLVER's coefficients (S^(-1/2) and S^(1/2) cancel between H^L and the Löwdin orbitals).  Allowance of the identity: the residual's
    chain bound carried into the sum, 2 |R| dR + dR^2 summed, plus 10 m E kappa of the closed form for the coefficients and the norm's own summation bound."""
    import nabladft_amd as nq
    cases = [c for c in DR.CASES if c[1] < c[0]]
    pairs = [DR.gapped_case(*c) for c in cases]
    Hs, Ss, nos = [p[0] for p in pairs], [p[1] for p in pairs], [c[1] for c in cases]
    ms = [h.shape[0] for h in Hs]
    bt = make_batch(ms, [[m] for m in ms])
    Hd, Sd = dev(pack(Hs)), dev(pack(Ss))
    eps, D, sol = nq.orbital_solution(Hd, Sd, bt.op, nos, return_solution=True)
    basis = nq.LowdinBasis.of(Sd, bt.op).check()
    sol.check()
    R0 = blocks(nq.scf_residual(Hd, D, basis).cpu().numpy(), ms)
    rng = np.random.Generator(np.random.PCG64(12))
    H2s = [h + 0.05 * np.abs(h).max() * symmetric(rng, h.shape[0]) for h in Hs]
    R2 = nq.scf_residual(dev(pack(H2s)), D, basis)
    sumsq = basis.orbitals.commutator_norms(R2)[0].cpu().numpy()
    R2b, Db, epsn = blocks(R2.cpu().numpy(), ms), blocks(D.cpu().numpy(), ms), eps.cpu().numpy()
    Cts = blocks(sol.coefficients.cpu().numpy(), ms)              # row k = orbital k
    for b, m in enumerate(ms):
        e_b = epsn[int(bt.op[b]):int(bt.op[b + 1])]
        bound, HL, DL = residual_bound(Hs[b], Ss[b], Db[b], nos[b], e_b)
        f0 = worst_ratio(R0[b], np.zeros((m, m)), bound + TINY)
        h = Cts[b][:nos[b]] @ H2s[b] @ Cts[b][nos[b]:].T
        want = 8.0 * float((h * h).sum())
        dR = residual_bound(H2s[b], Ss[b], Db[b], nos[b], e_b)[0]
        kap = float(np.linalg.cond(Ss[b]))
        allow = float((2.0 * np.abs(R2b[b]) * dR + dR * dR).sum()) + BOUND * m * E * kap * want + CR.norms_bound(R2b[b])
        f1 = abs(sumsq[b] - want) / max(allow, TINY)
        print(f"orbital_commutator_parity stationary m={m} n_occ={nos[b]}: |R| of the solver's own density / chain bound {f0:.3g} (max |R| {np.abs(R0[b]).max():.3g}); "
              f"|sumsq - 8 sum h_ia^2| / allowance {f1:.3g} (sumsq {sumsq[b]:.6g})")
        assert f0 <= 1.0 and f1 <= 1.0 and (m == 1 or want > 0.0), (b, m, f0, f1)


def test_closed_and_crossed_gaps_give_finite_residuals_and_gradients():
    """Predictions built in the target's orbitals, H = S C (diag(e) + V) C^T S with a small occupied-virtual coupling V: HOMO and LUMO coincident, then crossed.
    The closed form in those orbitals (P = the occupied projector, M = diag(e) + V): R^L = 2 Q [M, P] Q^T with Q = S^(1/2) C, and for L = 1/2 |R^L|^2:
    dL/dH = C [R_mo, 2 P] C^T with R_mo = 2 [M, P].  Allowance: 10 m E kappa of the magnitude of each quantity's own sums (the floor of the end-to-end test).
    ``orbital_solution`` on the same predictions is printed beside it: its response divides by eps_i - eps_a."""
    import nabladft_amd as nq
    m, n_occ = 17, 5
    Ht, S = DR.gapped_case(m, n_occ, 0.3, 1e2, 57)
    w, Cc, Dt = np_solution(Ht, S, n_occ)
    rng = np.random.Generator(np.random.PCG64(13))
    V = np.zeros((m, m))
    V[:n_occ, n_occ:] = 0.05 * rng.normal(size=(n_occ, m - n_occ))
    V = V + V.T
    Pm = np.diag((np.arange(m) < n_occ).astype(np.float64))
    preds, Ms = [], []
    for name in ("coincident", "crossed"):
        e = w.copy()
        if name == "coincident":
            e[n_occ] = e[n_occ - 1]
        else:
            e[n_occ - 1], e[n_occ] = w[n_occ], w[n_occ - 1]
        M = np.diag(e) + V
        SC = S @ Cc
        preds.append(LR.sym(SC @ M @ SC.T))
        Ms.append(M)
    op = np.array([0, m, 2 * m])
    H = dev(pack(preds)).requires_grad_(True)
    Sd, Dd = dev(pack([S, S])), dev(pack([Dt, Dt]))
    basis = nq.LowdinBasis.of(Sd, op).check()
    Rm = nq.scf_residual(H, Dd, basis)
    (0.5 * (Rm * Rm).sum()).backward()
    A = LR.functions(S)[0]
    Q = A @ Cc
    kap = float(np.linalg.cond(S))
    Rb, gb = blocks(Rm.detach().cpu().numpy(), [m, m]), blocks(H.grad.cpu().numpy(), [m, m])
    H2 = dev(pack(preds)).requires_grad_(True)
    eps2, D2 = nq.orbital_solution(H2, Sd, op, [n_occ, n_occ])
    (0.5 * ((D2 - Dd) ** 2).sum()).backward()
    g2 = blocks(H2.grad.cpu().numpy(), [m, m])
    for b, name in enumerate(("coincident", "crossed")):
        M = Ms[b]
        Rmo = 2.0 * (M @ Pm - Pm @ M)
        Rref = Q @ Rmo @ Q.T
        gref = Cc @ (2.0 * (Rmo @ Pm - Pm @ Rmo)) @ Cc.T
        aQ, aC = np.abs(Q), np.abs(Cc)
        allow_R = BOUND * m * E * kap * float((aQ @ (2.0 * (np.abs(M) @ Pm + Pm @ np.abs(M))) @ aQ.T).max())
        allow_g = BOUND * m * E * kap * float((aC @ (2.0 * (np.abs(Rmo) @ Pm + Pm @ np.abs(Rmo))) @ aC.T).max())
        eR, eg = float(np.abs(Rb[b] - Rref).max()), float(np.abs(gb[b] - gref).max())
        contrast = "finite, largest entry %.3g" % np.abs(g2[b]).max() if np.isfinite(g2[b]).all() else "NOT finite"
        print(f"orbital_commutator_parity gap safety {name} HOMO/LUMO: |R - closed form| / allowance {eR / allow_R:.3g}, |dL/dH - closed form| / allowance {eg / allow_g:.3g}, "
              f"largest |dL/dH| {np.abs(gb[b]).max():.3g}; orbital_solution's density-loss gradient on the same prediction: {contrast}")
        assert np.isfinite(Rb[b]).all() and np.isfinite(gb[b]).all() and eR <= allow_R and eg <= allow_g and np.abs(gref).max() > 0.0, (name, eR, eg)


# ---- 6. the errors of a test loop ---------------------------------------------------------------------------------------------------------------------------------------
def test_scf_residual_errors_against_the_restatement_with_a_failed_molecule():
    """The database batch first (its sixth overlap is indefinite: counted and left out), then a synthetic batch.  The root mean square and the maximum are
    1-Lipschitz in the largest entry of R, so each figure may differ from the restatement's by the mean over the molecules of the chain bound's largest entry."""
    import nabladft_amd as nq
    from nabladft_amd.orbitals import ScfResidualErrors
    probs = db_problems()
    z_all = [np.asarray(p[2], dtype=np.int64) for p in probs]
    batches = [[(p[0], p[1], int(nq.occupied_counts(z, [0, len(z)], 0)[0])) for p, z in zip(probs, z_all)],
               [DR.gapped_case(*c) + (c[1],) for c in DR.CASES if c[1] < c[0] and c[0] in (3, 17, 65)]]
    acc = ScfResidualErrors()
    rng = np.random.Generator(np.random.PCG64(14))
    Rs, slack = [], []
    for i, batch in enumerate(batches):
        ms = [h.shape[0] for h, _, _ in batch]
        op = np.concatenate([[0], np.cumsum(ms)])
        Hp = [h + 0.02 * np.abs(h).max() * symmetric(rng, h.shape[0]) for h, _, _ in batch]
        nos = [n for _, _, n in batch]
        target = nq.scf_target(dev(pack([h for h, _, _ in batch])), dev(pack([s for _, s, _ in batch])), op, nos)
        assert isinstance(target, nq.ScfTarget) and not target.DL.requires_grad and target.basis.info.cpu().tolist() == ([0, 0, 0, 0, 0, 1] if i == 0 else [0] * len(ms))
        assert acc.update(dev(pack(Hp)), target) is acc
        DLs = blocks(target.DL.cpu().numpy(), ms)
        for b, (h, s, n) in enumerate(batch):
            if i == 0 and b == 5:
                assert np.isnan(DLs[b]).all()
                Rs.append(np.full((ms[b], ms[b]), np.nan))
                continue
            eps, _, Dn = np_solution(h, s, n)
            Rs.append(CR.scf_residual(Hp[b], Dn, s)[0])
            slack.append(float(residual_bound(Hp[b], s, Dn, n, eps)[0].max()))
    got, want = acc.compute(), CR.errors(Rs)
    tol = float(np.mean(slack))
    print(f"orbital_commutator_parity errors: rms {got['scf_residual_rms']:.6g} (restatement {want['scf_residual_rms']:.6g}), max {got['scf_residual_max']:.6g} "
          f"({want['scf_residual_max']:.6g}), molecules {got['molecules']}, failed {got['failed']}; allowance {tol:.3g}")
    assert got["failed"] == want["failed"] == 1 and got["molecules"] == want["molecules"] == 8
    assert abs(got["scf_residual_rms"] - want["scf_residual_rms"]) <= tol and abs(got["scf_residual_max"] - want["scf_residual_max"]) <= tol
    acc.reset()
    with pytest.raises(RuntimeError, match="before any update"):
        acc.compute()


# ---- 7. the QHNet task ------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_commutator_task(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from nabladft_amd.orbitals import OrbitalState
    from test_qhnet_gpu import ORBITALS, load_case
    g, cfg, net, batch = load_case("small", torch.device(DEV))
    per_atom = np.array([sum(2 * l + 1 for l in ORBITALS[int(a)]) for a in g["z"]])
    ends = np.cumsum(g["sizes"])
    batch.hamiltonian, batch.overlap, o = [], [], 0
    rng = np.random.Generator(np.random.PCG64(6))
    ms = [int(per_atom[e - n:e].sum()) for n, e in zip(g["sizes"], ends)]
    for m in ms:
        batch.hamiltonian.append(g["target"][o:o + m, o:o + m].astype(np.float32))
        A = rng.normal(size=(m, m)) * 0.1 / np.sqrt(m)
        batch.overlap.append((np.eye(m) + A + A.T).astype(np.float32))       # a well conditioned overlap
        o += m
    charge = [0, -1, 1]                                           # the fixture's molecules hold 92, 9 and 31 electrons: closed shells as anion and cation
    base = {"hamiltonian": HamiltonianLoss(), "lowdin_charges": nq.LowdinChargeLoss("mse", charge)}
    base_c = {"hamiltonian": 1.0, "lowdin_charges": 0.0}
    losses = dict(base, scf_residual=nq.ScfResidualLoss("mse", charge))
    coefs = dict(base_c, scf_residual=0.7)
    make = lambda cls, ls, cs: cls("QHNet", net, None, None, ls, None, None, cs)
    solves = []                                                   # per solve: does its matrix carry a gradient (the prediction does, targets and overlaps do not)
    real = OrbitalState.solve
    monkeypatch.setattr(OrbitalState, "solve", lambda self, H, *a, **k: (solves.append(bool(H.requires_grad)), real(self, H, *a, **k))[1])
    params = [p for p in net.parameters() if p.requires_grad]

    def step(task):
        for p in params:
            p.grad = None
        loss = task.training_step(batch, 0)
        loss.backward()
        return loss.detach(), [None if p.grad is None else p.grad.detach().clone() for p in params]
    task = make(nq.QHNetCommutatorLightning, losses, coefs)
    loss, grads = step(task)
    assert solves == [False, False], solves                       # the decomposition of S and the target: NO solve of the prediction
    assert bool(torch.isfinite(loss)) and all(gr is None or bool(torch.isfinite(gr).all()) for gr in grads)
    assert any(gr is not None and bool((gr != 0).any()) for gr in grads)
    preds, targets, _ = task._evaluate(batch)
    Rp = preds["scf_residual"]
    assert targets["scf_residual"] is None and Rp.requires_grad and Rp.numel() == sum(m * m for m in ms) and bool(torch.isfinite(Rp).all())
    term = losses["scf_residual"](Rp, None, *preds["scf_residual_args"]).detach()
    by_hand = np.mean([(r ** 2).mean() for r in blocks(Rp.detach().cpu().numpy(), ms)])
    assert float(term) > 0.0 and abs(float(term) - by_hand) <= 1e-12 * by_hand
    # the parent without the key, and the coefficient at 0: QHNetLowdinLightning's step bit for bit, nothing solved
    del solves[:]
    parent = make(nq.QHNetLowdinLightning, base, base_c)
    loss_p, grads_p = step(parent)
    zero = make(nq.QHNetCommutatorLightning, losses, dict(coefs, scf_residual=0.0))
    loss_z, grads_z = step(zero)
    nokey = make(nq.QHNetCommutatorLightning, base, base_c)
    loss_n, grads_n = step(nokey)
    assert solves == []
    for l2, g2 in ((loss_z, grads_z), (loss_n, grads_n)):
        assert l2.dtype == loss_p.dtype and torch.equal(l2, loss_p) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g2, grads_p))
    assert torch.allclose((loss - loss_p).double(), 0.7 * term.double(), rtol=1e-4, atol=1e-6 * float(loss.abs()))
    # the cached batch fields: no solve at all, the same residual as the uncached step within float32 packing of the overlap (here: the same bits, the
    # cached matrices ARE what the uncached step computed)
    plan, asm = net.last_plan, net._asm
    op = np.concatenate([[0], np.cumsum(ms)])
    n_occ = nq.occupied_counts(batch.z, batch.ptr, charge, op)
    target = nq.scf_target(asm.pack_targets(plan, batch.hamiltonian), asm.pack_targets(plan, batch.overlap), op, n_occ)
    batch.lowdin_inv_half, batch.lowdin_half = blocks(target.basis.inv_half.cpu().numpy(), ms), blocks(target.basis.half.cpu().numpy(), ms)
    batch.target_density_lowdin = blocks(target.DL.cpu().numpy(), ms)
    del solves[:]
    loss_c, grads_c = step(task)
    assert solves == [], solves
    assert torch.equal(loss_c, loss) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads_c, grads))
    # the loss vanishes when the prediction is the target: the residual of the target's own Hamiltonian, within the chain's rounding
    Ht = asm.pack_targets(plan, batch.hamiltonian).double()
    R0 = nq.scf_residual_to_target(Ht, target)
    at_target = float(nq.ScfResidualLoss("mse")(R0, None, op))
    chain = []                                                    # the mean of squares is at most the square of the largest entry, which the chain bound holds
    for b, m in enumerate(ms):
        h, s = LR.lower_sym(batch.hamiltonian[b].astype(np.float64)), LR.lower_sym(batch.overlap[b].astype(np.float64))
        eps_b, _, Dn = np_solution(h, s, int(n_occ[b]))
        chain.append(float(residual_bound(h, s, Dn, int(n_occ[b]), eps_b)[0].max()) ** 2)
    print(f"orbital_commutator_parity qhnet task loss {float(loss):.9g} parent {float(loss_p):.9g} residual term {float(term):.6g}; the term at prediction = target "
          f"{at_target:.3g} (allowed {float(np.mean(chain)):.3g})")
    assert at_target <= float(np.mean(chain)) < float(term)
    # beside another orbital key the parent's step runs as it is and the term is added
    del solves[:]
    both = make(nq.QHNetCommutatorLightning, losses, dict(coefs, lowdin_charges=1.5))
    loss_b, _ = step(both)
    par_b = make(nq.QHNetLowdinLightning, base, dict(base_c, lowdin_charges=1.5))
    n_both = len(solves)
    loss_pb, _ = step(par_b)
    assert n_both == len(solves) - n_both == 3 and solves.count(True) == 2          # cached fields: the residual term adds no solve to the parent's three
    assert torch.allclose((loss_b - loss_pb).double(), 0.7 * term.double(), rtol=1e-4, atol=1e-6 * float(loss_b.abs()))
    batch.lowdin_half = None
    overlap, batch.overlap = batch.overlap, None
    with pytest.raises(ValueError, match="needs batch.overlap"):
        task.training_step(batch, 0)
    batch.overlap = overlap
