"""GPU: the purification kernels (csrc/orbpurify.hip) through the C ABI and through ``BatchedPurification`` / ``purified_density_matrix`` /
``QHNetPurifiedDensityLightning``, against the numpy restatement (tests/orbital_purify_ref.py) and the float64 yardsticks of the solver route
(tests/orbitals_ref.py, tests/orbital_density_ref.py), and against ``orbital_solution`` itself.

Bounds.  Orthogonaliser: |Z - Z_ref| <= 10 m 2^-52 kappa_2(S) max|Z| against ``np.linalg.cholesky`` + inverse.  Every product against numpy on the same
operands: |x - ref| <= (K + 4) 2^-53 sum |terms| with K the number of terms (the bound of tests/test_orbital_density_gpu.py), and bit for bit on small
integers (the sign of a zero aside).  End to end: D within 10 U_D, U_D = m 2^-52 kappa_2(S) (eps_max - eps_min) / (eps_LUMO - eps_HOMO) max|D| (gap factor 1 when n_occ = m), gH / gS
within 10 ``orbital_density_ref.units`` of ``closed_form``; ten is the project's standing margin for these units (test_orbitals_gpu.BOUND).  Tr(D S) = 2 n_occ
within 10 m 2^-52 kappa_2(S) 2 n_occ: Tr(D S) = 2 Tr(X Z S Z^T) and Z S Z^T = I to m 2^-52 kappa_2(S), tr X = n_occ to a few 2^-52 n_occ.  Two routes that
are each within 10 units of the truth are compared with each other within the same 10 units (the issue's yardstick); measured: 0.04 / 0.04 / 0.07 (D, gH, gS); against the yardstick 1.5 (D, m = 3) / 0.95 / 0.42.
Float32 results are allowed their own rounding, 2^-24 per element.  Every figure is printed as an ``orbital_purify_parity ...`` line (kept in
profiles/orbital_purify_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_purify_ref as PR
import orbitals_ref as R
from test_orbital_loss_gpu import blocks, db_plan
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, ptrs, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 17, 63, 64, 65, 127, 128, 129, 130]
SENTINEL = -7.25e300
GUARD = 64
U = 2.0 ** -53


def purification(ms):
    from nabladft_amd.orbitals import BatchedPurification
    op = np.concatenate([[0], np.cumsum(ms)])
    return BatchedPurification(op, DEV), op


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def unguard(buf, name, full=True):
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), name
    if full:
        assert not np.any(h[GUARD:-GUARD] == SENTINEL), name
    return h[GUARD:-GUARD].copy()


def call(name, st, *args):
    from nabladft_amd import _lib
    rc = getattr(_lib.load(), name)(_lib.ptr(st.buf), *st._dims, *args, _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()


def raw_congruence(pur, Z, A, trans, alpha=1.0, sym=False):
    """``nq_orb_pur_congruence`` into guarded buffers -> (tmp, out) numpy; Z None: tmp None."""
    from nabladft_amd import _lib
    P = pur.state.P
    At = dev(A)
    Zt = None if Z is None else dev(Z)
    bt, tmp = guarded(P)
    bo, out = guarded(P)
    call("nq_orb_pur_congruence", pur.state, _lib.ptr(Zt), int(trans), _lib.ptr(At), int(At.dtype == torch.float64), int(sym), float(alpha),
         _lib.ptr(tmp if Z is not None else None), _lib.ptr(out))
    return (None if Z is None else unguard(bt, "tmp")), unguard(bo, "out")


def raw_gemm(pur, A, Bm, C, alpha, beta):
    from nabladft_amd import _lib
    bo, out = guarded(pur.state.P)
    ts = [dev(A), dev(Bm), None if C is None else dev(C)]
    call("nq_orb_pur_gemm", pur.state, *[_lib.ptr(t) for t in ts], float(alpha), float(beta), _lib.ptr(out))
    return unguard(bo, "gemm")


def same_values(a, b):
    """Bit for bit, except that -0.0 and 0.0 are the same number (alpha * 0 carries alpha's sign)."""
    return same_bits(np.asarray(a) + 0.0, np.asarray(b) + 0.0)


def worst_ratio(got, ref, bound):
    err = np.abs(got - ref)
    assert np.all(err[bound == 0.0] == 0.0)
    return float((err[bound > 0.0] / bound[bound > 0.0]).max()) if np.any(bound > 0.0) else 0.0


def lower_tri(rng, m, integers=False):
    Z = np.tril(rng.integers(1, 4, size=(m, m)).astype(np.float64) * rng.choice([-1.0, 1.0], size=(m, m)) if integers else rng.normal(size=(m, m)))
    return Z


def symmetric(rng, m, integers=False):
    A = rng.integers(-3, 4, size=(m, m)).astype(np.float64) if integers else rng.normal(size=(m, m))
    return np.tril(A) + np.tril(A, -1).T


# ---- 1. the orthogonaliser ---------------------------------------------------------------------------------------------------------------------------------------
def test_orthogonalizer_against_numpy_and_a_failed_molecule():
    rng = np.random.Generator(np.random.PCG64(1))
    order = rng.permutation(len(SIZES))
    ms = [SIZES[i] for i in order] + [17]
    Ss = [DR.overlap(m, 1e2, rng) for m in ms]
    w, V = np.linalg.eigh(Ss[-1])
    w[3] = -0.25
    Ss[-1] = (V * w[None, :]) @ V.T                                  # not positive definite
    Ss[-1] = 0.5 * (Ss[-1] + Ss[-1].T)
    bad = len(ms) - 1
    worst = 0.0
    for dt in (np.float64, np.float32):
        S_ = [s.astype(dt).astype(np.float64) for s in Ss]
        pur, op = purification(ms)
        orth = pur.orthogonalize(dev(pack(S_, dt, poison=1e30)))     # the upper triangles are never read
        Zs = blocks(orth.Z.cpu().numpy(), ms)
        status, info = orth.status.cpu().numpy(), orth.info.cpu().numpy()
        assert status[bad] == 1 and np.all(status[:bad] == 0) and np.isnan(Zs[bad]).all()
        L = np.tril(S_[bad]).copy()                                  # the pivot the restated elimination meets first
        fail = 0
        for j in range(17):
            if not L[j, j] > 0.0:
                fail = j + 1
                break
            L[j:, j] /= np.sqrt(L[j, j])
            for k in range(j + 1, 17):
                L[k:, k] -= L[k:, j] * L[k, j]
        assert info[bad] == fail and fail > 0
        with pytest.raises(RuntimeError, match=f"molecule {bad}: the overlap matrix is not positive definite"):
            pur.check()
        for b, m in enumerate(ms[:bad]):
            ref = PR.orthogonalizer(S_[b])
            assert np.all(np.triu(Zs[b], 1) == 0.0) and not np.signbit(np.triu(Zs[b], 1)).any()
            bound = 10.0 * m * R.EPS * np.linalg.cond(S_[b]) * np.abs(ref).max()
            fig = float(np.abs(Zs[b] - ref).max() / bound)
            worst = max(worst, fig)
            assert fig <= 1.0, (b, m, fig)
    print(f"orbital_purify_parity orthogonalizer worst |Z - Z_ref| / (10 m eps kappa max|Z|) {worst:.3g}")


# ---- 2. the products -------------------------------------------------------------------------------------------------------------------------------------------------
def product_batch(seed, integers, ms=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    ms = [SIZES[i] for i in rng.permutation(len(SIZES))] if ms is None else ms
    return ms, [lower_tri(rng, m, integers) for m in ms], [symmetric(rng, m, integers) for m in ms], rng


def start_step(pur, ms, Xs, nos, max_iter=4):
    """A state whose X is written directly: ``prepare`` on a harmless H (which leaves kind = 0 for m >= 2), then X overwritten."""
    Hs = [np.diag(np.arange(m, dtype=np.float64)) for m in ms]
    pur.prepare(dev(pack(Hs)), nos, max_iter)
    pur.state.coeff.copy_(dev(pack(Xs)))


def check_step(pur, ms, Xs, nos, exact, tag):
    """One SP2 step on the X written into the state: Y, the slots, the traces, the log and the updated X against the restatement."""
    pur.step(0)
    st = pur.state
    Y, Xn = blocks(st.chol.cpu().numpy(), ms), blocks(st.coeff.cpu().numpy(), ms)
    ctl, log, iters = pur.ctl.cpu().numpy(), pur.log.cpu().numpy(), st.iters.cpu().numpy()
    worst = 0.0
    for b, m in enumerate(ms):
        if m == 1:                                                   # e_max = e_min: X = I, no iteration
            assert ctl[b, 2] == 2.0 and log[b, 0] == 0 and iters[b] == 0 and same_bits(Xn[b], Xs[b])   # kind 2 (X = I): untouched by the step
            continue
        X = Xs[b]
        ref = X @ X
        assert np.array_equal(Y[b], Y[b].T)
        if exact:
            assert same_values(Y[b], ref), (tag, b, m)
        else:
            fig = worst_ratio(Y[b], ref, (m + 4) * U * (np.abs(X) @ np.abs(X)))
            worst = max(worst, fig)
            assert fig <= 1.0, (tag, b, m, fig)
        nd = (m + 63) // 64
        for d in range(nd):                                          # the partial traces of the diagonal tiles
            sl = slice(64 * d, min(m, 64 * d + 64))
            tx, ty = np.diag(X)[sl], np.diag(Y[b])[sl]
            for got, part in ((ctl[b, 8 + 2 * d], tx), (ctl[b, 9 + 2 * d], ty)):
                assert abs(got - part.sum()) <= (64 + 4) * U * np.abs(part).sum(), (tag, b, m, d)
        assert np.all(ctl[b, 8 + 2 * nd:40] == 0.0)
        t = t2 = 0.0
        for d in range(nd):                                          # the slots in slot order
            t, t2 = t + ctl[b, 8 + 2 * d], t2 + ctl[b, 9 + 2 * d]
        assert ctl[b, 4] == t and ctl[b, 5] == t2 and ctl[b, 40] == t - t2
        n = nos[b]
        entry = PR.STOPPED if t - t2 == 0.0 else (1 if abs(t2 - n) <= abs(2.0 * t - t2 - n) else 2)      # the rule on the device's own traces
        assert log[b, 0] == entry and iters[b] == (0 if entry == PR.STOPPED else 1), (tag, b, m)
        want = X if entry == PR.STOPPED else (Y[b] if entry == 1 else 2.0 * X - Y[b])
        assert same_values(Xn[b], want), (tag, b, m)
    return worst


def test_exact_placement_with_small_integers():
    """Small integers in every operand: all products and sums are exact in float64, so lane maps, tile offsets, the cut contraction ranges and the mirror
    are compared with numpy bit for bit.  Z and the second operands are NOT symmetric, A is."""
    ms, Zs, As, rng = product_batch(2, True)
    pur, op = purification(ms)
    for trans in (False, True):
        tmp, out = raw_congruence(pur, pack(Zs), pack(As), trans, alpha=-2.0)
        for b, m in enumerate(ms):
            Z, A = Zs[b], As[b]
            T = A @ Z if trans else A @ Z.T
            full = -2.0 * (Z.T @ T if trans else Z @ T)
            assert same_values(blocks(tmp, ms)[b], T) and same_values(blocks(out, ms)[b], PR.lower_sym(full)), (trans, b, m)
    Ns = [rng.integers(-3, 4, size=(m, m)).astype(np.float64) for m in ms]              # the loader: lower triangle mirrored, or the symmetric part
    _, lo = raw_congruence(pur, None, pack(Ns), False, alpha=3.0)
    _, sy = raw_congruence(pur, None, pack(Ns), False, alpha=2.0, sym=True)
    Bs, Cs = [rng.integers(-3, 4, size=(m, m)).astype(np.float64) for m in ms], [rng.integers(-3, 4, size=(m, m)).astype(np.float64) for m in ms]
    g1, g0 = raw_gemm(pur, pack(Ns), pack(Bs), pack(Cs), 2.0, -1.0), raw_gemm(pur, pack(Ns), pack(Bs), None, 1.0, 5.0)
    for b, m in enumerate(ms):
        assert same_values(blocks(lo, ms)[b], 3.0 * PR.lower_sym(Ns[b])) and same_values(blocks(sy, ms)[b], Ns[b] + Ns[b].T)
        assert same_values(blocks(g1, ms)[b], 2.0 * (Ns[b] @ Bs[b]) - Cs[b]) and same_values(blocks(g0, ms)[b], Ns[b] @ Bs[b]), (b, m)
    nos = [max(1, m // 3) for m in ms]
    start_step(pur, ms, As, nos)
    check_step(pur, ms, As, nos, True, "integers")
    # the response step from the same X: Y again, Q = X1 X + X X1, and the update by the logged branch
    X1s = [symmetric(rng, m, True) for m in ms]
    Gt, X1, Q = pur.response_start(dev(pack(As)))
    pur.state.coeff.copy_(dev(pack(As)))
    X1.copy_(dev(pack(X1s)))
    pur.response_step(0, X1, Q)
    log = pur.log.cpu().numpy()
    Y, Xn, Qn, X1n = (blocks(t.cpu().numpy(), ms) for t in (pur.state.chol, pur.state.coeff, Q, X1))
    for b, m in enumerate(ms):
        if m == 1:
            continue
        X, A1 = As[b], X1s[b]
        q = A1 @ X + X @ A1
        assert same_values(Y[b], X @ X) and same_values(Qn[b], q), (b, m)
        assert log[b, 0] in (1, 2)
        assert same_values(Xn[b], X @ X if log[b, 0] == 1 else 2.0 * X - X @ X) and same_values(X1n[b], q if log[b, 0] == 1 else 2.0 * A1 - q)


def test_product_bounds_on_the_ragged_batch():
    ms, Zs, As, rng = product_batch(3, False)
    pur, op = purification(ms)
    worst = np.zeros(5)
    for trans in (False, True):
        tmp, out = raw_congruence(pur, pack(Zs), pack(As), trans)
        for b, m in enumerate(ms):
            Z, A, T = Zs[b], As[b], blocks(tmp, ms)[b]
            Zop = Z if trans else Z.T
            f1 = worst_ratio(T, (A.astype(np.longdouble) @ Zop.astype(np.longdouble)).astype(np.float64), (m + 4) * U * (np.abs(A) @ np.abs(Zop)))
            Zl = Z.T if trans else Z
            ref = (Zl.astype(np.longdouble) @ T.astype(np.longdouble)).astype(np.float64)
            got = blocks(out, ms)[b]
            assert np.array_equal(got, got.T)
            f2 = worst_ratio(np.tril(got), np.tril(ref), np.tril((m + 4) * U * (np.abs(Zl) @ np.abs(T))))
            worst[:2] = np.maximum(worst[:2], [f1, f2])
            assert f1 <= 1.0 and f2 <= 1.0, (trans, b, m, f1, f2)
    Bs = [rng.normal(size=(m, m)) for m in ms]
    g = raw_gemm(pur, pack(As), pack(Bs), None, 1.0, 0.0)
    for b, m in enumerate(ms):
        worst[2] = max(worst[2], worst_ratio(blocks(g, ms)[b], (As[b].astype(np.longdouble) @ Bs[b].astype(np.longdouble)).astype(np.float64),
                                             (m + 4) * U * (np.abs(As[b]) @ np.abs(Bs[b]))))
    assert worst[2] <= 1.0
    nos = [max(1, m // 3) for m in ms]
    Xs = [a / m for a, m in zip(As, ms)]
    start_step(pur, ms, Xs, nos)
    worst[3] = check_step(pur, ms, Xs, nos, False, "random")
    X1s = [symmetric(rng, m) for m in ms]
    Gt, X1, Q = pur.response_start(dev(pack(As)))
    pur.state.coeff.copy_(dev(pack(Xs)))
    X1.copy_(dev(pack(X1s)))
    Ybefore = pur.state.chol.clone()
    pur.response_step(0, X1, Q)
    assert torch.equal(Ybefore.view(torch.int64), pur.state.chol.view(torch.int64))   # the same product routine, the same summation order: Y bit for bit
    for b, m in enumerate(ms):
        if m == 1:
            continue
        X, A1 = Xs[b].astype(np.longdouble), X1s[b].astype(np.longdouble)
        got = blocks(Q.cpu().numpy(), ms)[b]
        assert np.array_equal(got, got.T)
        f = worst_ratio(np.tril(got), np.tril((A1 @ X + X @ A1).astype(np.float64)), np.tril((2 * m + 4) * U * (np.abs(X1s[b]) @ np.abs(Xs[b]) + np.abs(Xs[b]) @ np.abs(X1s[b]))))
        worst[4] = max(worst[4], f)
        assert f <= 1.0, (b, m, f)
    print("orbital_purify_parity kernels worst error / bound: congruence first %.3f second %.3f gemm %.3f square %.3f response %.3f" % tuple(worst))


def test_single_step_at_the_largest_size():
    """m = 1024, one SP2 step and one response step.  The reference is plain float64 numpy, whose own rounding shares the bound with the kernel's."""
    rng = np.random.Generator(np.random.PCG64(4))
    m = 1024
    X = symmetric(rng, m) / m
    pur, op = purification([m])
    start_step(pur, [m], [X], [300])
    w = check_step(pur, [m], [X], [300], False, "m=1024")
    print(f"orbital_purify_parity kernels m=1024 square worst error / bound {w:.3f}")


# ---- 3. the whole route -------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(inputs):
    """[(case, H, S, G, T, eps, D, gH, gS)] from ``closed_form`` on the inputs as the device sees them (float32: H rounded; standard: S = None)."""
    out = []
    for case in DR.CASES:
        H, S = DR.gapped_case(*case, standard=inputs == "standard")
        if inputs == "float32":
            H = H.astype(np.float32).astype(np.float64)
        G, T = DR.upstream(case[0], case[4])
        eps, D, gH, gS = DR.closed_form(H, S, case[1], DR.quadratic_loss(G, T, with_eps=False))
        out.append((case, H, S, G, T, eps, D, gH, gS))
    return out


def device_loss(D, refs, pp):
    total = 0.0
    for b, r in enumerate(refs):
        m = r[1].shape[0]
        Db = D[int(pp[b]):int(pp[b + 1])].view(m, m)
        total = total + (dev(r[3]) * Db).sum() + 0.5 * ((Db - dev(r[4])) ** 2).sum()
    return total


def figures(tag, refs, D, gH, gS, out_round):
    """``out_round``: the rounding of a float32 gradient of H; S and its gradient are float64 in every run."""
    ms = [r[1].shape[0] for r in refs]
    Ds, gHs = blocks(D, ms), blocks(gH, ms)
    gSs = None if gS is None else blocks(gS, ms)
    worst = np.zeros(4)
    for b, (case, H, S, G, T, eps, Dr, rH, rS) in enumerate(refs):
        m, n = case[0], case[1]
        uD = PR.density_unit(H, S, n, eps, Dr)
        uH, uS = DR.units(H, S, n, eps, rH, rS)
        kap = 1.0 if S is None else np.linalg.cond(S)
        assert np.array_equal(Ds[b], Ds[b].T) and np.array_equal(gHs[b], gHs[b].T)
        fD = float(np.abs(Ds[b] - Dr).max() / uD)
        ne = float((Ds[b] * (np.eye(m) if S is None else S)).sum())
        fN = abs(ne - 2.0 * n) / (m * R.EPS * kap * 2.0 * n)
        fH = float((np.maximum(np.abs(gHs[b] - rH) - out_round * np.abs(rH), 0.0) / uH).max())
        fS = 0.0
        if gSs is not None:
            assert np.array_equal(gSs[b], gSs[b].T)
            fS = float(np.abs(gSs[b] - rS).max() / uS)
        if n == m:
            assert np.all(gHs[b] == 0.0), (tag, case)                # X = I whatever H is: exactly zero
        worst = np.maximum(worst, [fD, fN, fH, fS])
        print(f"orbital_purify_parity end-to-end {tag} m={m} n_occ={n} kappa0={case[3]:g} D {fD:.3g} Tr(DS) {fN:.3g} gH {fH:.3g} gS {fS:.3g} (bound {BOUND:.0f})")
        assert fD <= BOUND and fN <= BOUND and fH <= BOUND and fS <= BOUND, (tag, case, fD, fN, fH, fS)
    print("orbital_purify_parity end-to-end %s worst D %.3g Tr(DS) %.3g gH %.3g gS %.3g" % ((tag,) + tuple(worst)))


def run_route(inputs):
    from nabladft_amd.orbital_loss import purified_density_matrix
    refs = reference(inputs)
    Hs, nos = [r[1] for r in refs], [r[0][1] for r in refs]
    op, pp = ptrs(Hs)
    H = dev(pack(Hs), torch.float32 if inputs == "float32" else torch.float64).requires_grad_(True)
    S = None if inputs == "standard" else dev(pack([r[2] for r in refs])).requires_grad_(True)
    D, pur = purified_density_matrix(H, S, op, nos, return_solution=True)
    assert D.dtype == torch.float64 and D.requires_grad
    device_loss(D, refs, pp).backward()
    pur.check()
    assert H.grad.dtype == H.dtype and H.grad.shape == H.shape
    return refs, op, pp, H, S, D, pur


@pytest.mark.parametrize("inputs", ["float64", "standard", "float32"])
def test_purification_end_to_end(inputs):
    refs, op, pp, H, S, D, pur = run_route(inputs)
    it = pur.iterations.cpu().numpy()
    ms = [r[1].shape[0] for r in refs]
    assert all((it[b] == 0) == (r[0][1] == r[0][0]) or ms[b] < 3 for b, r in enumerate(refs)) and it.max() <= 60
    print(f"orbital_purify_parity end-to-end {inputs} iterations {it.tolist()}")
    figures(inputs, refs, D.detach().cpu().numpy(), H.grad.double().cpu().numpy(), None if S is None else S.grad.cpu().numpy(),
            2.0 ** -24 if inputs == "float32" else 0.0)
    # the restatement takes the same branches and needs the same number of iterations
    log = pur.log.cpu().numpy()
    for b, r in enumerate(refs):
        sol = PR.density_and_gradients(r[1], r[2], r[0][1])[3]
        if sol["kind"] == 0 and ms[b] >= 17:
            assert abs(int(it[b]) - sol["iters"]) <= 2 and log[b, :8].tolist() == sol["log"][:8], (b, it[b], sol["iters"])


def test_agreement_with_orbital_solution():
    """The existing path as yardstick: the same batch through ``orbital_solution``; D and both gradients agree within the same units."""
    from nabladft_amd.orbital_loss import orbital_solution
    refs, op, pp, H, S, D, pur = run_route("float64")
    nos = [r[0][1] for r in refs]
    H2, S2 = H.detach().clone().requires_grad_(True), S.detach().clone().requires_grad_(True)
    eps, D2, sol = orbital_solution(H2, S2, op, nos, return_solution=True)
    device_loss(D2, refs, pp).backward()
    sol.check()
    ms = [r[1].shape[0] for r in refs]
    worst = np.zeros(3)
    for b, (case, Hm, Sm, G, T, e, Dr, rH, rS) in enumerate(refs):
        uD = PR.density_unit(Hm, Sm, case[1], e, Dr)
        uH, uS = DR.units(Hm, Sm, case[1], e, rH, rS)
        d = lambda x, y: np.abs(blocks(x.detach().cpu().numpy(), ms)[b] - blocks(y.detach().cpu().numpy(), ms)[b]).max()
        fig = np.array([d(D, D2) / uD, d(H.grad, H2.grad) / uH, d(S.grad, S2.grad) / uS])
        worst = np.maximum(worst, fig)
        assert np.all(fig <= BOUND), (case, fig)
    print("orbital_purify_parity against orbital_solution worst D %.3g gH %.3g gS %.3g (units, bound %.0f)" % (tuple(worst) + (BOUND,)))


# ---- 4. bitwise ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_batch_independent_and_the_response_repeats_x():
    refs = reference("float64")
    Hs, Ss, Gs, nos = [r[1] for r in refs], [r[2] for r in refs], [r[3] for r in refs], [r[0][1] for r in refs]
    ms = [h.shape[0] for h in Hs]

    def run(idx):
        pur, op = purification([ms[i] for i in idx])
        orth = pur.orthogonalize(dev(pack([Ss[i] for i in idx])))
        pur.purify(dev(pack([Hs[i] for i in idx])), [nos[i] for i in idx])
        X = pur.projector.clone()
        D = pur.density()
        gH, gS = pur.response(dev(pack([Gs[i] for i in idx])))
        assert torch.equal(X.view(torch.int64), pur.projector.view(torch.int64))   # the response pass reproduced the forward's X bit for bit
        gH1, none = pur.response(dev(pack([Gs[i] for i in idx])), overlap=False)
        assert none is None and torch.equal(gH1, gH)
        pur.check()
        return [t.cpu().numpy() for t in (orth.Z, X, D, gH, gS)]
    every = list(range(len(ms)))
    a, b2 = run(every), run(every)
    assert all(same_bits(x, y) for x, y in zip(a, b2))
    for b in (0, 3, 5, len(ms) - 1):                                 # alone: the same bits as inside the batch
        alone = run([b])
        for x, y in zip(alone, a):
            assert same_bits(x.reshape(ms[b], ms[b]), blocks(y, ms)[b]), (b, ms[b])


# ---- 5. failures and edges -----------------------------------------------------------------------------------------------------------------------------------------
def gapless(m, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lev = np.sort(rng.uniform(-5.0, 5.0, size=m))
    lev[n] = lev[n - 1]                                              # two equal levels across the Fermi level
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    A = (Q * lev[None, :]) @ Q.T
    return 0.5 * (A + A.T)


def test_failures_and_edge_cases():
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import BatchedOrbitals
    cases = [(17, 5, 0.3, 1e2, 1), (65, 21, 0.3, 1e2, 2), (33, 11, 0.3, 1e2, 3), (20, 0, 0.3, 1e2, 4), (20, 20, 0.3, 1e2, 5)]
    Hs = [DR.gapped_case(m, max(n, 1), g, k, s, standard=True)[0] for m, n, g, k, s in cases]
    Hs[1] = gapless(65, 21, 7)
    nos = [c[1] for c in cases]
    ms = [c[0] for c in cases]
    G = np.concatenate([np.random.Generator(np.random.PCG64(8)).normal(size=m * m) for m in ms])
    pur, op = purification(ms)
    pur.purify(dev(pack(Hs)), nos)
    D = blocks(pur.density().cpu().numpy(), ms)
    gH = blocks(pur.response(dev(G))[0].cpu().numpy(), ms)
    status, it = pur.status.cpu().numpy(), pur.iterations.cpu().numpy()
    assert status.tolist() == [0, 4, 0, 0, 0] and it[1] == 100 and it[3] == 0 and it[4] == 0
    assert np.isnan(D[1]).all() and np.isnan(gH[1]).all() and all(np.isfinite(D[b]).all() and np.isfinite(gH[b]).all() for b in (0, 2, 3, 4))
    assert np.all(D[3] == 0.0) and np.array_equal(D[4], 2.0 * np.eye(20)) and np.all(gH[3] == 0.0) and np.all(gH[4] == 0.0)   # n_occ = 0 and n_occ = m
    with pytest.raises(RuntimeError, match="molecule 1: the purification did not converge in 100 iterations"):
        pur.check()
    for b in (0, 2):                                                 # the neighbours of the failed molecule: as if alone
        alone, _ = purification([ms[b]])
        alone.purify(dev(pack([Hs[b]])), [nos[b]])
        assert same_bits(alone.density().cpu().numpy().reshape(ms[b], ms[b]), D[b])
        e, C = R.solve(Hs[b], None)
        Dr = 2.0 * C[:, :nos[b]] @ C[:, :nos[b]].T
        assert np.abs(D[b] - Dr).max() <= BOUND * PR.density_unit(Hs[b], None, nos[b], e, Dr)
    # max_iter too small: every molecule that iterates fails, the trivial ones do not
    short, _ = purification(ms)
    short.purify(dev(pack(Hs)), nos, max_iter=5)
    assert short.status.cpu().numpy().tolist() == [4, 4, 4, 0, 0] and short.iterations.cpu().numpy().tolist() == [5, 5, 5, 0, 0]
    assert np.isnan(blocks(short.density().cpu().numpy(), ms)[0]).all()
    # the same state again: the status is reset
    short.purify(dev(pack(Hs)), nos)
    assert short.status.cpu().numpy().tolist() == [0, 4, 0, 0, 0]
    # refusals
    with pytest.raises(ValueError, match="outside 0..m"):
        pur.purify(dev(pack(Hs)), [5, 21, 11, 0, 21])
    with pytest.raises(ValueError, match="max_iter"):
        pur.purify(dev(pack(Hs)), nos, max_iter=0)
    with pytest.raises(ValueError, match="entries"):
        pur.purify(dev(pack(Hs[:2])), nos)
    lib, st = _lib.load(), pur.state
    P = st.P
    t = torch.zeros(P, dtype=torch.float64, device=DEV)
    assert lib.nq_orb_pur_response_step(_lib.ptr(st.buf), *st._dims, 0, 100, _lib.ptr(pur.log), None, _lib.ptr(t), _lib.stream_ptr()) == _lib.NQ_ERR_ARG
    assert b"second output" in lib.nq_last_error()
    assert lib.nq_orb_pur_step(_lib.ptr(st.buf), *st._dims, 100, 100, _lib.ptr(pur.ctl), _lib.ptr(pur.log), _lib.stream_ptr()) == _lib.NQ_ERR_ARG
    assert lib.nq_orb_pur_congruence(_lib.ptr(st.buf), *st._dims, _lib.ptr(t), 0, _lib.ptr(t), 1, 0, 1.0, _lib.ptr(t), _lib.ptr(t), _lib.stream_ptr()) == _lib.NQ_ERR_ARG
    # a purification state passed to a call that reads coefficients, and a solver state passed to a purification step: header status -3, nothing touched
    before = st.coeff.clone()
    BatchedOrbitals.weighted_gram(pur, torch.ones(st.M, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="purification"):
        st.header()
    assert torch.equal(before.view(torch.int64), st.coeff.view(torch.int64))
    orb = BatchedOrbitals(op, DEV).solve(dev(pack(Hs)))
    coeff = orb.coefficients.clone()
    assert lib.nq_orb_pur_step(_lib.ptr(orb.state.buf), *orb.state._dims, 0, 100, _lib.ptr(pur.ctl), _lib.ptr(pur.log), _lib.stream_ptr()) == 0
    with pytest.raises(RuntimeError, match="purification"):
        orb.state.header()
    assert torch.equal(coeff, orb.coefficients)
    # other dimensions than nq_orb_init: header status -2, nothing touched
    fresh, _ = purification(ms)
    fresh.purify(dev(pack(Hs)), nos)
    X = fresh.projector.clone()
    B, M, P = fresh.state._dims
    assert lib.nq_orb_pur_step(_lib.ptr(fresh.state.buf), B, M + 1, P, 0, 100, _lib.ptr(fresh.ctl), _lib.ptr(fresh.log), _lib.stream_ptr()) == 0
    with pytest.raises(RuntimeError, match="other dimensions"):
        fresh.state.header()
    assert torch.equal(X.view(torch.int64), fresh.projector.view(torch.int64))


# ---- 6. populations and the losses on the database molecules -----------------------------------------------------------------------------------------------------
def test_losses_on_the_database_molecules_against_the_solver_route():
    """``purified_density_matrix`` -> ``populations`` -> ``MullikenChargeLoss`` + ``DensityMatrixLoss`` on the six database molecules against the
    ``orbital_solution`` route: the loss and both gradients, in the units of the yardstick.  A molecule whose overlap is not positive definite fails in
    both routes (status 1) and is left out of the loss."""
    import nabladft_amd as nq
    probs = db_problems()
    Hs, Ss = [p[0] for p in probs], [p[1] for p in probs]
    ms = [h.shape[0] for h in Hs]
    good = [b for b, s in enumerate(Ss) if np.linalg.eigvalsh(s).min() > 0.0]
    op, pp = ptrs(Hs)
    plan, per_atom = db_plan(probs)
    z = np.concatenate([np.asarray(p[2], dtype=np.int64) for p in probs])
    aptr = np.concatenate([[0], np.cumsum([len(p[2]) for p in probs])])
    n_occ = nq.occupied_counts(z, aptr, 0, op)
    rng = np.random.Generator(np.random.PCG64(12))
    q_t = dev(rng.normal(size=len(z)) * 0.3)
    D_t = dev(pack([2.0 * np.eye(m) + 0.1 * (lambda N: N + N.T)(rng.normal(size=(m, m))) for m in ms]))
    keep_d = dev(np.concatenate([np.full(m * m, float(b in good)) for b, m in enumerate(ms)]))
    keep_q = dev(np.concatenate([np.full(len(p[2]), float(b in good)) for b, p in enumerate(probs)]))
    l_q, l_d = nq.MullikenChargeLoss("mse"), nq.DensityMatrixLoss("mae")

    def route(purified):
        H, S = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss)).requires_grad_(True)
        if purified:
            D, sol = nq.purified_density_matrix(H, S, op, n_occ, return_solution=True)
        else:
            _, D, sol = nq.orbital_solution(H, S, op, n_occ, return_solution=True)
        status = sol.status.cpu().numpy()
        assert [b for b in range(len(ms)) if status[b] == 0] == good and all(status[b] == 1 for b in range(len(ms)) if b not in good)
        Dk = torch.where(keep_d > 0, D, D_t)                          # the failed molecule's NaN block contributes nothing
        pop = nq.populations(Dk, plan, S, None, sol)[0]
        q = torch.where(keep_q > 0, nq.mulliken_charges(z, pop), q_t)
        loss = l_q(q, q_t, aptr) + l_d(Dk, D_t, op)
        loss.backward()
        return float(loss.detach()), H.grad.cpu().numpy(), S.grad.cpu().numpy(), D.detach().cpu().numpy()
    lp, gHp, gSp, Dp = route(True)
    ls, gHs, gSs, Ds = route(False)
    assert abs(lp - ls) <= 1e-9 * abs(ls), (lp, ls)
    worst = np.zeros(3)
    for b in good:
        e, C = R.solve(Hs[b], Ss[b])
        n = int(n_occ[b])
        Dr = 2.0 * C[:, :n] @ C[:, :n].T
        rH, rS = blocks(gHs, ms)[b], blocks(gSs, ms)[b]
        uD = PR.density_unit(Hs[b], Ss[b], n, e, Dr)
        uH, uS = DR.units(Hs[b], Ss[b], n, e, rH, rS)
        fig = np.array([np.abs(blocks(Dp, ms)[b] - Dr).max() / uD, np.abs(blocks(gHp, ms)[b] - rH).max() / uH, np.abs(blocks(gSp, ms)[b] - rS).max() / uS])
        worst = np.maximum(worst, fig)
        print(f"orbital_purify_parity losses db {b} m={ms[b]} n_occ={n} gap {e[n] - e[n - 1]:.3f} D {fig[0]:.3g} gH {fig[1]:.3g} gS {fig[2]:.3g} (bound {BOUND:.0f})")
        assert np.all(fig <= BOUND), (b, fig)
    print("orbital_purify_parity losses loss %.15g solver route %.15g worst D %.3g gH %.3g gS %.3g" % ((lp, ls) + tuple(worst)))


# ---- 7. the QHNet task ------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_purified_density_task(monkeypatch):
    """One training step of ``QHNetPurifiedDensityLightning`` against ``QHNetDensityLightning`` with the same two keys.

    Bounds.  The two routes hand float64 gradients to the packed float32 prediction that differ by at most 2 x 10 units of the yardstick (each within 10 of
    the truth), far below the float32 rounding 2^-24 |g| they are cast with, so the gradient at the predicted Hamiltonian may differ by that rounding: one
    float32 ulp, 2^-23 |g|, plus the units.  From there both tasks run the same float32 backward of the network, a linear map evaluated with float32 sums: a
    perturbation of one ulp of its input moves an output by a few ulps of the largest entry of that parameter's gradient; 2^-20 max|grad| (eight ulps) is
    allowed per parameter tensor.  The losses are float32 sums of the same terms: relative 1e-6, the tolerance of the sibling test."""
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from nabladft_amd.orbitals import BatchedPurification
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
    charge = [0, -1, 1]
    coefs = {"hamiltonian": 1.0, "density_matrix": 0.5, "mulliken_charges": 2.0}
    losses = {"hamiltonian": HamiltonianLoss(), "density_matrix": nq.DensityMatrixLoss("mse", charge), "mulliken_charges": nq.MullikenChargeLoss("mse", charge)}
    make = lambda cls, ls, cs: cls("QHNet", net, None, None, ls, None, None, cs)
    calls = []
    real = BatchedPurification.orthogonalize
    monkeypatch.setattr(BatchedPurification, "orthogonalize", lambda self, S: (calls.append(1), real(self, S))[1])
    params = [p for p in net.parameters() if p.requires_grad]

    def step(cls):
        for p in params:
            p.grad = None
        task = make(cls, losses, coefs)
        loss = task.training_step(batch, 0)
        loss.backward()
        return loss.detach().double(), [None if p.grad is None else p.grad.detach().clone() for p in params], task
    lp, gp, task_p = step(nq.QHNetPurifiedDensityLightning)
    assert len(calls) == 1, len(calls)                             # ONE orthogonaliser launch per step, for prediction and target
    ls, gs, task_s = step(nq.QHNetDensityLightning)
    print("orbital_purify_parity qhnet task loss %.9g solver route %.9g" % (float(lp), float(ls)))
    assert torch.allclose(lp, ls, rtol=1e-6, atol=0.0)
    worst = 0.0
    for a, b in zip(gp, gs):
        assert (a is None) == (b is None)
        if a is not None and float(b.abs().max()) > 0.0:
            f = float((a - b).abs().max() / b.abs().max()) / 2.0 ** -20
            worst = max(worst, f)
            assert f <= 1.0, f
    print(f"orbital_purify_parity qhnet task worst parameter-gradient difference / (2^-20 max|grad|) {worst:.3g}")
    # the gradient arriving at the predicted Hamiltonian from the two orbital terms
    def at_prediction(task):
        preds, targets, _ = task._evaluate(batch)
        op = np.asarray(net.last_plan.mol_orb_ptr.cpu().numpy(), dtype=np.int64)
        terms = (coefs["density_matrix"] * losses["density_matrix"](preds["density_matrix"], targets["density_matrix"], op)
                 + coefs["mulliken_charges"] * losses["mulliken_charges"](preds["mulliken_charges"], targets["mulliken_charges"], batch.ptr))
        return torch.autograd.grad(terms, preds["hamiltonian"])[0].double().cpu().numpy()
    ga, gb = at_prediction(task_p), at_prediction(task_s)
    assert np.all(np.abs(ga - gb) <= 2.0 ** -22 * np.abs(gb) + 2.0 ** -30 * np.abs(gb).max())
    # an energy term has no place here; with both coefficients at 0 the step is QHNetLightning's and nothing is purified
    with_e = dict(losses, orbital_energies=nq.OrbitalEnergyLoss("mae", "occupied", charge))
    with pytest.raises(ValueError, match="no orbital energies"):
        make(nq.QHNetPurifiedDensityLightning, with_e, dict(coefs, orbital_energies=0.25)).training_step(batch, 0)
    plain = make(nq.QHNetLightning, {"hamiltonian": HamiltonianLoss()}, {"hamiltonian": 1.0})
    zero = make(nq.QHNetPurifiedDensityLightning, with_e, {"hamiltonian": 1.0, "orbital_energies": 0.0, "density_matrix": 0.0, "mulliken_charges": 0.0})
    before = len(calls)
    a, b = plain.training_step(batch, 0), zero.training_step(batch, 0)
    assert a.dtype == b.dtype and torch.equal(a.detach(), b.detach()) and len(calls) == before
