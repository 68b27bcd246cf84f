"""GPU: all occupied levels and coefficients without a full solve (csrc/orbocc.hip) through the C ABI and through ``BatchedPurification.occupied`` /
``OccupiedOrbitals`` / ``purified_occupied_energies`` / ``OccupiedEnergyLoss`` / ``QHNetPurifiedOrbitalLightning`` / ``PurifiedOrbitalErrors``, against
``np.linalg.eigh``, the numpy restatement (tests/orbital_occupied_ref.py), ``torch.linalg`` autograd and the solver route.

Units (tests/test_orbital_occupied_cpu.py): ``U_eps = m 2^-52 kappa_2(S) (eps_max - eps_min)`` for a level, floored at one ulp of the largest level (m = 1 has no
spread); ``U_eps / sep max(1, max|c c^T|)`` for ``c c^T``; ``u_Q = m^(3/2) 2^-52`` for the defects of the factor; ``(u_Q + 2 m 2^-52) kappa_2(S)`` for
``C S C^T - I``; for the gradients the units of tests/test_orbital_loss_gpu.py, ``U_H = m 2^-52 |S^-1|_2 max|g|`` and ``U_S = U_H |H|_2 |S^-1|_2``.  Bound 10 units each.
Every figure is printed as an ``orbital_occupied_parity ...`` line (kept in profiles/orbital_occupied_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_frontier_ref as FR
import orbital_grad_ref as GR
import orbital_occupied_ref as OR
import orbital_purify_ref as PR
from test_orbital_loss_gpu import blocks
from test_orbital_purify_gpu import SENTINEL, gapless, guarded, purification, unguard
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130]
sym = lambda a: 0.5 * (a + a.T)
nz = lambda a: np.nan_to_num(a, nan=-1.0)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(DEV)


def occupations(m):
    return sorted({n for n in (0, 1, m // 2, m - 1, m, 15, 16, 17, 63, 64, 65) if 0 <= n <= m})


def level_unit(m, ev, kappa):
    return max(OR.level_unit(m, ev[-1] - ev[0], kappa), 2.0 ** -52 * float(np.abs(ev).max()))


def uploaded(Hts, Xs, nos):
    """A purification state that holds these ``Ht`` and ``X`` (the kind word comes from a real ``purify`` of the standard problem, whose projector is then
    overwritten and whose status words are cleared)."""
    pur, op = purification([h.shape[0] for h in Hts])
    pur.purify(dev(pack(Hts)), nos)
    pur.state.work.copy_(dev(pack(Hts)))
    pur.state.coeff.copy_(dev(pack(Xs)))
    pur.state.status.zero_()
    return pur, op


def raw_factor(st, nos):
    """``nq_orb_occ_factor`` into guarded, sentinel-filled outputs -> dict of numpy arrays."""
    from nabladft_amd import _lib
    B, M, P = st.B, st.M, st.P
    Qb, Q = guarded(P)
    mb, mp = guarded(B)
    db, df = guarded(B)
    piv = torch.full((M + 16,), -77, dtype=torch.int32, device=DEV)
    stat = torch.full((B + 16,), -77, dtype=torch.int32, device=DEV)
    no_d = i32(nos)
    rc = _lib.load().nq_orb_occ_factor(_lib.ptr(st.buf), *st._dims, _lib.ptr(no_d), _lib.ptr(Q), _lib.ptr(piv[8:]), _lib.ptr(mp), _lib.ptr(df), _lib.ptr(stat[8:]),
                                       _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()
    ph, sh = piv.cpu().numpy(), stat.cpu().numpy()
    assert np.all(ph[:8] == -77) and np.all(ph[8 + M:] == -77) and np.all(sh[:8] == -77) and np.all(sh[8 + B:] == -77)
    return dict(Q=unguard(Qb, "Q", full=False), min_pivot=unguard(mb, "min_pivot"), defect=unguard(db, "defect"), pivots=ph[8:8 + M], status=sh[8:8 + B])


# ---- 1. the ragged batch --------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_reference():
    """Every m of SIZES with n_occ = 0, 1, m / 2, m - 1, m and the values around 16 and 64 (shuffled), a generalized problem with kappa_2(S) of about 1e2: per
    molecule H, S, Z, Ht, the levels and vectors of ``eigh`` and the exact projector."""
    cases = [(m, n) for m in SIZES for n in occupations(m)]
    order = np.random.Generator(np.random.PCG64(78)).permutation(len(cases))
    out = []
    for i in order:
        m, n = cases[i]
        rng = np.random.default_rng(700 + 10 * m + n)
        A, _ = FR.random_hamiltonian(rng, m, n, gap=0.3 if (m + n) % 2 == 0 else 0.01)
        if m == 1:
            A = np.array([[-3.5 + n]])
        S = DR.overlap(m, 1e2, np.random.Generator(np.random.PCG64(950 + m + n)))
        L = np.linalg.cholesky(S)
        H = PR.lower_sym(L @ A @ L.T)
        Z = PR.orthogonalizer(S)
        Ht = PR.congruence(Z, H, False)
        Xe, ev, U = FR.exact_projector(Ht, n)
        out.append(dict(m=m, n=n, H=H, S=S, Z=Z, Ht=Ht, Xe=PR.lower_sym(Xe), ev=ev, U=U, kappa=float(np.linalg.cond(S))))
    return out


def check_occupied(tag, refs, occ, fac=None, Xs=None):
    """Levels, ``c c^T``, ``C S C^T``, the NaN slots and (with ``fac``: a ``raw_factor`` result for the projectors ``Xs``) the factor's defects -> the worst figures."""
    eps, C = occ.energies.cpu().numpy(), blocks(occ.coefficients.cpu().numpy(), [r["m"] for r in refs])
    status, piv, minp, defect = occ.status.cpu().numpy(), occ.pivots.cpu().numpy(), occ.min_pivot.cpu().numpy(), occ.defect.cpu().numpy()
    assert not status.any(), (tag, status)
    worst = dict(level=0.0, cct=0.0, csc=0.0, qqt=0.0, qtq=0.0, left=0.0)
    o = 0
    for b, r in enumerate(refs):
        m, n = r["m"], r["n"]
        e, Cb = eps[o:o + m], C[b]
        assert np.isnan(e[n:]).all() and np.isnan(Cb[n:]).all() and np.isfinite(e[:n]).all() and np.isfinite(Cb[:n]).all(), (tag, b, m, n)
        assert np.all(piv[o + n:o + m] == -1) and len(set(piv[o:o + n].tolist())) == n and np.all((piv[o:o + n] >= 0) & (piv[o:o + n] < m)), (tag, b, m, n)
        assert defect[b] <= BOUND * OR.q_unit(m), (tag, b, m, n, defect[b] / OR.q_unit(m))
        worst["left"] = max(worst["left"], defect[b] / OR.q_unit(m))
        if n == 0:
            assert minp[b] == np.inf
        else:
            assert minp[b] >= (1.0 - 1e-9) / m, (tag, b, m, n, minp[b] * m)
            u = level_unit(m, r["ev"], r["kappa"])
            fig = dict(level=np.abs(e[:n] - r["ev"][:n]).max() / u, csc=np.abs(Cb[:n] @ r["S"] @ Cb[:n].T - np.eye(n)).max() / OR.csc_unit(m, r["kappa"]), cct=0.0)
            assert np.all(np.diff(e[:n]) >= 0)
            for k in range(n):
                ck = r["Z"].T @ r["U"][:, k]
                ref = np.outer(ck, ck)
                fig["cct"] = max(fig["cct"], np.abs(np.outer(Cb[k], Cb[k]) - ref).max() / (u / FR.separation(r["ev"], k) * max(1.0, np.abs(ref).max())))
                at = int(np.argmax(np.abs(Cb[k])))
                assert Cb[k, at] > 0                                   # the solver's sign rule
            if fac is not None:
                Q = blocks(fac["Q"], [x["m"] for x in refs])[b][:n]
                fig.update(qqt=np.abs(Q @ Q.T - np.eye(n)).max() / OR.q_unit(m), qtq=np.abs(Q.T @ Q - Xs[b]).max() / OR.q_unit(m))
                assert np.array_equal(fac["pivots"][o:o + m], piv[o:o + m]) and fac["min_pivot"][b] == minp[b] and fac["defect"][b] == defect[b]
                assert all(np.all(Q[j + 1:, piv[o + j]] == 0.0) for j in range(n))       # the entries of earlier pivots are exactly 0
            assert max(fig.values()) <= BOUND, (tag, b, m, n, fig)
            for k, v in fig.items():
                worst[k] = max(worst[k], v)
        o += m
    print(f"orbital_occupied_parity {tag}: worst " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (bound {BOUND:g} each)")
    return worst


def test_ragged_batch_with_uploaded_exact_projectors():
    """The kernels without SP2: Ht, the projector of ``eigh`` and Z come from numpy; n_occ = 0 and n_occ = m molecules sit in the middle of the batch."""
    refs = ragged_reference()
    nos = [r["n"] for r in refs]
    pur, _ = uploaded([r["Ht"] for r in refs], [r["Xe"] for r in refs], nos)
    fac = raw_factor(pur.state, nos)
    assert not fac["status"].any()
    occ = pur.occupied(transform=dev(pack([r["Z"] for r in refs])))
    check_occupied("exact projector, ragged m = 1..130", refs, occ.check(), fac, [r["Xe"] for r in refs])
    Qb = blocks(fac["Q"], [r["m"] for r in refs])
    for b, r in enumerate(refs):                                       # rows k >= n_occ of Q are untouched
        assert np.all(Qb[b][r["n"]:] == SENTINEL), b
    D = blocks(occ.density().cpu().numpy(), [r["m"] for r in refs])
    for b, r in enumerate(refs):
        ref = 2.0 * r["Z"].T @ r["Xe"] @ r["Z"]
        if r["n"] == 0:
            assert not D[b].any(), b                                   # an empty range: zeros
            continue
        assert np.abs(D[b] - ref).max() <= BOUND * PR.density_unit(r["H"], r["S"], r["n"], r["ev"], ref) and same_bits(D[b], D[b].T), b


def test_ragged_batch_after_the_purification_and_against_the_solver():
    import nabladft_amd as nq
    refs = ragged_reference()
    ms, nos = [r["m"] for r in refs], [r["n"] for r in refs]
    Hd, Sd = dev(pack([r["H"] for r in refs])), dev(pack([r["S"] for r in refs]))
    pur, op = purification(ms)
    pur.orthogonalize(Sd)
    pur.purify(Hd, nos).check()
    Xs = blocks(pur.projector.cpu().numpy(), ms)
    fac = raw_factor(pur.state, nos)
    occ = pur.occupied().check()
    check_occupied("SP2 projector, ragged m = 1..130", refs, occ, fac, Xs)
    Dp, Do = blocks(pur.density().cpu().numpy(), ms), blocks(occ.density().cpu().numpy(), ms)
    sol = nq.BatchedOrbitals(op, DEV).solve(Hd, Sd)
    es, eo = sol.energies.cpu().numpy(), occ.energies.cpu().numpy()
    o, worst = 0, np.zeros(2)
    for b, r in enumerate(refs):
        m, n = r["m"], r["n"]
        if n == 0:
            assert not Do[b].any() and not Dp[b].any(), b
            o += m
            continue
        ud = PR.density_unit(r["H"], r["S"], n, r["ev"], Dp[b])
        fig = [np.abs(Do[b] - Dp[b]).max() / ud, 0.0 if n == 0 else np.abs(eo[o:o + n] - es[o:o + n]).max() / level_unit(m, r["ev"], r["kappa"])]
        assert max(fig) <= BOUND, (b, m, n, fig)
        worst = np.maximum(worst, fig)
        o += m
    print(f"orbital_occupied_parity SP2 projector, ragged: density() against BatchedPurification.density() {worst[0]:.3g} U_D, levels against BatchedOrbitals.solve "
          f"{worst[1]:.3g} U_eps (bound {BOUND:g})")


def test_compare_against_the_solver_route():
    """``eps_mae_occ`` / ``similarity`` / ``similarity_min`` / ``homo_abs_err`` of two purified solutions against ``BatchedOrbitals.solve`` + ``compare`` on the same
    inputs.  Every level is within 10 U_eps of the solver's on either side, so the MAE and the HOMO error are within 20 U_eps; ``|c^T S c'|`` moves by at most
    the two ``c c^T`` errors, 10 (U_eps / sep) on either side, times ``kappa_2(S)`` for the product with ``S`` (already in U_eps)."""
    import nabladft_amd as nq
    from nabladft_amd.orbitals import OCCUPIED_FIGURES
    refs = [r for r in ragged_reference() if r["n"] >= 1 and ((r["m"] + r["n"]) % 2 == 0 or r["n"] == r["m"])][:40]       # the 0.3 gaps: a perturbation of 1e-4 keeps them open
    ms, nos = [r["m"] for r in refs], [r["n"] for r in refs]
    op = np.concatenate([[0], np.cumsum(ms)])
    rng = np.random.default_rng(12)
    Hp = []
    for r in refs:
        E = rng.standard_normal((r["m"], r["m"])) * 1e-4
        Hp.append(r["H"] + PR.lower_sym(E))
    Hd, Hpd, Sd = dev(pack([r["H"] for r in refs])), dev(pack(Hp)), dev(pack([r["S"] for r in refs]))
    pt, pp = purification(ms)[0], purification(ms)[0]
    orth = pt.orthogonalize(Sd)
    ot = pt.purify(Hd, nos, orthogonalizer=orth).occupied().check()
    opd = pp.purify(Hpd, nos, orthogonalizer=orth).occupied().check()
    figs = opd.compare(ot, Sd).cpu().numpy()
    full = nq.BatchedOrbitals(op, DEV).solve(Hpd, Sd).compare(nq.BatchedOrbitals(op, DEV).solve(Hd, Sd), nos, Sd).cpu().numpy()
    rows = [nq.orbitals.FIGURES.index(k) for k in ("eps_mae_occ", "psi_sim_occ", "psi_sim_min_occ", "homo_abs_err")]
    worst = np.zeros(4)
    for b, r in enumerate(refs):
        m, n = r["m"], r["n"]
        L = np.linalg.cholesky(r["S"])
        evp = np.linalg.eigvalsh(sym(np.linalg.solve(L, np.linalg.solve(L, Hp[b]).T).T))
        u = max(level_unit(m, r["ev"], r["kappa"]), level_unit(m, evp, r["kappa"]))
        sep = min(min(FR.separation(e, k) for k in range(n)) for e in (r["ev"], evp))
        unit = np.array([2 * u, 2 * u / sep, 2 * u / sep, 2 * u])
        fig = np.abs(figs[:, b] - full[rows, b]) / unit
        assert fig.max() <= BOUND, (b, m, n, fig)
        worst = np.maximum(worst, fig)
    print("orbital_occupied_parity compare against BatchedOrbitals.solve + compare: " + ", ".join(f"{k} {v:.3g}" for k, v in zip(OCCUPIED_FIGURES, worst))
          + f" (units 2 U_eps, 2 U_eps / sep, 2 U_eps / sep, 2 U_eps; bound {BOUND:g})")
    with pytest.raises(ValueError, match="different batches"):
        opd.compare(purification(ms[:2])[0].purify(dev(pack([r["H"] for r in refs[:2]])), nos[:2]).occupied(), None)


# ---- 2. integer data: reduce and back are exact ----------------------------------------------------------------------------------------------------------------------
def test_integer_data_is_exact():
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import OrbitalState
    ms = [65, 1, 17, 130, 64, 3, 20]
    nos = [21, 1, 17, 66, 16, 0, 5]
    rng = np.random.Generator(np.random.PCG64(4))
    Hts, Xs, keeps = [], [], []
    for m, n in zip(ms, nos):
        Hts.append(PR.lower_sym(rng.integers(-4, 5, size=(m, m)).astype(np.float64)))
        keep = np.sort(rng.permutation(m)[:n])
        X = np.zeros((m, m))
        X[keep, keep] = 1.0
        Xs.append(X)
        keeps.append(keep)
    pur, op = uploaded(Hts, Xs, nos)
    fac = raw_factor(pur.state, nos)
    assert not fac["status"].any()
    Qb = blocks(fac["Q"], ms)
    o = 0
    for b, (m, n) in enumerate(zip(ms, nos)):                          # a diagonal 0/1 projector: pivots in index order, unit rows, exactly
        assert fac["pivots"][o:o + n].tolist() == keeps[b].tolist() and np.array_equal(Qb[b][:n], np.eye(m)[keeps[b]]), b
        assert fac["min_pivot"][b] == (1.0 if n else np.inf) and fac["defect"][b] == 0.0
        o += m
    # reduce: Hs = Q Ht Q^T on integers
    occ_st = OrbitalState(op, DEV)
    occ_st.coeff.copy_(dev(np.where(fac["Q"] == SENTINEL, 0.0, fac["Q"])))
    no_d = i32(nos)
    occ_ptr = np.concatenate([[0], np.cumsum(np.array(nos, dtype=np.int64) * np.array(ms))]).astype(np.int64)
    rows = np.maximum(np.array(nos), 1)
    red = OrbitalState(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), DEV)
    O = int(occ_ptr[-1])
    optr = dev(occ_ptr)
    Gs, T = torch.empty(occ_st.P, dtype=torch.float64, device=DEV), torch.empty(O, dtype=torch.float64, device=DEV)
    occ_st.call("nq_orb_resp_project", _lib.ptr(no_d), _lib.ptr(optr), O, _lib.ptr(pur.state.work), _lib.ptr(Gs), _lib.ptr(T))
    hb, Hs = guarded(red.P)
    stat = i32(np.zeros(len(ms)))
    occ_st.call("nq_orb_occ_reduce", _lib.ptr(no_d), _lib.ptr(optr), O, _lib.ptr(T), _lib.ptr(stat), _lib.ptr(red.pack_ptr), red.P, _lib.ptr(Hs))
    Hs_h = blocks(unguard(hb, "Hs"), rows.tolist())
    for b, n in enumerate(nos):
        ref = OR.reduce(np.eye(ms[b])[keeps[b]], Hts[b])
        assert np.array_equal(Hs_h[b], ref) and same_bits(Hs_h[b], Hs_h[b].T), b
    # back: C = V Q W on integers (V, the reduced levels and W written directly)
    Vs = [rng.integers(-3, 4, size=(r, r)).astype(np.float64) for r in rows]
    Ws = [rng.integers(-2, 3, size=(m, m)).astype(np.float64) for m in ms]
    lev = np.concatenate([np.sort(rng.integers(-9, 10, size=r)).astype(np.float64) for r in rows])
    red.coeff.copy_(dev(pack(Vs)))
    red.eps.copy_(dev(lev))
    ub, U = guarded(max(O, 1))
    for W in (dev(pack(Ws)), None):
        occ_st.coeff.copy_(dev(np.where(fac["Q"] == SENTINEL, 7.0, fac["Q"])))       # 7: what back must overwrite with NaN in the rows k >= n_occ
        rc = _lib.load().nq_orb_occ_back(_lib.ptr(occ_st.buf), _lib.ptr(red.buf), *occ_st._dims, red.M, red.P, _lib.ptr(no_d), _lib.ptr(optr), O, _lib.ptr(W),
                                         _lib.ptr(stat), _lib.ptr(U), _lib.stream_ptr())
        assert rc == 0, _lib.load().nq_last_error()
        unguard(ub, "U", full=False)
        Cb, e = blocks(occ_st.coeff.cpu().numpy(), ms), occ_st.eps.cpu().numpy()
        o = ro = 0
        for b, (m, n) in enumerate(zip(ms, nos)):
            Q = np.eye(m)[keeps[b]]
            ref = OR.sign_rows((Vs[b][:n, :n] @ Q) @ Ws[b] if W is not None else Vs[b][:n, :n] @ Q) if n else np.zeros((0, m))
            assert np.array_equal(Cb[b][:n] + 0.0, ref + 0.0) and np.isnan(Cb[b][n:]).all(), (b, W is None)
            assert np.array_equal(e[o:o + n], lev[ro:ro + n]) and np.isnan(e[o + n:o + m]).all(), b
            o, ro = o + m, ro + rows[b]
        assert not occ_st.status.cpu().numpy().any()


# ---- 3. the largest size ---------------------------------------------------------------------------------------------------------------------------------------------
def test_one_molecule_at_the_largest_size():
    """m = 1024, n_occ = 300, an uploaded exact projector: two threads' worth of columns per thread, five 64-row tiles of the reduced block."""
    rng = np.random.default_rng(1024)
    m, n = 1024, 300
    Ht, _ = FR.random_hamiltonian(rng, m, n, gap=0.3)
    Xe, ev, U = FR.exact_projector(Ht, n)
    Xe = PR.lower_sym(Xe)
    pur, _ = uploaded([Ht], [Xe], [n])
    fac = raw_factor(pur.state, [n])
    occ = pur.occupied().check()
    r = dict(m=m, n=n, H=Ht, S=np.eye(m), Z=np.eye(m), Ht=Ht, Xe=Xe, ev=ev, U=U, kappa=1.0)
    check_occupied("m=1024 n_occ=300, exact projector", [r], occ, fac, [Xe])


# ---- 4. failures, reproducibility, batch independence ----------------------------------------------------------------------------------------------------------------
def test_failed_molecules_reproducibility_and_batch_independence():
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import OrbitalState
    good = [(65, 21, 0.3, 1e2, 2), (17, 5, 0.3, 1e2, 1), (130, 43, 0.3, 1e4, 99)]
    pairs = [DR.gapped_case(*c) for c in good]
    bad_S = np.eye(20)
    bad_S[7, 7] = -1.0                                               # not positive definite: status 1
    Hs = [pairs[0][0], gapless(33, 11, 7), pairs[1][0], np.diag(np.arange(20.0)), pairs[2][0], np.diag(np.arange(12.0))]
    Ss = [pairs[0][1], np.eye(33), pairs[1][1], bad_S, pairs[2][1], np.eye(12)]
    ms, nos = [h.shape[0] for h in Hs], [21, 11, 5, 5, 43, 4]

    def run(sel, spoil=True):
        pur, _ = purification([ms[b] for b in sel])
        pur.orthogonalize(dev(pack([Ss[b] for b in sel])))
        pur.purify(dev(pack([Hs[b] for b in sel])), [nos[b] for b in sel])
        if spoil and 5 in list(sel):                                 # an uploaded non-projector: X = I / 2
            o = int(pur.state.pack_ptr_host[list(sel).index(5)])
            pur.state.coeff[o:o + 144] = dev(0.5 * np.eye(12).reshape(-1))
        occ = pur.occupied()
        g = torch.ones(pur.state.M, dtype=torch.float64, device=DEV)
        gH, gS = occ.weighted_gram(g, -(occ.energies * g))
        sel_ms = [ms[b] for b in sel]
        return pur, occ, blocks(gH.cpu().numpy(), sel_ms), blocks(gS.cpu().numpy(), sel_ms)
    pur, occ, gH, gS = run(range(6))
    assert pur.status.cpu().tolist() == [0, 4, 0, 1, 0, 0] and occ.status.cpu().tolist() == [0, 4, 0, 1, 0, 5]
    assert occ.state.status.cpu().tolist() == [0, 4, 0, 1, 0, 5]
    eps, C = occ.energies.cpu().numpy(), blocks(occ.coefficients.cpu().numpy(), ms)
    off = np.concatenate([[0], np.cumsum(ms)])
    minp, defect, piv = occ.min_pivot.cpu().numpy(), occ.defect.cpu().numpy(), occ.pivots.cpu().numpy()
    for b in (1, 3, 5):                                              # each alone in its NaN
        assert np.isnan(eps[off[b]:off[b + 1]]).all() and np.isnan(C[b]).all() and np.isnan(gH[b]).all() and np.isnan(gS[b]).all(), b
        assert np.isnan(minp[b]) and np.isnan(defect[b]) and np.all(piv[off[b]:off[b + 1]] == -1), b
    for b in (0, 2, 4):
        n = nos[b]
        assert np.isfinite(eps[off[b]:off[b] + n]).all() and np.isfinite(C[b][:n]).all() and np.isfinite(gH[b]).all() and np.isfinite(gS[b]).all(), b
        assert same_bits(gH[b], gH[b].T) and same_bits(gS[b], gS[b].T)
        ev = np.linalg.eigvalsh(sym(np.linalg.solve(np.linalg.cholesky(Ss[b]), np.linalg.solve(np.linalg.cholesky(Ss[b]), Hs[b]).T).T))
        assert np.abs(eps[off[b]:off[b] + n] - ev[:n]).max() <= BOUND * level_unit(ms[b], ev, float(np.linalg.cond(Ss[b])))
    with pytest.raises(RuntimeError, match="molecule 1: the purification did not converge"):
        occ.check()
    _, alone5, _, _ = run([5])
    with pytest.raises(RuntimeError, match=r"molecule 0: the purified matrix is not a projector of rank n_occ=4 .*status 5"):
        alone5.check()
    _, occ2, gH2, gS2 = run(range(6))                                # bitwise reproducible
    for a, b in ((occ.energies, occ2.energies), (occ.coefficients, occ2.coefficients), (occ.min_pivot, occ2.min_pivot), (occ.defect, occ2.defect)):
        assert same_bits(nz(a.cpu().numpy()), nz(b.cpu().numpy()))
    assert np.array_equal(piv, occ2.pivots.cpu().numpy()) and all(same_bits(nz(x), nz(y)) for x, y in zip(gH + gS, gH2 + gS2))
    for b in (0, 2, 4):                                              # alone: the same bits as between failed neighbours
        _, oa, gHa, gSa = run([b])
        assert same_bits(nz(oa.energies.cpu().numpy()), nz(eps[off[b]:off[b + 1]])) and same_bits(nz(oa.coefficients.cpu().numpy()), nz(C[b].reshape(-1))), b
        assert same_bits(gHa[0], gH[b]) and same_bits(gSa[0], gS[b]) and np.array_equal(oa.pivots.cpu().numpy(), piv[off[b]:off[b + 1]]), b
    # a state that holds no purification is refused: header status -3, nothing touched
    st = OrbitalState(np.array([0, 5, 8]), DEV)
    arrays = [torch.full((80,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(3)]
    ints = [torch.full((16,), -77, dtype=torch.int32, device=DEV) for _ in range(2)]
    no = i32([2, 1])
    assert _lib.load().nq_orb_occ_factor(_lib.ptr(st.buf), *st._dims, _lib.ptr(no), _lib.ptr(arrays[0]), _lib.ptr(ints[0]), _lib.ptr(arrays[1]), _lib.ptr(arrays[2]),
                                         _lib.ptr(ints[1]), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(st.header_dev[4]) == -3 and all(bool((a == SENTINEL).all()) for a in arrays) and all(bool((t == -77).all()) for t in ints)
    with pytest.raises(RuntimeError, match="holds a purification"):
        st.header()
    # Python refusals
    with pytest.raises(RuntimeError, match="purify"):
        purification(ms)[0].occupied()
    with pytest.raises(ValueError, match="transform"):
        pur.occupied(transform=torch.zeros(3, dtype=torch.float64, device=DEV))
    import nabladft_amd as nq
    with pytest.raises(ValueError, match="another batch"):
        nq.purified_occupied_energies(dev(pack(Hs[:2])), None, [0, 8], [2], solution=pur)
    with pytest.raises(ValueError, match="orthogonalizer without"):
        nq.purified_occupied_energies(dev(pack(Hs)), None, off, nos, orthogonalizer=pur.orthogonalizer)


# ---- 5. through Python: the gradients --------------------------------------------------------------------------------------------------------------------------------
GENERAL = [c for c in DR.CASES if 1 <= c[1] <= c[0]]


def occupied_loss(eps, n):
    return torch.tanh(0.1 * eps[:n]).sum()


@functools.lru_cache(maxsize=None)
def autograd_reference(inputs):
    """Per case of GENERAL: (H, S) rounded as the inputs are, the levels and the symmetrised gradients of ``sum_{k < n_occ} tanh(0.1 eps_k)`` by ``torch.linalg``."""
    out = []
    for case in GENERAL:
        m, n = case[0], case[1]
        H, S = DR.gapped_case(*case, standard=inputs == "standard")
        if inputs == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        Ht = torch.tensor(H, requires_grad=True)
        St = torch.tensor(np.eye(m) if S is None else S, requires_grad=True)
        L = torch.linalg.cholesky(St)
        Y = torch.linalg.solve_triangular(L, Ht, upper=False)
        A = torch.linalg.solve_triangular(L, Y.T, upper=False)
        e = torch.linalg.eigvalsh(0.5 * (A + A.T))
        occupied_loss(e, n).backward()
        ev = e.detach().numpy()
        g = 0.1 / np.cosh(0.1 * ev[:n]) ** 2
        uH, uS = GR.units(H, S, g)
        out.append(dict(m=m, n=n, H=H, S=S, ev=ev, gH=sym(Ht.grad.numpy()), gS=sym(St.grad.numpy()), kappa=1.0 if S is None else float(np.linalg.cond(S)), uH=uH, uS=uS))
    return out


@pytest.mark.parametrize("inputs", ["float64", "float32", "standard", "transform"])
def test_purified_occupied_energies_gradients_against_the_solver_and_torch_autograd(inputs):
    import nabladft_amd as nq
    refs = autograd_reference("float64" if inputs == "transform" else inputs)
    ms, nos = [r["m"] for r in refs], [r["n"] for r in refs]
    op = np.concatenate([[0], np.cumsum(ms)])
    dt = np.float32 if inputs == "float32" else np.float64
    Hd = dev(pack([r["H"] for r in refs], dtype=dt)).requires_grad_(True)
    Sd = None if inputs == "standard" else dev(pack([r["S"] for r in refs], dtype=dt)).requires_grad_(True)
    sel = torch.from_numpy(np.concatenate([np.arange(m) < n for m, n in zip(ms, nos)])).to(DEV)
    mol = torch.from_numpy(np.repeat(np.arange(len(ms)), ms)).to(DEV)

    def loss_of(eps):
        return torch.where(sel, torch.tanh(0.1 * eps), torch.zeros_like(eps)).sum()
    if inputs == "transform":                                        # S^(-1/2) by Newton-Schulz, SP2 on the standard problem, the back-transform handed in
        target = nq.scf_target_iterative(Hd.detach(), Sd.detach(), op, nos).check()
        occ = target.purification.occupied(transform=target.basis.inv_half).check()
        eps = occ.energies
        g = torch.where(sel, 0.1 / torch.cosh(0.1 * eps) ** 2, torch.zeros_like(eps))
        gH, gS = occ.weighted_gram(g, -(eps * g))
    else:
        eps, pur = nq.purified_occupied_energies(Hd, Sd, op, nos, return_solution=True)
        occ = pur.occupied_orbitals.check()
        loss_of(eps).backward()
        assert Hd.grad.dtype == Hd.dtype and Hd.grad.shape == Hd.shape and (Sd is None or (Sd.grad.dtype == Sd.dtype and Sd.grad.shape == Sd.shape))
        gH, gS = Hd.grad.double(), None if Sd is None else Sd.grad.double()
    # the solver route on the same inputs
    H2 = Hd.detach().clone().requires_grad_(True)
    S2 = None if Sd is None else Sd.detach().clone().requires_grad_(True)
    e2 = nq.orbital_energies(H2, S2, op)
    loss_of(e2).backward()
    sH, sS = blocks(H2.grad.double().cpu().numpy(), ms), None if S2 is None else blocks(S2.grad.double().cpu().numpy(), ms)
    ee, Cb = eps.detach().cpu().numpy(), blocks(occ.coefficients.cpu().numpy(), ms)
    gHb, gSb = blocks(gH.cpu().numpy(), ms), None if gS is None else blocks(gS.cpu().numpy(), ms)
    worst, o = np.zeros(6), 0
    for b, r in enumerate(refs):
        m, n = r["m"], r["n"]
        u = level_unit(m, r["ev"], r["kappa"])
        r32 = 2.0 ** -24 if inputs == "float32" else 0.0              # the gradients are cast to the inputs' dtype
        assert np.isnan(ee[o + n:o + m]).all()
        fig = [np.abs(ee[o:o + n] - r["ev"][:n]).max() / u, np.abs(gHb[b] - r["gH"]).max() / (r["uH"] + r32 * np.abs(r["gH"]).max()),
               np.abs(gHb[b] - sH[b]).max() / (r["uH"] + 2 * r32 * np.abs(r["gH"]).max())]
        if gSb is not None:
            fig += [np.abs(gSb[b] - r["gS"]).max() / (r["uS"] + r32 * np.abs(r["gS"]).max()), np.abs(gSb[b] - sS[b]).max() / (r["uS"] + 2 * r32 * np.abs(r["gS"]).max())]
            assert same_bits(gSb[b], gSb[b].T)
        if inputs == "transform":
            fig.append(np.abs(Cb[b][:n] @ r["S"] @ Cb[b][:n].T - np.eye(n)).max() / OR.csc_unit(m, r["kappa"]))
        print(f"orbital_occupied_parity purified_occupied_energies {inputs} m={m} n_occ={n} kappa={r['kappa']:.3g}: " + " ".join(f"{v:.3g}" for v in fig))
        assert same_bits(gHb[b], gHb[b].T) and max(fig) <= BOUND, (inputs, b, m, n, fig)
        worst[:len(fig)] = np.maximum(worst[:len(fig)], fig)
        o += m
    print(f"orbital_occupied_parity purified_occupied_energies {inputs}: worst levels {worst[0]:.3g} U_eps, gH {worst[1]:.3g} (autograd) {worst[2]:.3g} (solver) U_H, "
          f"gS {worst[3]:.3g} (autograd) {worst[4]:.3g} (solver) U_S (bound {BOUND:g})")


def test_nothing_is_launched_without_an_upstream_gradient_and_the_overlap_half_is_skipped(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.orbitals import OrbitalState
    r = autograd_reference("float64")[3]
    op = [0, r["m"]]
    Hd, Sd = dev(r["H"].reshape(-1)).requires_grad_(True), dev(r["S"].reshape(-1))
    runs = []
    real_call = OrbitalState.call
    monkeypatch.setattr(OrbitalState, "call", lambda self, name, *a: (runs.append(name), real_call(self, name, *a))[1])
    eps = nq.purified_occupied_energies(Hd, Sd, op, [r["n"]])
    assert runs.count("nq_orb_pur_run") == 1 and runs.count("nq_orb_occ_factor") == 1 and runs.count("nq_orb_wgram") == 0
    before = len(runs)
    (Hd * 2.0).sum().backward()                                      # no upstream gradient reaches eps
    assert runs[before:] == []
    Hd.grad = None
    before = len(runs)
    eps[:r["n"]].sum().backward()                                    # S asks for nothing: one launch, one output
    assert runs[before:] == ["nq_orb_wgram"] and bool(torch.isfinite(Hd.grad).all())
    D, sol = nq.purified_density_matrix(Hd, Sd, op, [r["n"]], return_solution=True)
    before = len(runs)
    e2 = nq.purified_occupied_energies(Hd, Sd, op, [r["n"]], solution=sol)
    mine = runs[before:]
    assert "nq_orb_pur_run" not in mine and "nq_orb_pur_init" not in mine and mine.count("nq_orb_occ_factor") == 1      # the shared solution is not purified again
    assert same_bits(nz(e2.detach().cpu().numpy()), nz(eps.detach().cpu().numpy()))


# ---- 6. the QHNet task -------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_purified_orbital_task(monkeypatch):
    """One training step with an occupied-energy term and a density term: no ``nq_orb_solve`` sees the full M, one orthogonaliser, one purification of the
    prediction (and one of the target); and with ``OccupiedEnergyLoss("mae")`` alone the loss of ``QHNetOrbitalLightning`` with ``OrbitalEnergyLoss("mae",
    "occupied")``: every level is within 10 U_eps of the solver's on both sides, so the two means of absolute differences are within 20 U_eps (mean over the
    molecules) of each other, plus the float32 sum of the two terms (1e-6 relative, the tolerance of the sibling tests)."""
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from nabladft_amd.orbitals import BatchedPurification, OrbitalState
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
    charge = [0, -1, 1]
    make = lambda cls, ls, cs: cls("QHNet", net, None, None, ls, None, None, cs)
    counts = dict(orth=0)
    solves, launches = [], []
    real_solve, real_orth, real_call = OrbitalState.solve, BatchedPurification.orthogonalize, OrbitalState.call
    monkeypatch.setattr(OrbitalState, "solve", lambda self, *a, **k: (solves.append(self.M), real_solve(self, *a, **k))[1])
    monkeypatch.setattr(BatchedPurification, "orthogonalize", lambda self, *a, **k: (counts.__setitem__("orth", counts["orth"] + 1), real_orth(self, *a, **k))[1])
    monkeypatch.setattr(OrbitalState, "call", lambda self, name, *a: (launches.append(name), real_call(self, name, *a))[1])
    params = [p for p in net.parameters() if p.requires_grad]
    M = sum(ms)

    def step(task):
        for p in params:
            p.grad = None
        loss = task.training_step(batch, 0)
        loss.backward()
        return loss.detach().double()
    losses = {"hamiltonian": HamiltonianLoss(), "occupied_energies": nq.OccupiedEnergyLoss("mae", charge), "density_matrix": nq.DensityMatrixLoss("mse", charge)}
    coefs = {"hamiltonian": 1.0, "occupied_energies": 0.7, "density_matrix": 0.5}
    loss = step(make(nq.QHNetPurifiedOrbitalLightning, losses, coefs))
    assert counts == dict(orth=1) and len(solves) == 2 and all(s < M for s in solves), (counts, solves, M)       # the reduced blocks only; ONE orthogonaliser
    assert launches.count("nq_orb_pur_run") == 2 and launches.count("nq_orb_occ_factor") == 2       # target and prediction, each purified once: the density shares it
    assert launches.count("nq_orb_wgram") == 1
    assert bool(torch.isfinite(loss)) and sum(1 for p in params if p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0) > 0
    # the same levels as the solver's, in the loss
    only = {"hamiltonian": HamiltonianLoss(), "occupied_energies": nq.OccupiedEnergyLoss("mae", charge)}
    task = make(nq.QHNetPurifiedOrbitalLightning, only, {"hamiltonian": 1.0, "occupied_energies": 0.7})
    lp = step(task)
    assert all(s < M for s in solves)
    solver = {"hamiltonian": HamiltonianLoss(), "orbital_energies": nq.OrbitalEnergyLoss("mae", "occupied", charge)}
    ls = step(make(nq.QHNetOrbitalLightning, solver, {"hamiltonian": 1.0, "orbital_energies": 0.7}))
    assert solves[-2:] == [M, M]
    preds, targets, _ = task._evaluate(batch)
    units = []
    for b, m in enumerate(ms):
        S = PR.lower_sym(batch.overlap[b].astype(np.float64))
        L = np.linalg.cholesky(S)
        for Hb in (PR.lower_sym(batch.hamiltonian[b].astype(np.float64)), PR.lower_sym(blocks(preds["hamiltonian"].detach().double().cpu().numpy(), ms)[b])):
            ev = np.linalg.eigvalsh(sym(np.linalg.solve(L, np.linalg.solve(L, Hb).T).T))
            units.append(level_unit(m, ev, float(np.linalg.cond(S))))
    allow = 0.7 * 2.0 * BOUND * float(np.mean(units)) * 2.0 + 1e-6 * float(ls.abs())
    print(f"orbital_occupied_parity qhnet task loss with the occupied-energy and density terms {float(loss):.9g}; OccupiedEnergyLoss(mae) {float(lp):.9g} against "
          f"QHNetOrbitalLightning with OrbitalEnergyLoss(mae, occupied) {float(ls):.9g} (allowed difference {allow:.3g})")
    assert abs(float(lp) - float(ls)) <= allow
    # the parent's refusal stays; with the coefficient at 0 the step is the parent's
    with_e = dict(only, orbital_energies=nq.OrbitalEnergyLoss("mae", "occupied", charge))
    with pytest.raises(ValueError, match="occupied orbital energies only"):
        make(nq.QHNetPurifiedOrbitalLightning, with_e, {"hamiltonian": 1.0, "occupied_energies": 0.7, "orbital_energies": 0.25}).training_step(batch, 0)
    dens = {"hamiltonian": HamiltonianLoss(), "occupied_energies": nq.OccupiedEnergyLoss("mae", charge), "density_matrix": nq.DensityMatrixLoss("mse", charge)}
    zero = {"hamiltonian": 1.0, "occupied_energies": 0.0, "density_matrix": 0.5}
    before = len(launches)
    a = make(nq.QHNetPurifiedOrbitalLightning, dens, zero).training_step(batch, 0)
    mine = launches[before:]
    del dens["occupied_energies"], zero["occupied_energies"]         # the parent does not know the key
    b = make(nq.QHNetPurifiedFrontierLightning, dens, zero).training_step(batch, 0)
    assert torch.equal(a.detach(), b.detach()) and "nq_orb_occ_factor" not in mine and mine == launches[before + len(mine):]


# ---- 7. the figures of a test loop ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["synthetic", "database"])
def test_purified_orbital_errors_against_orbital_errors(which):
    """Two batches through ``PurifiedOrbitalErrors`` and ``OrbitalErrors``: the means of the four figures agree within the per-molecule allowances of
    ``test_compare_against_the_solver_route`` (their mean over the molecules)."""
    import nabladft_amd as nq
    from nabladft_amd.orbitals import OCCUPIED_FIGURES
    rng = np.random.default_rng(21)
    if which == "synthetic":
        probs = [DR.gapped_case(*c) + (c[1],) for c in GENERAL]
    else:
        probs = []
        for H, S, z in db_problems()[:5]:                             # the sixth molecule's overlap is indefinite (tests/test_orbital_lowdin_gpu.py)
            probs.append((H, S, int(nq.occupied_counts(np.asarray(z, dtype=np.int64), [0, len(z)], 0)[0])))
    mine, theirs = nq.PurifiedOrbitalErrors(), nq.OrbitalErrors()
    allow = np.zeros(4)
    half = (len(probs) + 1) // 2
    for batch in (probs[:half], probs[half:]):
        ms, nos = [p[0].shape[0] for p in batch], [p[2] for p in batch]
        op = np.concatenate([[0], np.cumsum(ms)])
        z, ptr = np.concatenate([[2 * n] for n in nos]), np.arange(len(batch) + 1)       # one "atom" of 2 n_occ electrons per molecule
        Hp = [p[0] + PR.lower_sym(rng.standard_normal(p[0].shape) * 1e-3) for p in batch]
        args = (dev(pack(Hp)), dev(pack([p[0] for p in batch])), dev(pack([p[1] for p in batch])), op, z, ptr)
        mine.update(*args)
        theirs.update(*args)
        for (H, S, n), Hq in zip(batch, Hp):
            m = H.shape[0]
            L = np.linalg.cholesky(S)
            evs = [np.linalg.eigvalsh(sym(np.linalg.solve(L, np.linalg.solve(L, X).T).T)) for X in (H, Hq)]
            u = max(level_unit(m, e, float(np.linalg.cond(S))) for e in evs)
            sep = min(min(FR.separation(e, k) for k in range(n)) for e in evs)
            allow += np.array([2 * u, 2 * u / sep, 2 * u / sep, 2 * u]) / len(probs)
    a, b = mine.compute(), theirs.compute()
    pairs = dict(eps_mae_occ="eps_mae_occ", similarity="psi_sim_occ", similarity_min="psi_sim_min_occ", homo_abs_err="homo_abs_err")
    assert tuple(a) == OCCUPIED_FIGURES
    fig = [abs(a[k] - b[pairs[k]]) / allow[i] for i, k in enumerate(OCCUPIED_FIGURES)]
    print(f"orbital_occupied_parity PurifiedOrbitalErrors {which}: " + ", ".join(f"{k} {a[k]:.6g} ({f:.3g} units from OrbitalErrors)" for k, f in zip(OCCUPIED_FIGURES, fig))
          + f" (bound {BOUND:g})")
    assert max(fig) <= BOUND, fig


def test_purified_orbital_errors_report_a_failure_in_an_earlier_batch():
    import nabladft_amd as nq
    H, S = DR.gapped_case(17, 5, 0.3, 1e2, 1)
    acc = nq.PurifiedOrbitalErrors()
    bad = [gapless(33, 11, 7), H]
    acc.update(dev(pack([H, H])), dev(pack([H, H])), dev(pack([S, S])), [0, 17, 34], [10, 10], [0, 1, 2])
    acc.update(dev(pack([H, bad[0]])), dev(pack([H, np.diag(np.arange(33.0))])), dev(pack([S, np.eye(33)])), [0, 17, 50], [10, 22], [0, 1, 2])
    acc.update(dev(pack([H])), dev(pack([H])), dev(pack([S])), [0, 17], [10], [0, 1])
    with pytest.raises(RuntimeError, match="batch 1, predicted Hamiltonian, molecule 1: the purification did not converge in 100 iterations"):
        acc.compute()
    acc.reset()
    acc.update(dev(pack([H])), dev(pack([H])), dev(pack([S])), [0, 17], [10], [0, 1])
    out = acc.compute()
    assert out["eps_mae_occ"] == 0.0 and out["homo_abs_err"] == 0.0 and abs(out["similarity"] - 1.0) <= BOUND * OR.csc_unit(17, float(np.linalg.cond(S)))
