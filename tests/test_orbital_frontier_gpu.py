"""GPU: HOMO, LUMO and their gradients without a solve (csrc/orbfrontier.hip) through the C ABI and through ``BatchedPurification.frontier`` /
``purified_frontier`` / ``FrontierLoss`` / ``QHNetPurifiedFrontierLightning``, against ``np.linalg.eigh``, the numpy restatement
(tests/orbital_frontier_ref.py), ``torch.linalg`` autograd and the solver route.

Units (the issue's): ``U_eps = m 2^-52 kappa_2(S) (eps_max - eps_min)`` for a level, floored at one ulp of the largest level (m = 1 has no spread; no number is
known better than its own last bit); ``U_g = U_eps / sep max|x x^T|`` for ``vec vec^T``, ``coef coef^T`` and the gradients built from them (``sep``: the distance
from the level to its nearest neighbour).  Bound 10 units each; ``iters`` within 2 of the restatement's.  Float32 results are allowed their own rounding, 2^-24
per element.  Every figure is printed as an ``orbital_frontier_parity ...`` line (kept in profiles/orbital_frontier_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_frontier_ref as FR
import orbital_purify_ref as PR
from test_orbital_loss_gpu import blocks
from test_orbital_purify_gpu import SENTINEL, gapless, guarded, purification, unguard
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 5, 17, 64, 65, 130]
TOL = 2.0 ** -44
sym = lambda a: 0.5 * (a + a.T)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(DEV)


def vlayout(ms, k_max):
    kk = np.minimum(np.asarray(ms, dtype=np.int64), k_max)
    return np.concatenate([[0], np.cumsum(2 * kk * np.asarray(ms, dtype=np.int64))]).astype(np.int64)


def raw_lanczos(st, Ht, X, shift, nos, W, k_max=256, tol=TOL):
    """``nq_orb_front_lanczos`` into guarded, sentinel-filled outputs -> dict of numpy arrays.  ``Ht`` / ``X`` / ``W``: device float64 [P] (W may be None)."""
    from nabladft_amd import _lib
    B, M = st.B, st.M
    vp = vlayout(st.m, k_max)
    names = dict(eps=2 * B, vec=2 * M, coef=2 * M, res=2 * B)
    bufs = {k: guarded(n) for k, n in names.items()}
    Vbuf, V = guarded(int(vp[-1]))
    iters = torch.full((2 * B + 16,), -77, dtype=torch.int32, device=DEV)
    conv = torch.full((2 * B + 16,), -77, dtype=torch.int32, device=DEV)
    no_d, vp_d = i32(nos), dev(vp)
    rc = _lib.load().nq_orb_front_lanczos(_lib.ptr(st.buf), *st._dims, _lib.ptr(Ht), _lib.ptr(X), _lib.ptr(shift), _lib.ptr(no_d), _lib.ptr(W), int(k_max),
                                          float(tol), _lib.ptr(V), _lib.ptr(vp_d), _lib.ptr(bufs["eps"][1]), _lib.ptr(bufs["vec"][1]), _lib.ptr(bufs["coef"][1]),
                                          _lib.ptr(iters[8:]), _lib.ptr(bufs["res"][1]), _lib.ptr(conv[8:]), _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()
    out = {k: unguard(b[0], k) for k, b in bufs.items()}
    unguard(Vbuf, "V", full=False)
    ih, ch = iters.cpu().numpy(), conv.cpu().numpy()
    assert np.all(ih[:8] == -77) and np.all(ih[8 + 2 * B:] == -77) and np.all(ch[:8] == -77) and np.all(ch[8 + 2 * B:] == -77)
    out.update(eps=out["eps"].reshape(B, 2), res=out["res"].reshape(B, 2), vec=out["vec"].reshape(2, M), coef=out["coef"].reshape(2, M),
               iters=ih[8:8 + 2 * B].reshape(B, 2), conv=ch[8:8 + 2 * B].reshape(B, 2))
    return out


def raw_gram(st, g, eps, coef, conv, overlap=True):
    from nabladft_amd import _lib
    bH, gH = guarded(st.P)
    bS, gS = guarded(st.P)
    g_d, e_d, c_d, v_d = dev(g), dev(eps), dev(coef), i32(conv)
    rc = _lib.load().nq_orb_front_gram(_lib.ptr(st.buf), *st._dims, _lib.ptr(g_d), _lib.ptr(e_d), _lib.ptr(c_d), _lib.ptr(v_d), _lib.ptr(gH),
                                       _lib.ptr(gS) if overlap else None, _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()
    return unguard(bH, "gH"), (unguard(bS, "gS") if overlap else unguard(bS, "gS", full=False))


def level_unit(m, ev, kappa):
    return max(FR.level_unit(m, ev[-1] - ev[0], kappa), 2.0 ** -52 * float(np.abs(ev).max()))


# ---- 1. the ragged batch through the C ABI -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_reference():
    """Every m of SIZES with n_occ = 0, 1, m / 2, m - 1, m (shuffled), a generalized problem with kappa_2(S) of about 1e2: per molecule H, S, Z, Ht, the levels of
    ``eigh``, the exact projector, and the restatement's sides on the exact projector and on its own SP2 projector."""
    cases = [(m, n) for m in SIZES for n in sorted({0, 1, m // 2, m - 1, m}) if 0 <= n <= m]
    order = np.random.Generator(np.random.PCG64(77)).permutation(len(cases))
    out = []
    for i in order:
        m, n = cases[i]
        rng = np.random.default_rng(500 + 10 * m + n)
        A, _ = FR.random_hamiltonian(rng, m, n, gap=0.3 if (m + n) % 2 == 0 else 0.01)
        if m == 1:
            A = np.array([[-3.5 + n]])                               # one level, not zero: the unit is an ulp of it
        S = DR.overlap(m, 1e2, np.random.Generator(np.random.PCG64(900 + m + n)))
        L = np.linalg.cholesky(S)
        H = PR.lower_sym(L @ A @ L.T)
        Z = PR.orthogonalizer(S)
        Ht = PR.congruence(Z, H, False)
        Xe, ev, U = FR.exact_projector(Ht, n)
        e_min, e_max = PR.bounds(Ht)
        sol = PR.purify(Ht, n)
        r = dict(m=m, n=n, H=H, S=S, Z=Z, Ht=Ht, Xe=Xe, ev=ev, U=U, shift=(e_min, e_max), kappa=float(np.linalg.cond(S)))
        r["exact"] = [FR.side(Ht, Xe, e_min, e_max, n, w, W=Z) for w in (FR.HOMO, FR.LUMO)]
        r["sp2"] = [FR.side(Ht, sol["X"], sol["e_min"], sol["e_max"], n, w, W=Z) for w in (FR.HOMO, FR.LUMO)]
        out.append(r)
    return out


def check_sides(tag, refs, got, which):
    """Levels, vectors, coefficients, step counts and flags of a launch against eigh and the restatement -> the worst figures."""
    worst = np.zeros(5)
    o = 0
    for b, r in enumerate(refs):
        m, n = r["m"], r["n"]
        u = level_unit(m, r["ev"], r["kappa"])
        for w, k in ((FR.HOMO, n - 1), (FR.LUMO, n)):
            ref = r[which][w]
            v, c = got["vec"][w, o:o + m], got["coef"][w, o:o + m]
            assert got["conv"][b, w] == ref["conv"], (tag, b, m, n, w, got["conv"][b, w])
            if ref["conv"] != 1:
                assert ref["conv"] == -1 and got["iters"][b, w] == 0 and np.isnan(got["eps"][b, w]) and np.isnan(got["res"][b, w]) and np.isnan(v).all() and np.isnan(c).all()
                continue
            sep = FR.separation(r["ev"], k)
            uk, ck = r["U"][:, k], r["Z"].T @ r["U"][:, k]
            fig = [abs(got["eps"][b, w] - r["ev"][k]) / u, np.abs(np.outer(v, v) - np.outer(uk, uk)).max() / (u / sep * np.abs(np.outer(uk, uk)).max()),
                   np.abs(np.outer(c, c) - np.outer(ck, ck)).max() / (u / sep * np.abs(np.outer(ck, ck)).max()), abs(c @ r["S"] @ c - 1.0) / (m * 2.0 ** -52 * r["kappa"]),
                   abs(int(got["iters"][b, w]) - ref["iters"])]
            worst = np.maximum(worst, fig)
            assert max(fig[:4]) <= BOUND and fig[4] <= 2, (tag, b, m, n, w, fig, int(got["iters"][b, w]), ref["iters"])
            assert abs(v @ v - 1.0) <= 16 * 2.0 ** -52 and got["res"][b, w] <= TOL * (r["shift"][1] - r["shift"][0]) * (1 + 1e-12)
            dim = n if w == FR.HOMO else m - n
            if dim == 1:
                assert got["iters"][b, w] <= 2, (tag, b, m, n, w)           # one step, or one more for the leaked direction
            assert got["iters"][b, w] <= min(m, 2 * dim + 1), (tag, b, m, n, w)   # Krylov exhaustion at dim + 1 at the latest in exact arithmetic
        o += m
    print(f"orbital_frontier_parity {tag}: worst level {worst[0]:.3g} U_eps, vec vec^T {worst[1]:.3g} U_g, coef coef^T {worst[2]:.3g} U_g, c^T S c - 1 {worst[3]:.3g} "
          f"m 2^-52 kappa, |iters - restatement| {int(worst[4])} (bounds {BOUND:g} {BOUND:g} {BOUND:g} {BOUND:g} 2)")
    return worst


def test_ragged_batch_with_an_uploaded_exact_projector():
    """The kernel without SP2: Ht, the projector of ``eigh``, the Gershgorin bounds and Z come from numpy."""
    refs = ragged_reference()
    ms, nos = [r["m"] for r in refs], [r["n"] for r in refs]
    pur, _ = purification(ms)
    got = raw_lanczos(pur.state, dev(pack([r["Ht"] for r in refs])), dev(pack([r["Xe"] for r in refs])), dev(np.array([r["shift"] for r in refs])), nos,
                      dev(pack([r["Z"] for r in refs])))
    check_sides("C ABI, exact projector, ragged m = 1..130", refs, got, "exact")
    again = raw_lanczos(pur.state, dev(pack([r["Ht"] for r in refs])), dev(pack([r["Xe"] for r in refs])), dev(np.array([r["shift"] for r in refs])), nos, None)
    for k in ("eps", "vec", "res"):
        assert same_bits(np.nan_to_num(again[k], nan=-1.0), np.nan_to_num(got[k], nan=-1.0)), k       # W only makes coef
    assert same_bits(np.nan_to_num(again["coef"], nan=-1.0), np.nan_to_num(again["vec"], nan=-1.0))   # W = NULL: coef = vec


def test_ragged_batch_after_the_purification():
    refs = ragged_reference()
    ms, nos = [r["m"] for r in refs], [r["n"] for r in refs]
    pur, _ = purification(ms)
    pur.orthogonalize(dev(pack([r["S"] for r in refs])))
    pur.purify(dev(pack([r["H"] for r in refs])), nos).check()
    st = pur.state
    got = raw_lanczos(st, st.work, st.coeff, pur.ctl[:, :2].contiguous(), nos, pur.orthogonalizer.Z)
    check_sides("C ABI, SP2 projector, ragged m = 1..130", refs, got, "sp2")
    lv = pur.frontier()
    pur.frontier_check(lv)
    assert same_bits(np.nan_to_num(torch.stack((lv.homo, lv.lumo), 1).cpu().numpy(), nan=-1.0), np.nan_to_num(got["eps"], nan=-1.0))
    assert same_bits(np.nan_to_num(lv.coeff.cpu().numpy(), nan=-1.0), np.nan_to_num(got["coef"], nan=-1.0))
    assert np.array_equal(lv.converged.cpu().numpy(), got["conv"]) and np.array_equal(lv.iterations.cpu().numpy(), got["iters"])
    gap = lv.gap.cpu().numpy()
    assert all(np.isnan(gap[b]) == (r["n"] in (0, r["m"])) for b, r in enumerate(refs))


def test_one_molecule_at_the_largest_size():
    """m = 1024, n_occ = 200, an uploaded exact projector, k_max = 256 (the restatement needs about 97 / 177 steps)."""
    rng = np.random.default_rng(1024)
    m, n = 1024, 200
    Ht, _ = FR.random_hamiltonian(rng, m, n, gap=0.3)
    Xe, ev, U = FR.exact_projector(Ht, n)
    e_min, e_max = PR.bounds(Ht)
    ref = [FR.side(Ht, Xe, e_min, e_max, n, w, tol=2.0 ** -40) for w in (FR.HOMO, FR.LUMO)]
    pur, _ = purification([m])
    got = raw_lanczos(pur.state, dev(Ht.reshape(-1)), dev(Xe.reshape(-1)), dev(np.array([[e_min, e_max]])), [n], None, k_max=256, tol=2.0 ** -40)
    u = level_unit(m, ev, 1.0)
    fig = [abs(got["eps"][0, w] - ev[k]) / u for w, k in ((0, n - 1), (1, n))]
    print(f"orbital_frontier_parity m=1024 n_occ=200 k_max=256 tol=2^-40: steps {got['iters'][0].tolist()} (restatement {[r['iters'] for r in ref]}), levels {fig[0]:.3g} "
          f"{fig[1]:.3g} U_eps (bound {BOUND:g})")
    assert got["conv"][0].tolist() == [1, 1] and [r["conv"] for r in ref] == [1, 1] and max(fig) <= BOUND
    assert all(abs(int(got["iters"][0, w]) - ref[w]["iters"]) <= 2 for w in (0, 1))
    for w, k in ((0, n - 1), (1, n)):
        v = got["vec"][w]
        assert np.abs(np.outer(v, v) - np.outer(U[:, k], U[:, k])).max() <= BOUND * u / FR.separation(ev, k) + 2.0 ** -40 * (e_max - e_min) / FR.separation(ev, k)


# ---- 2. failures and edges -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_side_that_needs_more_than_k_max_steps_is_alone_in_its_nan():
    rng = np.random.default_rng(130)
    cases = [(130, 3), (17, 5)]
    Hs = [FR.random_hamiltonian(rng, m, n)[0] for m, n in cases]
    ms, nos = [c[0] for c in cases], [c[1] for c in cases]
    pur, _ = purification(ms)
    pur.purify(dev(pack(Hs)), nos).check()
    lv = pur.frontier(k_max=8)
    conv, it = lv.converged.cpu().numpy(), lv.iterations.cpu().numpy()
    assert conv.tolist() == [[1, 0], [1, 0]] and it[0, 1] == 8 and it[1, 1] == 8 and it[0, 0] <= 6
    ev = np.linalg.eigvalsh(Hs[0])
    assert abs(float(lv.homo[0]) - ev[2]) <= BOUND * level_unit(130, ev, 1.0)
    assert bool(torch.isnan(lv.lumo).all()) and bool(torch.isnan(lv.gap).all()) and bool(torch.isnan(lv.residual[:, 1]).all())
    assert bool(torch.isnan(lv.coeff[1]).all()) and bool(torch.isnan(lv.vectors[1]).all()) and bool(torch.isfinite(lv.coeff[0]).all())
    with pytest.raises(RuntimeError, match=r"molecule 0: the LUMO did not converge in 8 Lanczos steps \(k_max=8, m=130\)"):
        pur.frontier_check(lv)
    one = torch.ones(2, dtype=torch.float64, device=DEV)
    gH, gS = pur.frontier_gradients(lv, one, None, overlap=False)   # a side with conv = 0 poisons its molecule's blocks, whatever its weight
    assert bool(torch.isnan(gH).all()) and gS is None
    full = pur.frontier(k_max=256)
    pur.frontier_check(full)
    assert same_bits(full.homo.cpu().numpy(), lv.homo.cpu().numpy())     # the HOMO side did not notice


def test_failed_molecules_equal_top_levels_reproducibility_and_batch_independence():
    rng = np.random.default_rng(33)
    m, n = 37, 9
    lev = np.concatenate([np.sort(rng.uniform(-20.0, -0.2, n)), np.sort(rng.uniform(0.2, 2.0, m - n))])
    lev[n - 2] = lev[n - 1]                                           # two equal top occupied levels
    Q = np.linalg.qr(rng.standard_normal((m, m)))[0]
    Hdeg = PR.lower_sym((Q * lev) @ Q.T)
    good = [(65, 21, 0.3, 1e2, 2), (17, 5, 0.3, 1e2, 1), (130, 43, 0.3, 1e4, 99)]
    pairs = [DR.gapped_case(*c) for c in good]
    bad_S = np.eye(20)
    bad_S[7, 7] = -1.0                                               # not positive definite: status 1
    Hs = [pairs[0][0], gapless(33, 11, 7), pairs[1][0], np.diag(np.arange(20.0)), pairs[2][0], Hdeg]
    Ss = [pairs[0][1], np.eye(33), pairs[1][1], bad_S, pairs[2][1], np.eye(m)]
    ms, nos = [h.shape[0] for h in Hs], [21, 11, 5, 5, 43, n]

    def run(sel):
        pur, _ = purification([ms[b] for b in sel])
        pur.orthogonalize(dev(pack([Ss[b] for b in sel])))
        pur.purify(dev(pack([Hs[b] for b in sel])), [nos[b] for b in sel])
        lv = pur.frontier()
        g = torch.ones(len(sel), dtype=torch.float64, device=DEV)
        gH, gS = pur.frontier_gradients(lv, -g, g)
        return pur, lv, blocks(gH.cpu().numpy(), [ms[b] for b in sel]), blocks(gS.cpu().numpy(), [ms[b] for b in sel])
    pur, lv, gH, gS = run(range(6))
    assert pur.status.cpu().tolist() == [0, 4, 0, 1, 0, 0]
    eps, conv = torch.stack((lv.homo, lv.lumo), 1).cpu().numpy(), lv.converged.cpu().numpy()
    assert conv.tolist() == [[1, 1], [0, 0], [1, 1], [0, 0], [1, 1], [1, 1]]
    off = np.concatenate([[0], np.cumsum(ms)])
    cf = lv.coeff.cpu().numpy()
    for b in (1, 3):                                                 # each alone in its NaN
        assert np.isnan(eps[b]).all() and np.isnan(cf[:, off[b]:off[b + 1]]).all() and np.isnan(gH[b]).all() and np.isnan(gS[b]).all()
    for b in (0, 2, 4, 5):
        assert np.isfinite(eps[b]).all() and np.isfinite(cf[:, off[b]:off[b + 1]]).all() and np.isfinite(gH[b]).all() and np.isfinite(gS[b]).all()
        assert same_bits(gH[b], gH[b].T) and same_bits(gS[b], gS[b].T)
    with pytest.raises(RuntimeError, match="molecule 1: the purification did not converge"):
        pur.frontier_check(lv)
    u = level_unit(m, lev, 1.0)
    print(f"orbital_frontier_parity equal top occupied levels m={m}: HOMO {abs(eps[5, 0] - lev[n - 1]) / u:.3g} LUMO {abs(eps[5, 1] - lev[n]) / u:.3g} U_eps")
    assert abs(eps[5, 0] - lev[n - 1]) <= BOUND * u and abs(eps[5, 1] - lev[n]) <= BOUND * u          # the level only: v v^T is not unique
    _, lv2, gH2, gS2 = run(range(6))                                 # bitwise reproducible
    for a, b in ((lv.homo, lv2.homo), (lv.lumo, lv2.lumo), (lv.coeff, lv2.coeff), (lv.vectors, lv2.vectors), (lv.residual, lv2.residual)):
        assert same_bits(np.nan_to_num(a.cpu().numpy(), nan=-1.0), np.nan_to_num(b.cpu().numpy(), nan=-1.0))
    assert np.array_equal(lv.iterations.cpu().numpy(), lv2.iterations.cpu().numpy())
    for b in (0, 4, 5):                                              # alone: the same bits as between failed neighbours
        _, la, gHa, gSa = run([b])
        assert same_bits(la.homo.cpu().numpy(), eps[b:b + 1, 0]) and same_bits(la.lumo.cpu().numpy(), eps[b:b + 1, 1]), b
        assert same_bits(la.coeff.cpu().numpy(), cf[:, off[b]:off[b + 1]]) and same_bits(gHa[0], gH[b]) and same_bits(gSa[0], gS[b]), b
        assert np.array_equal(la.iterations.cpu().numpy()[0], lv.iterations.cpu().numpy()[b])


def test_gram_is_exact_on_integers_and_exactly_symmetric():
    ms = [65, 1, 17, 130, 64, 3]
    rng = np.random.Generator(np.random.PCG64(4))
    M, B = sum(ms), len(ms)
    coef = rng.integers(-3, 4, size=(2, M)).astype(np.float64)
    g = rng.integers(-4, 5, size=(B, 2)).astype(np.float64)
    eps = rng.integers(-5, 6, size=(B, 2)).astype(np.float64)
    conv = np.array([[1, 1], [1, -1], [-1, 1], [1, 1], [1, 0], [-1, -1]])
    coef[1, 65:66] = np.nan                                          # what the kernel leaves for an absent level: must not be read
    coef[0, 66:83] = np.nan
    pur, _ = purification(ms)
    gH, gS = raw_gram(pur.state, g, eps, coef, conv)
    gH2, none = raw_gram(pur.state, g, eps, coef, conv, overlap=False)
    assert same_bits(np.nan_to_num(gH, nan=-1.0), np.nan_to_num(gH2, nan=-1.0)) and np.all(none == SENTINEL)
    o = 0
    for b, (m, h, s) in enumerate(zip(ms, blocks(gH, ms), blocks(gS, ms))):
        if 0 in conv[b]:
            assert np.isnan(h).all() and np.isnan(s).all(), b
        else:
            rH, rS = np.zeros((m, m)), np.zeros((m, m))
            for w in (0, 1):
                if conv[b, w] == 1:
                    cc = np.outer(coef[w, o:o + m], coef[w, o:o + m])
                    rH += g[b, w] * cc
                    rS -= g[b, w] * eps[b, w] * cc
            assert np.array_equal(h, rH) and np.array_equal(s + 0.0, rS + 0.0), b
        o += m
    # random data: exactly symmetric
    coef = rng.normal(size=(2, M))
    gH, gS = raw_gram(pur.state, rng.normal(size=(B, 2)), rng.normal(size=(B, 2)), coef, np.ones((B, 2)))
    for h, s in zip(blocks(gH, ms), blocks(gS, ms)):
        assert same_bits(h, h.T) and same_bits(s, s.T)


def test_dimension_mismatch_touches_nothing_and_python_refusals():
    from nabladft_amd import _lib
    ms = [5, 3]
    pur, op = purification(ms)
    Hs = [np.diag(np.arange(5.0)), np.diag(np.arange(3.0))]
    pur.purify(dev(pack(Hs)), [2, 1])
    st, lib = pur.state, _lib.load()
    arrays = [torch.full((80,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(6)]
    ints = [torch.full((8,), -77, dtype=torch.int32, device=DEV) for _ in range(2)]
    vp = dev(vlayout(ms, 256))
    p = [_lib.ptr(a) for a in arrays]
    shift, no = pur.ctl[:, :2].contiguous(), i32([2, 1])
    wrong = (2, 8, 36)                                               # instead of (2, 8, 34)
    X = st.coeff.clone()
    assert lib.nq_orb_front_lanczos(_lib.ptr(st.buf), *wrong, _lib.ptr(st.work), _lib.ptr(st.coeff), _lib.ptr(shift), _lib.ptr(no), None, 256, TOL, p[0], _lib.ptr(vp), p[1], p[2],
                                    p[3], _lib.ptr(ints[0]), p[4], _lib.ptr(ints[1]), _lib.stream_ptr()) == 0, lib.nq_last_error()
    torch.cuda.synchronize()
    assert int(st.header_dev[4]) == -2 and all(bool((a == SENTINEL).all()) for a in arrays) and all(bool((t == -77).all()) for t in ints)
    with pytest.raises(RuntimeError, match="other dimensions"):
        st.header()
    st.header_dev[4] = 0
    coef = torch.zeros(16, dtype=torch.float64, device=DEV)
    assert lib.nq_orb_front_gram(_lib.ptr(st.buf), *wrong, _lib.ptr(shift), _lib.ptr(shift), _lib.ptr(coef), _lib.ptr(no), p[0], p[1], _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(st.header_dev[4]) == -2 and all(bool((a == SENTINEL).all()) for a in arrays) and torch.equal(X.view(torch.int64), st.coeff.view(torch.int64))
    st.header_dev[4] = 0
    # a workspace slice that is too small: conv 0 and NaN, nothing written behind it
    small = dev(np.array([0, 10, 20], dtype=np.int64))
    assert lib.nq_orb_front_lanczos(_lib.ptr(st.buf), *st._dims, _lib.ptr(st.work), _lib.ptr(st.coeff), _lib.ptr(shift), _lib.ptr(no), None, 256, TOL, p[0], _lib.ptr(small), p[1],
                                    p[2], p[3], _lib.ptr(ints[0]), p[4], _lib.ptr(ints[1]), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((arrays[0] == SENTINEL).all()) and ints[1][:4].cpu().tolist() == [0, 0, 0, 0] and bool(torch.isnan(arrays[1][:4]).all())
    # Python
    with pytest.raises(ValueError, match="k_max"):
        pur.frontier(k_max=0)
    with pytest.raises(ValueError, match="k_max"):
        pur.frontier(k_max=1025)
    with pytest.raises(ValueError, match="tol"):
        pur.frontier(tol=0.0)
    with pytest.raises(ValueError, match="transform"):
        pur.frontier(transform=torch.zeros(3, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="purify"):
        purification(ms)[0].frontier()
    import nabladft_amd as nq
    with pytest.raises(ValueError, match="another batch"):
        nq.purified_frontier(dev(pack(Hs)), None, [0, 8], [2], solution=pur)
    with pytest.raises(ValueError, match="orthogonalizer without"):
        nq.purified_frontier(dev(pack(Hs)), None, op, [2, 1], orthogonalizer=pur.orthogonalize(dev(pack([np.eye(5), np.eye(3)]))))


# ---- 3. through Python: the gradients --------------------------------------------------------------------------------------------------------------------------------
GENERAL = [c for c in DR.CASES if 1 <= c[1] < c[0]]
G_HOMO, G_LUMO = -0.7, 1.3


@functools.lru_cache(maxsize=None)
def autograd_reference(inputs):
    """Per case of GENERAL: (H, S) rounded as the inputs are, the levels and the symmetrised gradients of ``G_HOMO homo + G_LUMO lumo`` by ``torch.linalg``."""
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
        (G_HOMO * e[n - 1] + G_LUMO * e[n]).backward()
        ev = e.detach().numpy()
        out.append(dict(m=m, n=n, H=H, S=S, ev=ev, gH=sym(Ht.grad.numpy()), gS=sym(St.grad.numpy()), kappa=1.0 if S is None else float(np.linalg.cond(S))))
    return out


def gradient_units(r, coefs, eps):
    """(U_eps, U_g of gH, U_g of gS) from the device's own coefficient vectors ``coefs`` = (c_homo, c_lumo)."""
    u = level_unit(r["m"], r["ev"], r["kappa"])
    uH = sum(u / FR.separation(r["ev"], k) * np.abs(g * np.outer(c, c)).max() for c, k, g in zip(coefs, (r["n"] - 1, r["n"]), (G_HOMO, G_LUMO)))
    uS = sum(u / FR.separation(r["ev"], k) * np.abs(g * e * np.outer(c, c)).max() for c, k, g, e in zip(coefs, (r["n"] - 1, r["n"]), (G_HOMO, G_LUMO), eps))
    return u, uH, uS


@pytest.mark.parametrize("inputs", ["float64", "float32", "standard", "transform"])
def test_purified_frontier_gradients_against_torch_autograd(inputs):
    import nabladft_amd as nq
    refs = autograd_reference("float64" if inputs == "transform" else inputs)
    ms, nos = [r["m"] for r in refs], [r["n"] for r in refs]
    op = np.concatenate([[0], np.cumsum(ms)])
    dt = np.float32 if inputs == "float32" else np.float64
    Hd = dev(pack([r["H"] for r in refs], dtype=dt)).requires_grad_(True)
    Sd = None if inputs == "standard" else dev(pack([r["S"] for r in refs], dtype=dt)).requires_grad_(True)
    if inputs == "transform":                                        # S^(-1/2) by Newton-Schulz, SP2 on the standard problem, the back-transform handed in
        target = nq.scf_target_iterative(Hd.detach(), Sd.detach(), op, nos).check()
        pur = target.purification
        lv = pur.frontier(transform=target.basis.inv_half)
        pur.frontier_check(lv)
        B = len(ms)
        gH, gS = pur.frontier_gradients(lv, torch.full((B,), G_HOMO, dtype=torch.float64, device=DEV), torch.full((B,), G_LUMO, dtype=torch.float64, device=DEV))
        homo, lumo = lv.homo, lv.lumo
    else:
        homo, lumo, pur = nq.purified_frontier(Hd, Sd, op, nos, return_solution=True)
        pur.frontier_check(pur.levels)
        lv = pur.levels
        (G_HOMO * homo.sum() + G_LUMO * lumo.sum()).backward()
        assert Hd.grad.dtype == Hd.dtype and Hd.grad.shape == Hd.shape and (Sd is None or (Sd.grad.dtype == Sd.dtype and Sd.grad.shape == Sd.shape))
        gH, gS = Hd.grad.double(), None if Sd is None else Sd.grad.double()
    eh, el, cf = homo.detach().cpu().numpy(), lumo.detach().cpu().numpy(), lv.coeff.cpu().numpy()
    gHb, gSb = blocks(gH.cpu().numpy(), ms), None if gS is None else blocks(gS.cpu().numpy(), ms)
    worst, o = np.zeros(4), 0
    for b, r in enumerate(refs):
        m, n = r["m"], r["n"]
        u, uH, uS = gradient_units(r, (cf[0, o:o + m], cf[1, o:o + m]), (eh[b], el[b]))
        r32 = 2.0 ** -24 if inputs == "float32" else 0.0              # the gradients are cast to the inputs' dtype
        fig = [abs(eh[b] - r["ev"][n - 1]) / u, abs(el[b] - r["ev"][n]) / u, np.abs(gHb[b] - r["gH"]).max() / (uH + r32 * np.abs(r["gH"]).max())]
        if gSb is not None:
            fig.append(np.abs(gSb[b] - r["gS"]).max() / (uS + r32 * np.abs(r["gS"]).max()))
            assert same_bits(gSb[b], gSb[b].T)
        assert same_bits(gHb[b], gHb[b].T) and max(fig) <= BOUND, (inputs, b, m, n, fig)
        worst[:len(fig)] = np.maximum(worst[:len(fig)], fig)
        o += m
    print(f"orbital_frontier_parity purified_frontier {inputs}: worst HOMO {worst[0]:.3g} LUMO {worst[1]:.3g} U_eps, gH {worst[2]:.3g} gS {worst[3]:.3g} U_g "
          f"against torch.linalg autograd (bound {BOUND:g})")


def test_nothing_is_launched_without_an_upstream_gradient_and_the_overlap_half_is_skipped(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedPurification, OrbitalState
    r = autograd_reference("float64")[2]
    calls = []
    real = BatchedPurification.frontier_gradients
    monkeypatch.setattr(BatchedPurification, "frontier_gradients", lambda self, lv, gh, gl, overlap=True: (calls.append((gh is not None, gl is not None, overlap)),
                                                                                                          real(self, lv, gh, gl, overlap))[1])
    op = [0, r["m"]]
    Hd, Sd = dev(r["H"].reshape(-1)).requires_grad_(True), dev(r["S"].reshape(-1))
    homo, lumo = nq.purified_frontier(Hd, Sd, op, [r["n"]])
    assert calls == []
    lumo.sum().backward()                                            # the HOMO has no upstream gradient; S asks for nothing
    assert calls == [(False, True, False)] and bool(torch.isfinite(Hd.grad).all())
    D, sol = nq.purified_density_matrix(Hd, Sd, op, [r["n"]], return_solution=True)
    runs = []
    real_call = OrbitalState.call
    monkeypatch.setattr(OrbitalState, "call", lambda self, name, *a: (runs.append(name), real_call(self, name, *a))[1])
    h2, l2 = nq.purified_frontier(Hd, Sd, op, [r["n"]], solution=sol)
    assert runs == ["nq_orb_front_lanczos"]                          # the shared solution is not purified again
    assert same_bits(h2.detach().cpu().numpy(), homo.detach().cpu().numpy()) and same_bits(l2.detach().cpu().numpy(), lumo.detach().cpu().numpy())


# ---- 4. against the solver route --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["synthetic", "database"])
def test_levels_against_the_solver(which):
    import nabladft_amd as nq
    if which == "synthetic":
        probs = [DR.gapped_case(*c) + (c[1],) for c in GENERAL]
    else:
        probs = []
        for H, S, z in db_problems()[:5]:                             # the sixth molecule's overlap is indefinite (tests/test_orbital_lowdin_gpu.py)
            probs.append((H, S, int(nq.occupied_counts(np.asarray(z, dtype=np.int64), [0, len(z)], 0)[0])))
    ms, nos = [p[0].shape[0] for p in probs], [p[2] for p in probs]
    op = np.concatenate([[0], np.cumsum(ms)])
    Hd, Sd = dev(pack([p[0] for p in probs])), dev(pack([p[1] for p in probs]))
    homo, lumo, pur = nq.purified_frontier(Hd, Sd, op, nos, return_solution=True)
    pur.frontier_check(pur.levels)
    sh, sl, sg = nq.BatchedOrbitals(op, DEV).solve(Hd, Sd).frontier(nos)
    worst = 0.0
    for b, (H, S, n) in enumerate(probs):
        L = np.linalg.cholesky(S)
        ev = np.linalg.eigvalsh(sym(np.linalg.solve(L, np.linalg.solve(L, H).T).T))
        u = level_unit(ms[b], ev, float(np.linalg.cond(S)))
        fig = [abs(float(homo[b]) - float(sh[b])) / u, abs(float(lumo[b]) - float(sl[b])) / u, abs(float(homo[b]) - ev[n - 1]) / u, abs(float(lumo[b]) - ev[n]) / u]
        worst = max(worst, max(fig))
        print(f"orbital_frontier_parity levels {which} {b} m={ms[b]} n_occ={n} gap {ev[n] - ev[n - 1]:.3f} steps {pur.levels.iterations[b].tolist()}: against the solver "
              f"{fig[0]:.3g} {fig[1]:.3g}, against numpy {fig[2]:.3g} {fig[3]:.3g} U_eps (bound {BOUND:g})")
        assert max(fig) <= BOUND, (which, b, fig)
    gap = pur.levels.gap.cpu().numpy()
    assert np.array_equal(gap, (lumo - homo).detach().cpu().numpy())


# ---- 5. the QHNet task ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_purified_frontier_task(monkeypatch):
    """One training step with a gap term and a density term: no solve, one orthogonaliser, one purification of the prediction (and one of the target), finite
    loss, gradients at the parameters; and with ``FrontierLoss("mae", "both")`` alone the loss of ``QHNetOrbitalLightning`` with
    ``OrbitalEnergyLoss("mae", "frontier")``: the four levels per molecule are each within 10 U_eps of the solver's, so the two means of absolute differences are
    within 20 U_eps (mean over the molecules) of each other, plus the float32 sum of the two terms (1e-6 relative, the tolerance of the sibling tests)."""
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
    counts = dict(solve=0, orth=0)
    launches = []
    real_solve, real_orth, real_call = OrbitalState.solve, BatchedPurification.orthogonalize, OrbitalState.call
    monkeypatch.setattr(OrbitalState, "solve", lambda self, *a, **k: (counts.__setitem__("solve", counts["solve"] + 1), real_solve(self, *a, **k))[1])
    monkeypatch.setattr(BatchedPurification, "orthogonalize", lambda self, *a, **k: (counts.__setitem__("orth", counts["orth"] + 1), real_orth(self, *a, **k))[1])
    monkeypatch.setattr(OrbitalState, "call", lambda self, name, *a: (launches.append(name), real_call(self, name, *a))[1])
    params = [p for p in net.parameters() if p.requires_grad]

    def step(task):
        for p in params:
            p.grad = None
        loss = task.training_step(batch, 0)
        loss.backward()
        return loss.detach().double()
    losses = {"hamiltonian": HamiltonianLoss(), "frontier": nq.FrontierLoss("mae", "gap", charge), "density_matrix": nq.DensityMatrixLoss("mse", charge)}
    coefs = {"hamiltonian": 1.0, "frontier": 0.7, "density_matrix": 0.5}
    loss = step(make(nq.QHNetPurifiedFrontierLightning, losses, coefs))
    assert counts == dict(solve=0, orth=1), counts                   # no nq_orb_solve; ONE orthogonaliser for prediction and target
    assert launches.count("nq_orb_pur_run") == 2 and launches.count("nq_orb_front_lanczos") == 2      # target and prediction, each purified once
    assert launches.count("nq_orb_front_gram") == 1
    assert bool(torch.isfinite(loss)) and sum(1 for p in params if p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0) > 0
    # the same levels as the solver's, in the loss
    both = {"hamiltonian": HamiltonianLoss(), "frontier": nq.FrontierLoss("mae", "both", charge)}
    task = make(nq.QHNetPurifiedFrontierLightning, both, {"hamiltonian": 1.0, "frontier": 0.7})
    lp = step(task)
    assert counts["solve"] == 0
    solver = {"hamiltonian": HamiltonianLoss(), "orbital_energies": nq.OrbitalEnergyLoss("mae", "frontier", charge)}
    ls = step(make(nq.QHNetOrbitalLightning, solver, {"hamiltonian": 1.0, "orbital_energies": 0.7}))
    assert counts["solve"] == 2
    preds, targets, _ = task._evaluate(batch)
    units = []
    for b, m in enumerate(ms):
        S = PR.lower_sym(batch.overlap[b].astype(np.float64))
        L = np.linalg.cholesky(S)
        for Hb in (PR.lower_sym(batch.hamiltonian[b].astype(np.float64)), PR.lower_sym(blocks(preds["hamiltonian"].detach().double().cpu().numpy(), ms)[b])):
            ev = np.linalg.eigvalsh(sym(np.linalg.solve(L, np.linalg.solve(L, Hb).T).T))
            units.append(level_unit(m, ev, float(np.linalg.cond(S))))
    allow = 0.7 * 2.0 * BOUND * float(np.mean(units)) * 2.0 + 1e-6 * float(ls.abs())
    print(f"orbital_frontier_parity qhnet task loss with the gap and density terms {float(loss):.9g}; FrontierLoss(mae, both) {float(lp):.9g} against "
          f"QHNetOrbitalLightning with OrbitalEnergyLoss(mae, frontier) {float(ls):.9g} (allowed difference {allow:.3g})")
    assert abs(float(lp) - float(ls)) <= allow
    # the parent's refusal stays; with the coefficient at 0 the step is the parent's
    with_e = dict(both, orbital_energies=nq.OrbitalEnergyLoss("mae", "occupied", charge))
    with pytest.raises(ValueError, match="no orbital energies"):
        make(nq.QHNetPurifiedFrontierLightning, with_e, {"hamiltonian": 1.0, "frontier": 0.7, "orbital_energies": 0.25}).training_step(batch, 0)
    dens = {"hamiltonian": HamiltonianLoss(), "frontier": nq.FrontierLoss("mae", "gap", charge), "density_matrix": nq.DensityMatrixLoss("mse", charge)}
    zero = {"hamiltonian": 1.0, "frontier": 0.0, "density_matrix": 0.5}
    before = len(launches)
    a = make(nq.QHNetPurifiedFrontierLightning, dens, zero).training_step(batch, 0)
    mine = launches[before:]
    del dens["frontier"], zero["frontier"]                           # the parent does not know the key
    b = make(nq.QHNetPurifiedDensityLightning, dens, zero).training_step(batch, 0)
    assert torch.equal(a.detach(), b.detach()) and "nq_orb_front_lanczos" not in mine and mine == launches[before + len(mine):]
