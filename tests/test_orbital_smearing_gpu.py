"""GPU: Fermi-smeared occupations and their gradient chain (csrc/orbsmear.hip) through the C ABI, and ``smeared_solution`` / ``QHNetSmearedDensityLightning`` of
nabladft_amd.orbital_loss end to end against the float64 yardstick (tests/orbital_smearing_ref.py, whose own spread tests/test_orbital_smearing_cpu.py pins).

Bounds.  ``nq_orb_fermi`` against the numpy bisection on the device's own eps: |sum F - n_elec| <= (m + 4) 2^-53 n_elec, |mu - mu_ref| <= 2 (m + 4) 2^-53 n_elec /
|sum F'| + 2 ulp(mu), occ / docc / entropy within 4 x the measured figures of the header's functions (tests/test_orbsmear_host_cpu.py) of numpy at the device's
mu (the entropy, a sum of m terms, gets the dot-product bound on top).  Product steps, on coefficients and energies written into the state (no solve), each
against numpy on the same operands: |x - ref| <= (K + 4) 2^-53 sum |terms|, K the contraction length; the MO step adds the epilogue's figure times |K W|; the
diagonal step, a few sums of m terms of header functions, is held to the same (m + 4) 2^-53 times the sum of the magnitudes of its terms.  End to end, with the device
solver: max(10, 4 x the spread of the two reference routes) in the units of orbital_smearing_ref.units, the module's rule.  Float32 results are allowed their
own rounding, 2^-24 per element.  Every figure is printed as an ``orbital_smearing_parity ...`` line (kept in profiles/orbital_smearing_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_smearing_ref as SR
import orbitals_ref as R
from test_orbital_loss_gpu import blocks, state_with
from test_orbitals_gpu import BOUND, DEV, dev, pack, ptrs
from test_orbsmear_host_cpu import MEASURED_ULP

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SENTINEL = -7.25e300
GUARD = 64
HDR = {k: 4.0 * v for k, v in MEASURED_ULP.items()}                # the header's functions on the device against numpy, in units of 2^-53


# ---- the solved batches: every case of the yardstick in one ragged batch, solved once -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problems(inputs):
    """[(case, H, S, n_elec, kT)] of the non-coincident cases as the device sees them."""
    out = []
    for case in SR.CASES:
        m, no, gap, k0, seed, ne, kT = case
        H, S = DR.gapped_case(m, no, gap, k0, seed, standard=inputs == "standard")
        if inputs == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        out.append((case, H, S, ne, kT))
    return out


@functools.lru_cache(maxsize=None)
def coincident():
    return [((m, no, seed, ne, kT, kind),) + SR.coincident_case(m, no, seed, kind) + (ne, kT) for m, no, seed, ne, kT, kind in SR.COINCIDENT]


@pytest.fixture(scope="module")
def solved():
    from nabladft_amd import BatchedOrbitals
    pr = problems("float64")
    Hs, Ss = [p[1] for p in pr], [p[2] for p in pr]
    op, pp = ptrs(Hs)
    orb = BatchedOrbitals(op, DEV).solve(dev(pack(Hs)), dev(pack(Ss))).check()
    return orb, op, pp, np.array([p[3] for p in pr]), np.array([p[4] for p in pr])


# ---- 1. nq_orb_fermi ---------------------------------------------------------------------------------------------------------------------------------------------
def fermi_host(fr):
    return [t.cpu().numpy() for t in (fr.mu, fr.occ, fr.docc, fr.entropy, fr.info)]


def test_fermi_against_the_numpy_bisection(solved):
    from nabladft_amd import BatchedOrbitals
    orb, op, pp, ne, kT = solved
    fr = orb.fermi(ne, kT)
    mu, occ, docc, ent, info = fermi_host(fr)
    eps = orb.energies.cpu().numpy()
    assert not info.any()
    worst = np.zeros(5)
    for b in range(len(ne)):
        e, F, dF = eps[op[b]:op[b + 1]], occ[op[b]:op[b + 1]], docc[op[b]:op[b + 1]]
        m = e.shape[0]
        mu_ref, _, dF_ref, _ = SR.fermi(e, ne[b], kT[b])
        f_sum = abs(F.sum() - ne[b]) / ((m + 4) * U * ne[b])
        f_mu = abs(mu[b] - mu_ref) / (2 * (m + 4) * U * ne[b] / abs(dF_ref.sum()) + 2 * np.spacing(abs(mu[b])))
        x = (e - mu[b]) / kT[b]
        scale = lambda r: np.maximum(np.abs(r), 2.0 ** -52 * np.abs(r).max())
        f_occ = (np.abs(F - SR.occ_of(x)) / scale(SR.occ_of(x))).max() / (HDR["F"] * U)
        f_docc = (np.abs(dF - SR.docc_of(x, kT[b])) / scale(SR.docc_of(x, kT[b]))).max() / (HDR["dF"] * U)
        s = SR.entropy_of(x)
        f_ent = abs(ent[b] - s.sum()) / ((HDR["entropy"] + m + 4) * U * max(s.sum(), np.finfo(float).tiny))
        worst = np.maximum(worst, [f_sum, f_mu, f_occ, f_docc, f_ent])
        assert max(f_sum, f_mu, f_occ, f_docc, f_ent) <= 1.0, (SR.CASES[b], f_sum, f_mu, f_occ, f_docc, f_ent)
        assert np.all(dF <= 0.0) and np.all(F >= 0.0) and np.all(F <= 2.0)
    print("orbital_smearing_parity fermi worst fraction of the bound: sum F %.3f mu %.3f occ %.3f docc %.3f entropy %.3f" % tuple(worst))
    # bitwise: a second call, and the batch in reversed order
    again = fermi_host(orb.fermi(ne, kT))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again, (mu, occ, docc, ent, info)))
    pr = problems("float64")[::-1]
    Hs, Ss = [p[1] for p in pr], [p[2] for p in pr]
    rop, _ = ptrs(Hs)
    rev = BatchedOrbitals(rop, DEV).solve(dev(pack(Hs)), dev(pack(Ss)))
    rmu, rocc, rdocc, rent, _ = fermi_host(rev.fermi(ne[::-1].copy(), kT[::-1].copy()))
    B = len(ne)
    assert np.array_equal(rmu[::-1], mu) and np.array_equal(rent[::-1], ent)
    for b in range(B):
        rb = B - 1 - b
        assert np.array_equal(rocc[rop[rb]:rop[rb + 1]], occ[op[b]:op[b + 1]]) and np.array_equal(rdocc[rop[rb]:rop[rb + 1]], docc[op[b]:op[b + 1]])


def test_fermi_refusals_touch_their_own_molecule_only_and_the_zero_temperature_limit():
    from nabladft_amd import BatchedOrbitals
    ms, nos = [17, 3, 65, 17, 2, 17], [5, 1, 21, 5, 1, 5]
    pairs = [DR.gapped_case(m, n, 0.3, 1e2, 500 + i) for i, (m, n) in enumerate(zip(ms, nos))]
    Hs, Ss = [p[0] for p in pairs], [p[1] for p in pairs]
    Ss[4] = -Ss[4]                                                # an indefinite overlap: the solver fails on molecule 4
    op, _ = ptrs(Hs)
    orb = BatchedOrbitals(op, DEV).solve(dev(pack(Hs)), dev(pack(Ss)))
    good_ne, good_kT = 2.0 * np.array(nos, dtype=np.float64), np.full(6, 0.05)
    ref = fermi_host(orb.fermi(good_ne, good_kT))
    assert ref[4].tolist() == [0, 0, 0, 0, 1, 0]
    ne, kT = good_ne.copy(), good_kT.copy()
    ne[0], ne[1], kT[3], kT[5] = 0.0, 2.0 * ms[1], 0.0, 1e305      # 1e305: finite, but the bracket of mu would not be
    mu, occ, docc, ent, info = fermi_host(orb.fermi(ne, kT))
    assert info.tolist() == [1, 1, 0, 1, 1, 1]
    for b in range(6):
        sl = slice(op[b], op[b + 1])
        if info[b]:
            assert np.isnan(mu[b]) and np.isnan(ent[b]) and np.isnan(occ[sl]).all() and np.isnan(docc[sl]).all()
        else:                                                     # the neighbours: bit for bit what the clean call gave
            assert mu[b] == ref[0][b] and ent[b] == ref[3][b] and np.array_equal(occ[sl], ref[1][sl]) and np.array_equal(docc[sl], ref[2][sl])
    with pytest.raises(RuntimeError, match="Fermi"):
        orb2 = BatchedOrbitals(op[:2], DEV).solve(dev(pack(Hs[:1])), dev(pack(Ss[:1])))
        orb2.fermi(0.0, 0.05)
        orb2.check()
    # kT = 1e-6 with a gap of 0.3: integer occupations, mu inside the gap, no entropy
    mu, occ, docc, ent, info = fermi_host(orb.fermi(good_ne, 1e-6))
    eps = orb.energies.cpu().numpy()
    for b in (0, 1, 2, 3, 5):
        e = eps[op[b]:op[b + 1]]
        assert info[b] == 0 and np.array_equal(occ[op[b]:op[b + 1]], np.where(np.arange(ms[b]) < nos[b], 2.0, 0.0)) and ent[b] == 0.0
        assert np.isfinite(mu[b]) and e[nos[b] - 1] < mu[b] < e[nos[b]]


# ---- 2. every product step alone ------------------------------------------------------------------------------------------------------------------------------------
def raw(name, orb, ins, sizes, fill=None):
    """One entry point of csrc/orbsmear.hip into sentinel-filled buffers with a guard band before and after -> numpy arrays (None where ``sizes`` has None).
    ``fill``: initial contents of the outputs (the diagonal step updates in place)."""
    from nabladft_amd import _lib
    st = orb.state
    bufs = [None if n is None else torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV) for n in sizes]
    outs = [None if b is None else b[GUARD:b.numel() - GUARD] for b in bufs]
    if fill is not None:
        for o, f in zip(outs, fill):
            if o is not None:
                o.copy_(dev(f))
    ins_d = [None if t is None else dev(t) for t in ins]
    rc = getattr(_lib.load(), name)(_lib.ptr(st.buf), *st._dims, *[_lib.ptr(t) for t in ins_d], *[_lib.ptr(o) for o in outs], _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()
    res = []
    for b in bufs:
        if b is None:
            res.append(None)
            continue
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), name
        assert fill is not None or not np.any(h[GUARD:-GUARD] == SENTINEL), name
        res.append(h[GUARD:-GUARD].copy())
    return res


def frac(got, ref, bound):
    if np.size(ref) == 0:                                        # the off-diagonal part of a 1 x 1 block
        return 0.0
    return float((np.abs(got - ref) / np.maximum(bound, np.finfo(float).tiny)).max())


def run_steps(ms, seed, tag, two=True):
    """The five steps on random operands, each against numpy (np.longdouble sums) on the operands the device used -> the worst fraction of the bounds."""
    L = np.longdouble
    rng = np.random.Generator(np.random.PCG64(seed))
    Cs = [rng.normal(size=(m, m)) for m in ms]
    es = [np.sort(rng.uniform(-2.0, 1.0, size=m)) for m in ms]
    for e in es:
        if e.shape[0] > 2:
            e[1] = e[0]                                           # two coincident levels in every molecule that has them
    orb, op = state_with(ms, Cs)
    orb.state.eps.copy_(dev(np.concatenate(es)))
    B, M, P = len(ms), int(sum(ms)), int(sum(m * m for m in ms))
    kT = rng.uniform(0.05, 0.3, size=B)
    mu = np.array([np.median(e) + 0.01 for e in es])
    lay = orb.full_layout()
    G = rng.normal(size=P)
    from nabladft_amd import _lib
    Gs, T = torch.empty(P, dtype=torch.float64, device=DEV), torch.empty(P, dtype=torch.float64, device=DEV)
    assert _lib.load().nq_orb_resp_project(_lib.ptr(orb.state.buf), *orb.state._dims, _lib.ptr(lay[0]), _lib.ptr(lay[1]), lay[2], _lib.ptr(dev(G)), _lib.ptr(Gs),
                                           _lib.ptr(T), _lib.stream_ptr()) == 0
    T = T.cpu().numpy()
    AH, AS, wd = raw("nq_orb_smear_mo", orb, [mu, kT, T], [P, P if two else None, M], fill=[np.full(P, 7.0), np.full(P, 7.0), np.zeros(M)])
    worst = {}
    Gb, Tb, AHb, ASb = blocks(G, ms), blocks(T, ms), blocks(AH, ms), (blocks(AS, ms) if two else [None] * B)
    o = np.concatenate([[0], np.cumsum(ms)])
    xs = [(es[b] - mu[b]) / kT[b] for b in range(B)]
    Fs, dFs = [SR.occ_of(x) for x in xs], [SR.docc_of(x, kT[b]) for b, x in enumerate(xs)]
    for b, m in enumerate(ms):
        Ct, e, x, F = Cs[b], es[b], xs[b], Fs[b]
        off = ~np.eye(m, dtype=bool)
        Gsb = 0.5 * (Gb[b] + Gb[b].T)
        worst["project"] = max(worst.get("project", 0), frac(Tb[b], (Gsb.astype(L) @ Ct.T.astype(L)).astype(float), (m + 4) * U * (np.abs(Gsb) @ np.abs(Ct.T))))
        W, mag = (Ct.astype(L) @ Tb[b].astype(L)).astype(float), np.abs(Ct) @ np.abs(Tb[b])
        K = SR.K_of(x[:, None], x[None, :], kT[b])
        K = np.where(x[:, None] == x[None, :], dFs[b][:, None] + 0 * K, K)
        bH = np.abs(K) * (m + 4) * U * mag + (HDR["K"] + 1) * U * np.abs(K * W)
        worst["mo A_H"] = max(worst.get("mo A_H", 0), frac(AHb[b][off], (K * W)[off], bH[off]))
        assert np.all(np.diag(AHb[b]) == 7.0)                      # the diagonal is the next step's
        worst["mo wdiag"] = max(worst.get("mo wdiag", 0), frac(wd[o[b]:o[b + 1]], np.diag(W), (m + 4) * U * np.diag(mag)))
        if two:
            KS = SR.KS_of(F[:, None], F[None, :], e[:, None], e[None, :], K)
            ksmag = 0.5 * (F[:, None] + F[None, :]) + np.abs(0.5 * (e[:, None] + e[None, :]) * K)
            bS = np.abs(KS) * (m + 4) * U * mag + (HDR["KS"] + HDR["K"] + 1) * U * ksmag * np.abs(W)
            worst["mo A_S"] = max(worst.get("mo A_S", 0), frac(ASb[b][off], (KS * W)[off], bS[off]))
    # the diagonal step, in place
    g_eps, g_occ, g_mu, g_ent = rng.normal(size=M), rng.normal(size=M), rng.normal(size=B), rng.normal(size=B)
    occ, docc = np.concatenate(Fs), np.concatenate(dFs)
    AH2, AS2 = raw("nq_orb_smear_diag", orb, [mu, kT, occ, docc, wd, g_eps, g_occ, g_mu, g_ent], [P, P if two else None], fill=[AH, AS if two else None])
    AH2b, AS2b = blocks(AH2, ms), (blocks(AS2, ms) if two else [None] * B)
    for b, m in enumerate(ms):
        sl = slice(o[b], o[b + 1])
        x, F, dF, w = xs[b].astype(L), Fs[b].astype(L), dFs[b].astype(L), wd[sl].astype(L)
        gF = g_occ[sl] + g_ent[b] * x + w
        ax = np.abs(x)
        p = np.exp(-(ax - ax.min())) / (1 + np.exp(-ax)) ** 2
        p = p / p.sum()
        e = g_eps[sl] + dF * (gF - (p * gF).sum()) + p * g_mu[b]
        gFa = np.abs(g_occ[sl]) + np.abs(g_ent[b] * x) + np.abs(w)
        amag = (np.abs(g_eps[sl]) + np.abs(dF) * (gFa + (p * gFa).sum()) + p * abs(g_mu[b])).astype(float)
        off = ~np.eye(m, dtype=bool)
        assert np.array_equal(AH2b[b][off], AHb[b][off])          # off the diagonal: untouched
        worst["diag A_H"] = max(worst.get("diag A_H", 0), frac(np.diag(AH2b[b]), e.astype(float), (m + 4) * U * amag))
        if two:
            assert np.array_equal(AS2b[b][off], ASb[b][off])
            ref = (-es[b] * e - F * w).astype(float)
            worst["diag A_S"] = max(worst.get("diag A_S", 0), frac(np.diag(AS2b[b]), ref, (m + 4) * U * (np.abs(es[b]) * amag + np.abs(Fs[b] * wd[sl]))))
    RH, RS = raw("nq_orb_smear_back", orb, [AH2, AS2 if two else None], [P, P if two else None])
    RHb, RSb = blocks(RH, ms), (blocks(RS, ms) if two else [None] * B)
    for b, m in enumerate(ms):
        for name, A, Rt in (("back H", AH2b[b], RHb[b]), ("back S", AS2b[b], RSb[b])):
            if A is not None:
                worst[name] = max(worst.get(name, 0), frac(Rt, (A.T.astype(L) @ Cs[b].astype(L)).astype(float), (m + 4) * U * (np.abs(A.T) @ np.abs(Cs[b]))))
    X = orb.syr2k(dev(RH), dev(RS) if two else None, lay)
    for b, m in enumerate(ms):
        for name, Rt, Xd in (("rank-2k H", RHb[b], X[0]), ("rank-2k S", RSb[b], X[1])):
            if Rt is not None:
                got = blocks(Xd.cpu().numpy(), ms)[b]
                Ct = Cs[b].astype(L)
                ref = (0.5 * (Rt.T.astype(L) @ Ct + Ct.T @ Rt.astype(L))).astype(float)
                assert np.array_equal(got, got.T)
                worst[name] = max(worst.get(name, 0), frac(got, ref, (2 * m + 4) * U * 0.5 * (np.abs(Rt.T) @ np.abs(Cs[b]) + np.abs(Cs[b].T) @ np.abs(Rt))))
    print(f"orbital_smearing_parity kernels {tag} worst fraction of the bound: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("two", [True, False])
def test_kernel_bounds_on_ragged_sizes(two):
    worst = run_steps([17, 1, 130, 2, 65, 3, 64, 128, 63], 31, "ragged two outputs" if two else "ragged one output", two)
    assert max(worst.values()) <= 1.0, worst


def test_kernel_bounds_at_the_largest_size():
    worst = run_steps([1024], 32, "m=1024")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("diagonal", [True, False])
def test_exact_on_small_integers(diagonal):
    """Integer coefficients and an even integer G with all levels equal: K = F' and KS are the same power of two for every pair (x = 0, kT = 1/4: K = -2,
    F = 1; eps = -1/2: KS = -(1 + (-1/2)(-2)) = -2), so every product is exact and the chain is C A C^T bit for bit with A = -2 W off the diagonal.
    ``diagonal``: docc = -2 as ``fermi`` would give, on sizes that are powers of two, where the weights p = 1 / m of the diagonal step are exact;
    otherwise docc = 0 (the diagonal of A_H is then exactly zero), on sizes on both sides of the tiles."""
    from nabladft_amd.orbitals import FermiResult
    ms = [4, 64, 1, 128, 2] if diagonal else [5, 65, 1, 130, 63]
    rng = np.random.Generator(np.random.PCG64(33))
    Cs = [rng.integers(-2, 3, size=(m, m)).astype(np.float64) for m in ms]
    orb, op = state_with(ms, Cs)
    M, P, B = sum(ms), sum(m * m for m in ms), len(ms)
    orb.state.eps.copy_(dev(np.full(M, -0.5)))
    dF = -2.0 if diagonal else 0.0
    fr = FermiResult(dev(np.full(B, -0.5)), dev(np.ones(M)), dev(np.full(M, dF)), dev(np.zeros(B)), None, None, dev(np.full(B, 0.25)))
    G = rng.integers(-3, 4, size=P).astype(np.float64) * 2.0
    for overlap in (True, False):
        gH, gS = orb.smeared_response(dev(G), fr, overlap=overlap)
        assert (gS is None) == (not overlap)
        for b, m in enumerate(ms):
            Gb = blocks(G, ms)[b]
            C = Cs[b].T                                            # orbitals as columns
            W = C.T @ (0.5 * (Gb + Gb.T)) @ C
            e = dF * (np.diag(W) - np.diag(W).sum() / m)
            AH, AS = -2.0 * W, -2.0 * W
            AH[np.diag_indices(m)] = e
            AS[np.diag_indices(m)] = 0.5 * e - np.diag(W)
            got = blocks(gH.cpu().numpy(), ms)[b]
            assert np.array_equal(got, C @ AH @ C.T) and np.array_equal(got, got.T), (m, overlap)
            if overlap:
                assert np.array_equal(blocks(gS.cpu().numpy(), ms)[b], C @ AS @ C.T), m


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(inputs):
    """Route (a) and the spread of the two routes for every non-coincident case: [(H, S, ne, kT, G, T, w, ref tuple, bound_H, bound_S)]."""
    out = []
    for case, H, S, ne, kT in problems(inputs):
        G, T, w = SR.upstream(case[0], case[4])
        fH, fS, a = SR.spread(H, S, ne, kT, SR.full_loss(G, T, w))
        out.append((H, S, ne, kT, G, T, w, a, max(BOUND, 4.0 * fH), max(BOUND, 4.0 * fS)))
    return out


@functools.lru_cache(maxsize=None)
def reference_coincident():
    """Route (b), and its spread under another permutation, for the coincident cases."""
    out = []
    for case, H, S, ne, kT in coincident():
        G, T, w = SR.upstream(case[0], case[2])
        loss = SR.full_loss(G, T, w, label_invariant=True)
        b, b2 = SR.closed_form(H, S, ne, kT, loss), SR.closed_form(H, S, ne, kT, loss, seed=3)
        uH, uS = SR.units(H, S, b[0], b[3], kT, b[5], b[6])
        out.append((H, S, ne, kT, G, T, w, b, max(BOUND, 4.0 * np.abs(b[5] - b2[5]).max() / uH), max(BOUND, 4.0 * np.abs(b[6] - b2[6]).max() / uS)))
    return out


def device_loss(sol, refs, op, pp, label_invariant):
    total = 0.0
    for b, r in enumerate(refs):
        m = r[0].shape[0]
        Db = sol.D[int(pp[b]):int(pp[b + 1])].view(m, m)
        eps, occ = sol.eps[int(op[b]):int(op[b + 1])], sol.occ[int(op[b]):int(op[b + 1])]
        total = total + (dev(r[4]) * Db).sum() + 0.5 * ((Db - dev(r[5])) ** 2).sum() + torch.tanh(0.1 * eps).sum() + 0.1 * sol.mu[b] - 0.3 * sol.entropy[b]
        total = total + 0.2 * (occ * eps).sum()
        if not label_invariant:
            total = total + (dev(r[6]) * occ).sum() + (dev(r[6]) * torch.sin(eps / 5.0)).sum()
    return total


def check_gradients(tag, refs, gHd, gSd, out_round):
    ms = [r[0].shape[0] for r in refs]
    gHs = blocks(gHd.double().cpu().numpy(), ms)
    gSs = None if gSd is None else blocks(gSd.double().cpu().numpy(), ms)
    for b, (H, S, ne, kT, G, T, w, a, bH, bS) in enumerate(refs):
        uH, uS = SR.units(H, S, a[0], a[3], kT, a[5], a[6])
        assert np.array_equal(gHs[b], gHs[b].T) and np.isfinite(gHs[b]).all()
        fH = float((np.maximum(np.abs(gHs[b] - a[5]) - out_round * np.abs(a[5]), 0.0) / uH).max())
        fS = 0.0
        if gSs is not None and S is not None:
            assert np.array_equal(gSs[b], gSs[b].T)
            fS = float((np.maximum(np.abs(gSs[b] - a[6]) - out_round * np.abs(a[6]), 0.0) / uS).max())
        print(f"orbital_smearing_parity end-to-end {tag} m={ms[b]} n_elec={ne:g} kT={kT:g} gH {fH:.3g} (bound {bH:.1f}) gS {fS:.3g} (bound {bS:.1f})")
        assert fH <= bH and fS <= bS, (tag, b, fH, fS)


def end_to_end(refs, tdt, with_s, label_invariant, tag):
    from nabladft_amd import smeared_solution
    Hs, Ss = [r[0] for r in refs], [r[1] for r in refs]
    op, pp = ptrs(Hs)
    H = dev(pack(Hs), tdt).requires_grad_(True)
    S = dev(pack(Ss), tdt).requires_grad_(True) if with_s else None
    sol, orb = smeared_solution(H, S, op, [r[2] for r in refs], [r[3] for r in refs], return_solution=True)
    assert all(t.dtype == torch.float64 and t.requires_grad for t in sol)
    device_loss(sol, refs, op, pp, label_invariant).backward()
    orb.check()
    assert H.grad.dtype == tdt and (S is None or S.grad.dtype == tdt)
    check_gradients(tag, refs, H.grad, None if S is None else S.grad, 2.0 ** -24 if tdt == torch.float32 else 0.0)
    return sol, orb, H, S, op, pp


@pytest.mark.parametrize("inputs", ["float64", "float32", "standard"])
def test_smeared_gradients_end_to_end(inputs):
    sol, orb, H, S, op, pp = end_to_end(reference(inputs), torch.float32 if inputs == "float32" else torch.float64, inputs != "standard", False, inputs)
    if inputs != "float64":
        return
    # the forward on the way: D exactly symmetric, Tr(D S) = n_elec within the bound of the population test (m + 4 roundings of the sum of magnitudes)
    refs = reference(inputs)
    Db, Sb = blocks(sol.D.detach().cpu().numpy(), [r[0].shape[0] for r in refs]), [r[1] for r in refs]
    for b, r in enumerate(refs):
        m = r[0].shape[0]
        assert np.array_equal(Db[b], Db[b].T)
        kap = R.spectral(r[0], r[1])[2]
        assert abs((Db[b] * Sb[b]).sum() - r[2]) <= BOUND * m * R.EPS * kap * max(np.abs(Db[b] * Sb[b]).sum(), r[2]), b
    # bitwise reproducible
    from nabladft_amd import smeared_solution
    H2, S2 = H.detach().clone().requires_grad_(True), S.detach().clone().requires_grad_(True)
    sol2 = smeared_solution(H2, S2, op, [r[2] for r in refs], [r[3] for r in refs])
    device_loss(sol2, refs, op, pp, False).backward()
    assert torch.equal(H2.grad, H.grad) and torch.equal(S2.grad, S.grad) and all(torch.equal(a, b) for a, b in zip(sol, sol2))


def test_coincident_levels_against_the_closed_form():
    end_to_end(reference_coincident(), torch.float64, True, True, "coincident")


def test_crossed_gap_contrast_with_the_closed_shell_chain():
    """Where the HOMO and the LUMO coincide ``orbital_solution`` documents inf / NaN in that molecule's gradient block; ``smeared_solution`` is finite there and
    within max(10, 4 x the closed form's own spread) units of the closed form on the same problem."""
    from nabladft_amd import orbital_solution, smeared_solution
    kT = 0.05
    # crossed by construction AND in floating point: a diagonal H under S = 1 whose HOMO and LUMO are the same number, so that the device's two levels
    # are bit for bit equal (a dense H crossed at 0 comes back from the solver a rounding apart, and the closed-shell chain then returns finite garbage)
    lev = np.concatenate([np.linspace(-9.0, -1.0, 4), [0.0, 0.0], np.linspace(0.5, 2.0, 11)])
    Hc, Sc = np.diag(lev), np.eye(17)
    Hg, Sg = DR.gapped_case(17, 5, 0.3, 1e2, 77)
    op, pp = ptrs([Hc, Hg])
    G = dev(np.random.Generator(np.random.PCG64(5)).normal(size=int(pp[-1])))
    H, S = dev(pack([Hc, Hg])).requires_grad_(True), dev(pack([Sc, Sg])).requires_grad_(True)
    eps, D = orbital_solution(H, S, op, [5, 5])
    (G * D).sum().backward()
    gc = H.grad.detach().clone()
    assert not torch.isfinite(gc[:289]).all() and torch.isfinite(gc[289:]).all()
    H.grad = S.grad = None
    sol = smeared_solution(H, S, op, [10.0, 10.0], kT)
    ((G * sol.D).sum() + sol.entropy.sum() + sol.mu.sum()).backward()
    assert torch.isfinite(H.grad).all() and torch.isfinite(S.grad).all()
    e_dev = sol.eps.detach().cpu().numpy()
    assert e_dev[4] == e_dev[5] == 0.0                            # bit for bit equal on the device: the x_i == x_j branch of the divided difference
    # the crossed block against the closed form of the same (label-invariant) loss on the same diagonal problem, and that form's own spread
    Gc = torch.from_numpy(G[:289].cpu().numpy().reshape(17, 17))
    loss = lambda eps_, D_, occ_, mu_, ent_, S_, H_: (Gc * D_).sum() + ent_ + mu_
    b, b2 = SR.closed_form(Hc, Sc, 10.0, kT, loss), SR.closed_form(Hc, Sc, 10.0, kT, loss, seed=3)
    uH, uS = SR.units(Hc, Sc, b[0], b[3], kT, b[5], b[6])
    bH, bS = max(BOUND, 4.0 * np.abs(b[5] - b2[5]).max() / uH), max(BOUND, 4.0 * np.abs(b[6] - b2[6]).max() / uS)
    gH, gS = H.grad[:289].cpu().numpy().reshape(17, 17), S.grad[:289].cpu().numpy().reshape(17, 17)
    fH, fS = float(np.abs(gH - b[5]).max() / uH), float(np.abs(gS - b[6]).max() / uS)
    print("orbital_smearing_parity crossed gap (device levels bitwise equal): closed-shell block finite %s; smeared block gH %.3g (bound %.1f) gS %.3g "
          "(bound %.1f), max |gH| %.3g" % (bool(torch.isfinite(gc[:289]).all()), fH, bH, fS, bS, float(np.abs(gH).max())))
    assert fH <= bH and fS <= bS, (fH, fS)


def test_zero_temperature_limit_is_the_closed_shell_chain():
    from nabladft_amd import orbital_solution, smeared_solution
    cases = [c for c in DR.CASES if c[1] < c[0]]
    pairs = [DR.gapped_case(*c) for c in cases]
    Hs, Ss, nos = [p[0] for p in pairs], [p[1] for p in pairs], [c[1] for c in cases]
    op, pp = ptrs(Hs)
    G = dev(np.random.Generator(np.random.PCG64(6)).normal(size=int(pp[-1])))
    grads = []
    for smeared in (False, True):
        H, S = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss)).requires_grad_(True)
        if smeared:
            sol = smeared_solution(H, S, op, [2.0 * n for n in nos], 0.3 / 200.0)
            eps, D = sol.eps, sol.D
        else:
            eps, D = orbital_solution(H, S, op, nos)
        ((G * D).sum() + torch.tanh(0.1 * eps).sum()).backward()
        grads.append((blocks(H.grad.cpu().numpy(), [h.shape[0] for h in Hs]), blocks(S.grad.cpu().numpy(), [h.shape[0] for h in Hs]), eps.detach().cpu().numpy()))
    for b, c in enumerate(cases):
        e = grads[0][2][op[b]:op[b + 1]]
        uH, uS = DR.units(Hs[b], Ss[b], nos[b], e, grads[0][0][b], grads[0][1][b])
        fH, fS = np.abs(grads[0][0][b] - grads[1][0][b]).max() / uH, np.abs(grads[0][1][b] - grads[1][1][b]).max() / uS
        print(f"orbital_smearing_parity zero-temperature limit m={c[0]} n_occ={c[1]} gH {fH:.3g} gS {fS:.3g} (bound {BOUND})")
        assert fH <= BOUND and fS <= BOUND, (c, fH, fS)


def test_failed_molecule_and_members_without_gradient(monkeypatch):
    from nabladft_amd import _lib, smeared_solution
    pairs = [DR.gapped_case(m, n, 0.3, 1e2, 600 + i) for i, (m, n) in enumerate([(17, 5), (3, 1), (65, 21)])]
    Hs, Ss = [p[0] for p in pairs], [p[1] for p in pairs]
    Ss[1] = -Ss[1]
    op, pp = ptrs(Hs)
    H, S = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss)).requires_grad_(True)
    sol, orb = smeared_solution(H, S, op, [10.0, 2.0, 42.0], 0.05, return_solution=True)
    (sol.D.nansum() + sol.mu.nansum()).backward()
    for t, ptr in ((H.grad, pp), (S.grad, pp), (sol.D, pp), (sol.eps, op), (sol.occ, op)):
        t = t.detach()
        assert torch.isnan(t[int(ptr[1]):int(ptr[2])]).all() and torch.isfinite(t[:int(ptr[1])]).all() and torch.isfinite(t[int(ptr[2]):]).all()
    assert torch.isnan(sol.mu[1]) and torch.isfinite(sol.mu[[0, 2]]).all()
    with pytest.raises(RuntimeError, match="molecule 1"):
        orb.check()
    # what the backward launches: a call counter on the library handle
    lib = _lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("nq_orb_"):
                return fn
            return lambda *a: (calls.append(name), fn(*a))[1]
    good = [pairs[0], pairs[2]]
    op2, pp2 = ptrs([p[0] for p in good])
    H, S = dev(pack([p[0] for p in good])).requires_grad_(True), dev(pack([p[1] for p in good])).requires_grad_(True)
    sol, orb2 = smeared_solution(H, S, op2, [10.0, 42.0], 0.05, return_solution=True)
    # without an upstream gradient for D the chain is sum_k e_k c_k c_k^T from one weighted Gram launch: the same numbers as the products over all pairs on a
    # diagonal A, within the dot-product bound of both sums (m terms there, 2m here)
    fr = orb2.fermi([10.0, 42.0], 0.05)
    ones = torch.ones(2, dtype=torch.float64, device=DEV)
    A = torch.zeros(int(pp2[-1]), dtype=torch.float64, device=DEV)
    orb2.smear_diag(A, None, torch.zeros(int(op2[-1]), dtype=torch.float64, device=DEV), fr, g_mu=ones, g_ent=ones)
    full = orb2.syr2k(*orb2.smear_back(A, None), orb2.full_layout())[0].cpu().numpy()
    short = orb2.smeared_response(None, fr, g_mu=ones, g_ent=ones, overlap=False)[0].cpu().numpy()
    ms2 = [17, 65]
    for b, m in enumerate(ms2):
        Ct, e = blocks(orb2.coefficients.cpu().numpy(), ms2)[b], np.diag(blocks(A.cpu().numpy(), ms2)[b])
        mag = np.abs(Ct).T @ (np.abs(e)[:, None] * np.abs(Ct))
        assert np.all(np.abs(blocks(full, ms2)[b] - blocks(short, ms2)[b]) <= (3 * m + 8) * U * mag) and np.abs(e).max() > 0.0
    monkeypatch.setattr(_lib, "load", lambda: Counting())
    sol.eps.sum().backward(retain_graph=True)
    assert calls == ["nq_orb_wgram"], calls
    del calls[:]
    (sol.mu.sum() + sol.entropy.sum()).backward(retain_graph=True)
    assert calls == ["nq_orb_smear_diag", "nq_orb_wgram"], calls     # no upstream gradient for D: A is diagonal, no product over all pairs
    del calls[:]
    sol.D.sum().backward(retain_graph=True)
    assert calls == ["nq_orb_resp_project", "nq_orb_smear_mo", "nq_orb_smear_diag", "nq_orb_smear_back", "nq_orb_syr2k"], calls
    del calls[:]
    Hn = H.detach().clone().requires_grad_(True)
    smeared_solution(Hn, S.detach(), op2, [10.0, 42.0], 0.05).D.sum().backward()
    assert "nq_orb_smear_mo" in calls and Hn.grad is not None and torch.isfinite(Hn.grad).all()


# ---- 4. the QHNet task ------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_smeared_density_task():
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from test_qhnet_gpu import ORBITALS, load_case
    g, cfg, net, batch = load_case("small", torch.device(DEV))
    per_atom = np.array([sum(2 * l + 1 for l in ORBITALS[int(a)]) for a in g["z"]])
    ends = np.cumsum(g["sizes"])
    sizes_orb = [int(per_atom[e - n:e].sum()) for n, e in zip(g["sizes"], ends)]
    batch.hamiltonian, batch.overlap, o = [], [], 0
    rng = np.random.Generator(np.random.PCG64(6))
    for m in sizes_orb:
        batch.hamiltonian.append(g["target"][o:o + m, o:o + m].astype(np.float32))
        A = rng.normal(size=(m, m)) * 0.1 / np.sqrt(m)
        batch.overlap.append((np.eye(m) + A + A.T).astype(np.float32))
        o += m
    coefs = {"hamiltonian": 1.0, "orbital_energies": 0.25, "density_matrix": 0.5, "mulliken_charges": 2.0}
    losses = {"hamiltonian": HamiltonianLoss(), "orbital_energies": nq.OrbitalEnergyLoss("mae", "occupied"), "density_matrix": nq.DensityMatrixLoss("mse"),
              "mulliken_charges": nq.MullikenChargeLoss("mse")}
    assert nq.electron_counts(batch.z, batch.ptr).tolist() == [92.0, 9.0, 31.0]       # neutral: two of the three molecules hold an odd number of electrons
    make = lambda cls, ls, cs: cls("QHNet", net, None, None, ls, None, None, cs)
    task = make(nq.QHNetSmearedDensityLightning, losses, coefs)
    assert task.kT == 0.01
    task.kT = 0.02
    for p in net.parameters():
        p.grad = None
    loss = task.training_step(batch, 0)
    assert torch.isfinite(loss) and float(loss) > 0.0
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)
    # the target fed as the prediction: every orbital term is exactly zero
    preds, targets, _ = task._evaluate(batch)
    real = nq.QHNetLightning._evaluate

    def fed(self, b):
        p, t, a = real(self, b)
        p["hamiltonian"] = t["hamiltonian"].clone()
        return p, t, a
    import unittest.mock as mock
    with mock.patch.object(nq.QHNetLightning, "_evaluate", fed):
        p2, t2, _ = task._evaluate(batch)
        for k in nq.QHNetSmearedDensityLightning.KEYS:
            assert float(losses[k](p2[k], t2[k], *p2[k + "_args"])) == 0.0, k
    # no orbital key active: QHNetLightning's step, bit for bit
    plain = make(nq.QHNetLightning, {"hamiltonian": HamiltonianLoss()}, {"hamiltonian": 1.0})
    zero = make(nq.QHNetSmearedDensityLightning, losses, {"hamiltonian": 1.0, "orbital_energies": 0.0, "density_matrix": 0.0, "mulliken_charges": 0.0})
    a, b = plain.training_step(batch, 0), zero.training_step(batch, 0)
    assert a.dtype == b.dtype and torch.equal(a.detach(), b.detach())
