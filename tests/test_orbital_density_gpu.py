"""GPU: the density-response kernels and the reverse of the population kernel (csrc/orbresp.hip) through the C ABI, and the differentiable density, populations,
losses and the QHNet task of nabladft_amd.orbital_loss end to end against the float64 yardstick (tests/orbital_density_ref.py, whose own spread
tests/test_orbital_density_cpu.py pins).

Bounds.  Kernels, on coefficients and energies written into the state (no solve), each step against numpy on the same operands:
|x - ref| <= (K + 4) 2^-53 sum |terms| with K the number of terms of the sum (gamma_{K+2} with two spare roundings; any summation order).  Step 1: K = m, the
terms hold Gs = fl((G + G^T) / 2), which numpy forms with the same single rounding.  Step 2: K = m for W; A_H = 4 W / d with d = fl(eps_i - eps_a), the same
in numpy, adds the division's rounding: (K + 5) 2^-53 |4 / d| sum |terms|; A_S = -eps_i A_H is one more product, held to (K + 5) 2^-53 |4 eps_i / d| sum |terms| (one
of the two spare roundings pays for it); the occupied rows -2 W are an exact scaling.  Step 3: K = m - n_occ for Rt_H (the zero rows of A_H add nothing),
K = m for Rt_S.  Step 4: K = 2 n_occ, the halving is exact.
End to end, with the device solver: max(10, 4 x the spread of the two reference routes for that case, computed here on the host) in the units of
orbital_density_ref.units; ten is the bound the project holds the solver to (test_orbitals_gpu.BOUND).  Float32 results are allowed their own rounding,
2^-24 per element.  Every figure is printed as an ``orbital_density_parity ...`` line (kept in profiles/orbital_density_parity.txt)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbitals_ref as R
from test_orbital_loss_gpu import blocks, db_plan, i32, state_with
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, ptrs, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 130]
SENTINEL = -7.25e300
GUARD = 64
U = 2.0 ** -53


# ---- raw launches into guarded buffers --------------------------------------------------------------------------------------------------------------------
def layout(ms, nos):
    occ = np.concatenate([[0], np.cumsum(np.asarray(nos, dtype=np.int64) * np.asarray(ms, dtype=np.int64))]).astype(np.int64)
    return i32(nos), dev(occ), int(occ[-1]), occ


def raw(name, orb, lay, ins, sizes):
    """One entry point of csrc/orbresp.hip into sentinel-filled buffers with a guard band before and after -> numpy arrays (None where ``sizes`` has None:
    that output is passed as NULL).  Asserts that the guards still hold the sentinel and that none survives inside."""
    from nabladft_amd import _lib
    st = orb.state
    bufs = [None if n is None else torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV) for n in sizes]
    outs = [None if b is None else b[GUARD:b.numel() - GUARD] for b in bufs]
    ins_d = [None if t is None else dev(t) for t in ins]          # kept alive until the results are read back
    rc = getattr(_lib.load(), name)(_lib.ptr(st.buf), *st._dims, _lib.ptr(lay[0]), _lib.ptr(lay[1]), lay[2], *[_lib.ptr(t) for t in ins_d],
                                    *[_lib.ptr(o) for o in outs], _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()
    res = []
    for b in bufs:
        if b is None:
            res.append(None)
            continue
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), name
        assert not np.any(h[GUARD:-GUARD] == SENTINEL), name
        res.append(h[GUARD:-GUARD].copy())
    return res


def project(orb, lay, G):
    return raw("nq_orb_resp_project", orb, lay, [G], [orb.state.P, lay[2]])[1]


def oblocks(flat, occ, ms, nos, rows_are_orbitals):
    """Occupied-packed array -> per-molecule [m, n_occ] (T, A) or [n_occ, m] (Rt)."""
    return [flat[occ[b]:occ[b] + m * n].reshape((m, n) if rows_are_orbitals else (n, m)) for b, (m, n) in enumerate(zip(ms, nos))]


def occupations(kind, ms):
    if kind == "one":
        return [1] * len(ms)
    if kind == "full":
        return list(ms)
    if kind == "all_but_one":
        return [max(1, m - 1) for m in ms]
    out = []                                                     # "ragged": n_occ % 4 != 0 and (m - n_occ) % 4 != 0 where m allows it
    for m in ms:
        ok = [n for n in range(1, m + 1) if n % 4 and (m - n) % 4]
        out.append(ok[len(ok) // 3] if ok else 1)
    return out


KINDS = ["one", "full", "all_but_one", "ragged"]


@functools.lru_cache(maxsize=None)
def random_batch():
    """The sizes in shuffled order plus two molecules of 65 orbitals that get n_occ = 16 and 17 -> (ms, Ct blocks, eps blocks)."""
    rng = np.random.Generator(np.random.PCG64(21))
    ms = [SIZES[i] for i in rng.permutation(len(SIZES))] + [65, 65]
    Cs = [rng.normal(size=(m, m)) for m in ms]
    es = [np.sort(rng.uniform(-20.0, 2.0, size=m)) for m in ms]
    return ms, Cs, es


def prepared(ms, Cs, es):
    orb, op = state_with(ms, Cs)
    orb.state.eps.copy_(dev(np.concatenate(es)))
    return orb, op


def batch_occ(kind):
    ms = random_batch()[0]
    return occupations(kind, ms[:-2]) + [16, 17]


# ---- numpy restatements of the four steps, each with the sum of absolute terms its bound is made of ---------------------------------------------------
def ref_project(Ct, n, G, ft=np.longdouble):
    Gs = 0.5 * (G + G.T)
    return (Gs.astype(ft) @ Ct[:n].T.astype(ft)).astype(np.float64), np.abs(Gs) @ np.abs(Ct[:n].T)


def ref_mo(Ct, eps, n, T, ft=np.longdouble):
    m = Ct.shape[0]
    W, mag = (Ct.astype(ft) @ T.astype(ft)).astype(np.float64), np.abs(Ct) @ np.abs(T)
    AH, AS, bH, bS = np.zeros((m, n)), np.zeros((m, n)), np.zeros((m, n)), np.zeros((m, n))
    AS[:n], bS[:n] = -2.0 * W[:n], (m + 4) * U * 2.0 * mag[:n]
    if n < m:
        d = eps[None, :n] - eps[n:, None]
        AH[n:] = 4.0 * W[n:] / d
        AS[n:] = -eps[None, :n] * AH[n:]
        bH[n:] = (m + 5) * U * np.abs(4.0 / d) * mag[n:]
        bS[n:] = np.abs(eps[None, :n]) * bH[n:]
    return AH, AS, bH, bS


def ref_back(Ct, n, AH, AS, ft=np.longdouble):
    m = Ct.shape[0]
    RH, RS = (AH.T.astype(ft) @ Ct.astype(ft)).astype(np.float64), (AS.T.astype(ft) @ Ct.astype(ft)).astype(np.float64)
    return RH, RS, (m - n + 4) * U * (np.abs(AH.T) @ np.abs(Ct)), (m + 4) * U * (np.abs(AS.T) @ np.abs(Ct))


def ref_syr2k(Ct, n, Rt, ft=np.longdouble):
    Co = Ct[:n].astype(ft)
    X = (0.5 * (Rt.T.astype(ft) @ Co + Co.T @ Rt.astype(ft))).astype(np.float64)
    return X, (2 * n + 4) * U * 0.5 * (np.abs(Rt.T) @ np.abs(Ct[:n]) + np.abs(Ct[:n].T) @ np.abs(Rt))


def worst_ratio(got, ref, bound):
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    assert np.all(err[bound == 0.0] == 0.0)
    return float((err[bound > 0.0] / bound[bound > 0.0]).max()) if np.any(bound > 0.0) else 0.0


def run_steps(ms, Cs, es, nos, seed, ft=np.longdouble, tag=""):
    """Every step on random operands of its own, both with and without the second weight set, against numpy."""
    rng = np.random.Generator(np.random.PCG64(seed))
    orb, op = prepared(ms, Cs, es)
    lay = layout(ms, nos)
    occ, O, P = lay[3], lay[2], orb.state.P
    G = np.concatenate([rng.normal(size=m * m) for m in ms])
    Tn, AHn, ASn, R0n, R1n = (rng.normal(size=O) for _ in range(5))
    for b, (m, n) in enumerate(zip(ms, nos)):                    # A_H as the chain hands it over: zero over the occupied rows
        AHn[occ[b]:occ[b] + n * n] = 0.0
    T = project(orb, lay, G)
    AH, AS = raw("nq_orb_resp_mo", orb, lay, [Tn], [O, O])
    AH1, none = raw("nq_orb_resp_mo", orb, lay, [Tn], [O, None])
    RH, RS = raw("nq_orb_resp_back", orb, lay, [AHn, ASn], [O, O])
    RH1, _ = raw("nq_orb_resp_back", orb, lay, [AHn, None], [O, None])
    X0, X1 = raw("nq_orb_syr2k", orb, lay, [R0n, R1n], [P, P])
    X01, _ = raw("nq_orb_syr2k", orb, lay, [R0n, None], [P, None])
    assert none is None and same_bits(AH1, AH) and same_bits(RH1, RH) and same_bits(X01, X0)   # one weight set: the same bits
    worst = np.zeros(7)
    for b, (m, n) in enumerate(zip(ms, nos)):
        Ct, eps = Cs[b], es[b]
        Gb = G[orb.pack_ptr[b]:orb.pack_ptr[b + 1]].reshape(m, m)
        ob = lambda flat, rows: oblocks(flat, occ, ms, nos, rows)[b]
        t_ref, t_mag = ref_project(Ct, n, Gb, ft)
        ah, as_, bH, bS = ref_mo(Ct, eps, n, ob(Tn, True), ft)
        rh, rs, bRH, bRS = ref_back(Ct, n, ob(AHn, True), ob(ASn, True), ft)
        x0, b0 = ref_syr2k(Ct, n, ob(R0n, False), ft)
        x1, b1 = ref_syr2k(Ct, n, ob(R1n, False), ft)
        Xb0, Xb1 = blocks(X0, ms)[b], blocks(X1, ms)[b]
        assert np.array_equal(Xb0, Xb0.T) and np.array_equal(Xb1, Xb1.T), (tag, b, m, n)     # exactly symmetric
        assert np.all(ob(AH, True)[:n] == 0.0)
        fig = np.array([worst_ratio(ob(T, True), t_ref, (m + 4) * U * t_mag), worst_ratio(ob(AH, True), ah, bH), worst_ratio(ob(AS, True), as_, bS),
                        worst_ratio(ob(RH, False), rh, bRH), worst_ratio(ob(RS, False), rs, bRS), worst_ratio(Xb0, x0, b0), worst_ratio(Xb1, x1, b1)])
        worst = np.maximum(worst, fig)
        assert np.all(fig <= 1.0), (tag, b, m, n, fig)
    print("orbital_density_parity kernels %s worst error / bound: project %.3f mo A_H %.3f A_S %.3f back Rt_H %.3f Rt_S %.3f syr2k %.3f %.3f" % ((tag,) + tuple(worst)))


# ---- 1. exact placement -------------------------------------------------------------------------------------------------------------------------------------
def test_exact_placement_with_small_integers():
    """Small non-zero integers in every operand: all products and sums are exact in float64 (the halves of Gs and of the last step too), the one division is
    correctly rounded on both sides: lane maps, tile offsets, the transposed LDS tiles and the mirror are compared with numpy bit for bit."""
    ms = [5, 1, 65, 17, 130, 64]
    nos = [2, 1, 17, 17, 43, 63]
    rng = np.random.Generator(np.random.PCG64(1))
    nz = lambda size, top: rng.integers(1, top + 1, size=size).astype(np.float64) * rng.choice([-1.0, 1.0], size=size)
    Cs = [nz((m, m), 3) for m in ms]
    es = [np.concatenate([nz(n, 5), 6.0 + np.arange(m - n)]) for m, n in zip(ms, nos)]        # integer energies, occupied and virtual never equal
    orb, op = prepared(ms, Cs, es)
    lay = layout(ms, nos)
    occ, O, P = lay[3], lay[2], orb.state.P
    G = nz(P, 4)
    T = project(orb, lay, G)
    AH, AS = raw("nq_orb_resp_mo", orb, lay, [T], [O, O])
    AHi, ASi, R0, R1 = nz(O, 3), nz(O, 3), nz(O, 3), nz(O, 3)
    for b, (m, n) in enumerate(zip(ms, nos)):                    # A_H as the chain hands it over: zero over the occupied rows
        AHi[occ[b]:occ[b] + n * n] = 0.0
    RH, RS = raw("nq_orb_resp_back", orb, lay, [AHi, ASi], [O, O])
    RH1, _ = raw("nq_orb_resp_back", orb, lay, [AHi, None], [O, None])
    X0, X1 = raw("nq_orb_syr2k", orb, lay, [R0, R1], [P, P])
    for b, (m, n) in enumerate(zip(ms, nos)):
        Ct, eps = Cs[b], es[b]
        ob = lambda flat, rows: oblocks(flat, occ, ms, nos, rows)[b]
        Gb = G[orb.pack_ptr[b]:orb.pack_ptr[b + 1]].reshape(m, m)
        Tb = (0.5 * (Gb + Gb.T)) @ Ct[:n].T
        assert same_bits(ob(T, True), Tb + 0.0), (b, m, n)
        W = Ct @ Tb
        ah, as_ = np.zeros((m, n)), -2.0 * W
        ah[n:] = 4.0 * W[n:] / (eps[None, :n] - eps[n:, None])
        as_[n:] = -eps[None, :n] * ah[n:]
        assert same_bits(ob(AH, True), ah) and same_bits(ob(AS, True), as_), (b, m, n)
        assert same_bits(ob(RH, False), ob(AHi, True).T @ Ct + 0.0) and same_bits(ob(RS, False), ob(ASi, True).T @ Ct + 0.0), (b, m, n)
        assert same_bits(ob(RH1, False), ob(RH, False)), (b, m, n)                           # alone, Rt_H skips the zero rows: the same bits
        for X, Rt in ((X0, R0), (X1, R1)):
            ref = 0.5 * (ob(Rt, False).T @ Ct[:n] + Ct[:n].T @ ob(Rt, False)) + 0.0
            assert same_bits(blocks(X, ms)[b], ref), (b, m, n)


# ---- 2. the kernels' bounds -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_bounds_on_ragged_sizes_and_occupations(kind):
    ms, Cs, es = random_batch()
    nos = batch_occ(kind)
    assert all(1 <= n <= m for n, m in zip(nos, ms))
    if kind == "ragged":
        assert all(n % 4 and (m - n) % 4 for n, m in zip(nos[:-2], ms[:-2]) if m >= 15)
    run_steps(ms, Cs, es, nos, 30 + KINDS.index(kind), tag=kind)


def test_kernel_bounds_at_the_largest_size():
    """m = 1024 with n_occ = 300, once, kernels only.  The reference is plain float64 numpy (an extended-precision product of this size takes too long for a
    test), so its own rounding shares the bound with the kernel's."""
    rng = np.random.Generator(np.random.PCG64(3))
    run_steps([1024], [rng.normal(size=(1024, 1024))], [np.sort(rng.uniform(-20.0, 2.0, size=1024))], [300], 4, ft=np.float64, tag="m=1024 n_occ=300")


# ---- 3. bitwise -------------------------------------------------------------------------------------------------------------------------------------------------
def chain(orb, lay, G, overlap=True):
    """The four launches as ``density_response`` chains them -> every intermediate, numpy."""
    O, P = lay[2], orb.state.P
    T = project(orb, lay, G)
    AH, AS = raw("nq_orb_resp_mo", orb, lay, [T], [O, O if overlap else None])
    RH, RS = raw("nq_orb_resp_back", orb, lay, [AH, AS], [O, O if overlap else None])
    XH, XS = raw("nq_orb_syr2k", orb, lay, [RH, RS], [P, P if overlap else None])
    return T, AH, AS, RH, RS, XH, XS


def test_bitwise_reproducible_and_batch_independent():
    ms, Cs, es = random_batch()
    nos = batch_occ("ragged")
    rng = np.random.Generator(np.random.PCG64(5))
    Gs = [rng.normal(size=m * m) for m in ms]
    orb, op = prepared(ms, Cs, es)
    lay = layout(ms, nos)
    a, b2 = chain(orb, lay, np.concatenate(Gs)), chain(orb, lay, np.concatenate(Gs))
    assert all(same_bits(x, y) for x, y in zip(a, b2))
    h = chain(orb, lay, np.concatenate(Gs), overlap=False)       # without the overlap half: the same dL/dH bit for bit
    assert h[2] is None and h[4] is None and h[6] is None and same_bits(h[5], a[5])
    # the Python chain is the same four launches
    gH, gS = orb.density_response(dev(np.concatenate(Gs)), nos)
    assert same_bits(gH.cpu().numpy(), a[5]) and same_bits(gS.cpu().numpy(), a[6])
    occ = lay[3]
    for b, (m, n) in enumerate(zip(ms, nos)):
        alone, _ = prepared([m], [Cs[b]], [es[b]])
        c = chain(alone, layout([m], [n]), Gs[b])
        for x, y in zip(c[:5], a[:5]):
            assert same_bits(x, y[occ[b]:occ[b + 1]]), (b, m, n)
        for x, y in zip(c[5:], a[5:]):
            assert same_bits(x.reshape(m, m), blocks(y, ms)[b]), (b, m, n)


# ---- 4. a failed molecule, no occupied orbital, no virtual orbital -----------------------------------------------------------------------------------------------
def test_failed_molecule_gets_nan_and_the_empty_ranges_give_zeros():
    rng = np.random.Generator(np.random.PCG64(6))
    ms = [24, 65, 5, 63, 17]
    nos = [7, 30, 0, 21, 17]                                     # molecule 2: no occupied orbital; molecule 4: no virtual orbital
    Cs = [rng.normal(size=(m, m)) for m in ms]
    es = [np.sort(rng.uniform(-20.0, 2.0, size=m)) for m in ms]
    G = np.concatenate([rng.normal(size=m * m) for m in ms])
    orb, op = prepared(ms, Cs, es)
    lay = layout(ms, nos)
    occ = lay[3]
    clean = chain(orb, lay, G)
    Xh, Xs = blocks(clean[5], ms), blocks(clean[6], ms)
    assert same_bits(Xh[2], np.zeros((5, 5))) and same_bits(Xs[2], np.zeros((5, 5)))            # n_occ = 0: zeros
    assert np.all(Xh[4] == 0.0) and np.abs(Xs[4]).max() > 0.0                                # n_occ = m: dL/dH is exactly zero, dL/dS is not
    orb.state.status[1] = 1                                      # as the solver marks a molecule whose overlap is not positive definite
    bad = chain(orb, lay, G)
    for x, c in zip(bad[:5], clean[:5]):
        assert np.isnan(x[occ[1]:occ[2]]).all() and same_bits(x[:occ[1]], c[:occ[1]]) and same_bits(x[occ[2]:], c[occ[2]:])
    for x, c in zip(bad[5:], clean[5:]):
        got, ref = blocks(x, ms), blocks(c, ms)
        assert np.isnan(got[1]).all() and all(same_bits(got[b], ref[b]) for b in (0, 2, 3, 4))


# ---- 5. the reverse of the population kernel ------------------------------------------------------------------------------------------------------------------------
def test_population_backward_against_the_formula():
    """Two molecules whose first and last atoms own orbital ranges of different lengths (the last atom of the batch ends at M), a NON-symmetric D, poisoned
    upper triangles of S and H; with S, with S = None, float32 S and H, and with missing upstream gradients."""
    ms, per_atom = [7, 4], [[3, 1, 3], [1, 3]]
    rng = np.random.Generator(np.random.PCG64(9))
    orb, op = state_with(ms, [rng.normal(size=(m, m)) for m in ms])
    sym = lambda a: np.tril(a) + np.tril(a, -1).T
    Ds, Ss, Hs = [rng.normal(size=(m, m)) for m in ms], [sym(rng.normal(size=(m, m))) for m in ms], [sym(rng.normal(size=(m, m))) for m in ms]
    flat = [n for mol in per_atom for n in mol]
    plan = SimpleNamespace(B=2, N=5, m_total=11, total=65, mol_ptr=i32([0, 3, 5]), orb_ptr=dev(np.concatenate([[0], np.cumsum(flat)]).astype(np.int64)))
    g_pop, g_ne, g_eb = rng.normal(size=5), rng.normal(size=2), rng.normal(size=2)
    D = dev(pack(Ds))
    for with_s, dt in ((True, np.float64), (False, np.float64), (True, np.float32)):
        S_ = [s.astype(dt).astype(np.float64) for s in Ss]
        H_ = [h.astype(dt).astype(np.float64) for h in Hs]
        Sd = dev(pack(S_, dt, poison=1e30)) if with_s else None
        Hd = dev(pack(H_, dt, poison=1e30))
        for gp, gn, ge in ((g_pop, g_ne, g_eb), (None, g_ne, None), (g_pop, None, None)):
            d = lambda x: None if x is None else dev(x)
            gD, gS, gH = orb.populations_backward(plan, d(gp), d(gn), d(ge), D, Sd, Hd, want_s=with_s, want_h=True)
            assert (gS is None) == (not with_s)
            a0 = 0
            for b, m in enumerate(ms):
                ga = np.zeros(m) if gp is None else np.repeat(gp[a0:a0 + len(per_atom[b])], per_atom[b])
                a0 += len(per_atom[b])
                ne, eb = (0.0 if gn is None else gn[b]), (0.0 if ge is None else ge[b])
                Sm = S_[b] if with_s else np.eye(m)
                rD = (0.5 * (ga[:, None] + ga[None, :]) + ne) * Sm + eb * H_[b]
                rS = 0.5 * ((ga[:, None] + ne) * Ds[b] + (ga[None, :] + ne) * Ds[b].T)
                rH = eb * (0.5 * (Ds[b] + Ds[b].T))
                tol = 4.0 * R.EPS
                assert np.all(np.abs(blocks(gD.cpu().numpy(), ms)[b] - rD) <= tol * (np.abs(0.5 * (ga[:, None] + ga[None, :])) + abs(ne) + abs(eb)) * (np.abs(Sm) + np.abs(H_[b])))
                assert np.all(np.abs(blocks(gH.cpu().numpy(), ms)[b] - rH) <= tol * np.abs(eb) * (np.abs(Ds[b]) + np.abs(Ds[b].T)))
                if with_s:
                    assert np.all(np.abs(blocks(gS.cpu().numpy(), ms)[b] - rS) <= tol * (np.abs(ga).max() + abs(ne)) * (np.abs(Ds[b]) + np.abs(Ds[b].T)))
    # through autograd: the dense formulas on symmetrised leaves
    from nabladft_amd.orbital_loss import populations
    Ds = [0.5 * (d + d.T) for d in Ds]                           # a density is symmetric; the dense formulas below are written on symmetrised leaves
    Dt, St, Ht = dev(pack(Ds)).requires_grad_(True), dev(pack(Ss)).requires_grad_(True), dev(pack(Hs)).requires_grad_(True)
    pop, nelec, eband = populations(Dt, plan, St, Ht, orb)
    (pop * dev(g_pop)).sum().add((nelec * dev(g_ne)).sum()).add((eband * dev(g_eb)).sum()).backward()
    a0 = 0
    for b, m in enumerate(ms):
        leaves = [torch.tensor(x, requires_grad=True) for x in (Ds[b], Ss[b], Hs[b])]
        Dm, Sm, Hm = [0.5 * (x + x.T) for x in leaves]
        rows = (Dm * Sm).sum(1)
        ends = np.concatenate([[0], np.cumsum(per_atom[b])])
        atom_pop = torch.stack([rows[i:j].sum() for i, j in zip(ends[:-1], ends[1:])])
        loss = (atom_pop * torch.from_numpy(g_pop[a0:a0 + len(per_atom[b])])).sum() + g_ne[b] * rows.sum() + g_eb[b] * (Dm * Hm).sum()
        a0 += len(per_atom[b])
        loss.backward()
        for got, leaf in zip((Dt.grad, St.grad, Ht.grad), leaves):
            g, r = blocks(got.cpu().numpy(), ms)[b], leaf.grad.numpy()
            assert np.abs(g - r).max() <= 16 * R.EPS * max(1.0, np.abs(r).max()), (b, np.abs(g - r).max())


# ---- 6. end to end with the device solver -----------------------------------------------------------------------------------------------------------------------
def case_loss(case):
    m, n_occ, seed = case[0], case[1], case[4]
    G, T = DR.upstream(m, seed)
    return G, T, n_occ < m                                       # every orbital occupied: no energy term, dL/dH is compared with exact zero


@functools.lru_cache(maxsize=None)
def reference(inputs):
    """Route (a) and the spread of the two routes for every case, once per kind of input: [(case, H, S, G, T, with_eps, eps, D, gH, gS, bound_H, bound_S)] on
    the inputs as the device sees them (float32: rounded; standard: S = None)."""
    out = []
    for case in DR.CASES:
        H, S = DR.gapped_case(*case, standard=inputs == "standard")
        if inputs == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        G, T, with_eps = case_loss(case)
        fH, fS, eps, D, gH, gS = DR.spread(H, S, case[1], DR.quadratic_loss(G, T, with_eps))
        out.append((case, H, S, G, T, with_eps, eps, D, gH, gS, max(BOUND, 4.0 * (fH if with_eps else 0.0)), max(BOUND, 4.0 * fS)))
    return out


def device_loss(eps, D, refs, op, pp):
    total = 0.0
    for b, r in enumerate(refs):
        m = r[1].shape[0]
        Db = D[int(pp[b]):int(pp[b + 1])].view(m, m)
        total = total + (dev(r[3]) * Db).sum() + 0.5 * ((Db - dev(r[4])) ** 2).sum()
        if r[5]:
            total = total + torch.tanh(0.1 * eps[int(op[b]):int(op[b + 1])]).sum()
    return total


def check_gradients(tag, refs, gHd, gSd, out_round):
    ms = [r[1].shape[0] for r in refs]
    gHs = blocks(gHd.double().cpu().numpy(), ms)
    gSs = None if gSd is None else blocks(gSd.double().cpu().numpy(), ms)
    for b, (case, H, S, G, T, with_eps, eps, D, gH, gS, bH, bS) in enumerate(refs):
        m, n = case[0], case[1]
        uH, uS = DR.units(H, S, n, eps, gH, gS)
        assert np.array_equal(gHs[b], gHs[b].T)
        if n == m:
            assert np.all(gHs[b] == 0.0), (tag, case)            # no virtual orbital and no energy term: exactly zero
            fH = 0.0
        else:
            fH = float((np.maximum(np.abs(gHs[b] - gH) - out_round * np.abs(gH), 0.0) / uH).max())
        fS = 0.0
        if gSs is not None:
            fS = float((np.maximum(np.abs(gSs[b] - gS) - out_round * np.abs(gS), 0.0) / uS).max())
            assert np.array_equal(gSs[b], gSs[b].T)
        print(f"orbital_density_parity end-to-end {tag} m={m} n_occ={n} kappa0={case[3]:g} gH {fH:.3g} (bound {bH:.1f}) gS {fS:.3g} (bound {bS:.1f})")
        assert fH <= bH and fS <= bS, (tag, case, fH, fS)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_density_gradients_end_to_end(dtype):
    from nabladft_amd.orbital_loss import orbital_solution
    refs = reference(dtype)
    Hs, Ss, nos = [r[1] for r in refs], [r[2] for r in refs], [r[0][1] for r in refs]
    op, pp = ptrs(Hs)
    tdt = getattr(torch, dtype)
    H, S = dev(pack(Hs), tdt).requires_grad_(True), dev(pack(Ss), tdt).requires_grad_(True)
    eps, D, sol = orbital_solution(H, S, op, nos, return_solution=True)
    assert eps.dtype == torch.float64 and D.dtype == torch.float64 and eps.requires_grad and D.requires_grad and not sol.coefficients.requires_grad
    device_loss(eps, D, refs, op, pp).backward()
    sol.check()
    assert H.grad.dtype == tdt and S.grad.dtype == tdt and H.grad.shape == H.shape and S.grad.shape == S.shape
    Db = blocks(D.detach().cpu().numpy(), [h.shape[0] for h in Hs])
    for b, r in enumerate(refs):                                  # the forward: the density itself, in the units of the existing density test
        m, n = r[0][0], r[0][1]
        assert np.abs(Db[b] - r[7]).max() <= BOUND * m * R.EPS * R.spectral(r[1], r[2])[2] * (r[6][-1] - r[6][0] + 1.0) / 0.3 * max(1.0, np.abs(r[7]).max())
    check_gradients(dtype, refs, H.grad, S.grad, 2.0 ** -24 if dtype == "float32" else 0.0)


def test_density_gradients_without_an_overlap_gradient_and_without_an_overlap():
    from nabladft_amd.orbital_loss import density_matrix, orbital_energies, orbital_solution
    refs = reference("float64")
    Hs, Ss, nos = [r[1] for r in refs], [r[2] for r in refs], [r[0][1] for r in refs]
    op, pp = ptrs(Hs)
    # S without requires_grad: no gS, the same gH bit for bit
    H, S = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss))
    device_loss(*orbital_solution(H, S, op, nos), refs, op, pp).backward()
    H2, S2 = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss)).requires_grad_(True)
    device_loss(*orbital_solution(H2, S2, op, nos), refs, op, pp).backward()
    assert S.grad is None and S2.grad is not None and torch.equal(H.grad, H2.grad)
    # the density alone: its gradient plus the energies' (orbital_energies) is the gradient of both, the same addition
    H3 = dev(pack(Hs)).requires_grad_(True)
    D3 = density_matrix(H3, S, op, nos)
    zero_eps = torch.zeros(int(op[-1]), dtype=torch.float64, device=DEV)
    (device_loss(zero_eps, D3, refs, op, pp)).backward()
    H5 = dev(pack(Hs)).requires_grad_(True)
    device_loss(orbital_energies(H5, S, op), torch.zeros_like(D3), refs, op, pp).backward()
    assert torch.equal(H5.grad + H3.grad, H.grad)
    # S = None: the standard problem against its own two reference routes
    std = reference("standard")
    Hstd = [r[1] for r in std]
    H4 = dev(pack(Hstd)).requires_grad_(True)
    device_loss(*orbital_solution(H4, None, op, nos), std, op, pp).backward()
    check_gradients("standard", std, H4.grad, None, 0.0)


def test_degenerate_occupied_levels_are_harmless():
    """Two equal occupied levels: the device gradients against route (b) -- route (a) is off by orders of magnitude here (tests/test_orbital_density_cpu.py) --
    held to max(10, 4 x the spread of route (b) under two permutations), finite everywhere."""
    from nabladft_amd.orbital_loss import density_matrix
    m, n = 65, 21
    H, S = DR.gapped_case(m, n, 0.3, 1e2, 5, degenerate=True)
    G, T = DR.upstream(m, 5)
    loss = DR.quadratic_loss(G, T, with_eps=False)
    eps, _, gH, gS = DR.closed_form(H, S, n, loss)
    _, _, gH2, gS2 = DR.closed_form(H, S, n, loss, seed=3)
    uH, uS = DR.units(H, S, n, eps, gH, gS)
    bH, bS = max(BOUND, 4.0 * np.abs(gH - gH2).max() / uH), max(BOUND, 4.0 * np.abs(gS - gS2).max() / uS)
    Hd, Sd = dev(H.reshape(-1)).requires_grad_(True), dev(S.reshape(-1)).requires_grad_(True)
    D, sol = density_matrix(Hd, Sd, [0, m], [n], return_solution=True)
    Db = D.view(m, m)
    ((dev(G) * Db).sum() + 0.5 * ((Db - dev(T)) ** 2).sum()).backward()
    sol.check()
    e = sol.energies.cpu().numpy()
    gHd, gSd = Hd.grad.cpu().numpy().reshape(m, m), Sd.grad.cpu().numpy().reshape(m, m)
    assert np.isfinite(gHd).all() and np.isfinite(gSd).all()
    fH, fS = float(np.abs(gHd - gH).max() / uH), float(np.abs(gSd - gS).max() / uS)
    print(f"orbital_density_parity end-to-end degenerate m={m} n_occ={n} eps_1 - eps_0 {e[1] - e[0]:.3e} gH {fH:.3g} (bound {bH:.1f}) gS {fS:.3g} (bound {bS:.1f})")
    assert fH <= bH and fS <= bS


# ---- 7. populations and the losses on the database molecules --------------------------------------------------------------------------------------------------------
def test_population_and_loss_gradients_on_the_database_molecules():
    """H, S -> density -> populations -> charges, ``MullikenChargeLoss`` + ``DensityMatrixLoss`` + weighted electron counts and band energies, on the five
    database molecules with a positive definite overlap: the loss against the dense formulas, its gradients against route (a) of the same loss."""
    import nabladft_amd as nq
    probs = db_problems()[:5]
    Hs, Ss = [p[0] for p in probs], [p[1] for p in probs]
    ms = [h.shape[0] for h in Hs]
    B = len(ms)
    op, pp = ptrs(Hs)
    plan, per_atom = db_plan(probs)
    z = np.concatenate([np.asarray(p[2], dtype=np.int64) for p in probs])
    aptr = np.concatenate([[0], np.cumsum([len(p[2]) for p in probs])])
    n_occ = nq.occupied_counts(z, aptr, 0, op)
    rng = np.random.Generator(np.random.PCG64(12))
    q_t = rng.normal(size=len(z)) * 0.3
    D_t = [np.asarray(2.0 * np.eye(m) + 0.1 * (lambda N: N + N.T)(rng.normal(size=(m, m)))) for m in ms]
    w_ne, w_eb = rng.normal(size=B), rng.normal(size=B) * 0.01
    l_q, l_d = nq.MullikenChargeLoss("mse"), nq.DensityMatrixLoss("mae")
    H, S = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss)).requires_grad_(True)
    eps, D, sol = nq.orbital_solution(H, S, op, n_occ, return_solution=True)
    pop, nelec, eband = nq.populations(D, plan, S, H, sol)
    q = nq.mulliken_charges(z, pop)
    t_q, t_d = l_q(q, dev(q_t), aptr), l_d(D, dev(pack(D_t)), op)
    loss = t_q + t_d + (nelec * dev(w_ne)).sum() + (eband * dev(w_eb)).sum()
    loss.backward()
    sol.check()
    ref_total, worst = 0.0, np.zeros(2)
    for b, m in enumerate(ms):
        atoms = slice(int(aptr[b]), int(aptr[b + 1]))
        ends = np.concatenate([[0], np.cumsum(per_atom[atoms])])
        zt, qt, Dt = torch.from_numpy(z[atoms].astype(np.float64)), torch.from_numpy(q_t[atoms]), torch.from_numpy(D_t[b])

        def mol_loss(eps_, D_, S_, H_, parts=None):
            rows = (D_ * S_).sum(1)
            pa = torch.stack([rows[i:j].sum() for i, j in zip(ends[:-1], ends[1:])])
            a, c = ((zt - pa - qt) ** 2).mean() / B, (D_ - Dt).abs().mean() / B
            if parts is not None:
                parts += [float(a), float(c)]
            return a + c + w_ne[b] * rows.sum() + w_eb[b] * (D_ * H_).sum()
        n = int(n_occ[b])
        fH, fS, e_ref, D_ref, gH, gS = DR.spread(Hs[b], Ss[b], n, mol_loss)
        parts = []
        ref_total += float(mol_loss(None, torch.from_numpy(D_ref), torch.from_numpy(Ss[b]), torch.from_numpy(Hs[b]), parts))
        uH, uS = DR.units(Hs[b], Ss[b], n, e_ref, gH, gS)
        dH = float(np.abs(blocks(H.grad.cpu().numpy(), ms)[b] - gH).max() / uH)
        dS = float(np.abs(blocks(S.grad.cpu().numpy(), ms)[b] - gS).max() / uS)
        worst = np.maximum(worst, [dH, dS])
        print(f"orbital_density_parity losses db {b} m={m} n_occ={n} gH {dH:.3g} (bound {max(BOUND, 4 * fH):.1f}) gS {dS:.3g} (bound {max(BOUND, 4 * fS):.1f})")
        assert dH <= max(BOUND, 4.0 * fH) and dS <= max(BOUND, 4.0 * fS), (b, dH, dS)
    print(f"orbital_density_parity losses loss {float(loss.detach()):.15g} dense formulas {ref_total:.15g} worst gH {worst[0]:.3f} gS {worst[1]:.3f}")
    assert abs(float(loss.detach()) - ref_total) <= 1e-9 * abs(ref_total)
    # the two losses alone, against numpy on the device's own quantities
    qd, Dd = q.detach().cpu().numpy(), blocks(D.detach().cpu().numpy(), ms)
    ref_q = np.mean([((qd[a:e] - q_t[a:e]) ** 2).mean() for a, e in zip(aptr[:-1], aptr[1:])])
    ref_d = np.mean([np.abs(Dd[b] - D_t[b]).mean() for b in range(B)])
    assert abs(float(t_q.detach()) - ref_q) <= 1e-12 * ref_q and abs(float(t_d.detach()) - ref_d) <= 1e-12 * ref_d
    assert abs(float(nq.MullikenChargeLoss("mae")(q, dev(q_t), aptr).detach()) - np.mean([np.abs(qd[a:e] - q_t[a:e]).mean() for a, e in zip(aptr[:-1], aptr[1:])])) <= 1e-12
    assert abs(float(nq.DensityMatrixLoss("mse")(D, dev(pack(D_t)), op).detach()) - np.mean([((Dd[b] - D_t[b]) ** 2).mean() for b in range(B)])) <= 1e-12


# ---- 8. the QHNet task ------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_density_task(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from nabladft_amd.orbitals import OrbitalState
    from test_qhnet_gpu import ORBITALS, load_case
    devc = torch.device(DEV)
    g, cfg, net, batch = load_case("small", devc)
    per_atom = np.array([sum(2 * l + 1 for l in ORBITALS[int(a)]) for a in g["z"]])
    ends = np.cumsum(g["sizes"])
    sizes_orb = [int(per_atom[e - n:e].sum()) for n, e in zip(g["sizes"], ends)]
    batch.hamiltonian, batch.overlap, o = [], [], 0
    rng = np.random.Generator(np.random.PCG64(6))
    for m in sizes_orb:
        batch.hamiltonian.append(g["target"][o:o + m, o:o + m].astype(np.float32))
        A = rng.normal(size=(m, m)) * 0.1 / np.sqrt(m)
        batch.overlap.append((np.eye(m) + A + A.T).astype(np.float32))       # a well conditioned overlap
        o += m
    charge = [0, -1, 1]                                           # the fixture's molecules hold 92, 9 and 31 electrons: closed shells as anion and cation
    coefs = {"hamiltonian": 1.0, "orbital_energies": 0.25, "density_matrix": 0.5, "mulliken_charges": 2.0}
    losses = {"hamiltonian": HamiltonianLoss(), "orbital_energies": nq.OrbitalEnergyLoss("mae", "occupied", charge),
              "density_matrix": nq.DensityMatrixLoss("mse", charge), "mulliken_charges": nq.MullikenChargeLoss("mse", charge)}
    make = lambda cls, ls, cs: cls("QHNet", net, None, None, ls, None, None, cs)
    task = make(nq.QHNetDensityLightning, losses, coefs)
    solves = []
    real = OrbitalState.solve
    monkeypatch.setattr(OrbitalState, "solve", lambda self, *a, **k: (solves.append(1), real(self, *a, **k))[1])
    loss = task.training_step(batch, 0)
    assert len(solves) == 2, len(solves)                           # one solve of the prediction, one of the target, for three orbital terms
    # the terms by hand, on the quantities the step hands to the losses
    preds, targets, loss_args = task._evaluate(batch)
    assert len(solves) == 4
    pred = preds["hamiltonian"]
    plan = net.last_plan
    n_occ = nq.occupied_counts(batch.z, batch.ptr, charge, plan)
    assert n_occ.tolist() == [46, 5, 15]
    op = np.asarray(plan.mol_orb_ptr.cpu().numpy(), dtype=np.int64)
    terms = {"hamiltonian": losses["hamiltonian"](pred, targets["hamiltonian"], None),
             "orbital_energies": losses["orbital_energies"](preds["orbital_energies"], targets["orbital_energies"], n_occ, op),
             "density_matrix": losses["density_matrix"](preds["density_matrix"], targets["density_matrix"], op),
             "mulliken_charges": losses["mulliken_charges"](preds["mulliken_charges"], targets["mulliken_charges"], batch.ptr)}
    assert all(not targets[k].requires_grad for k in targets) and all(float(terms[k].detach()) > 0.0 for k in terms)
    hand = sum(coefs[k] * terms[k] for k in terms)
    print("orbital_density_parity qhnet task loss %.9g by hand %.9g (%s)" % (float(loss.detach()), float(hand.detach()),
                                                                             " ".join(f"{k} {float(v.detach()):.6g}" for k, v in terms.items())))
    assert torch.allclose(loss.detach().double(), hand.detach().double(), rtol=1e-6, atol=0.0)
    # the gradient arriving at the predicted Hamiltonian from the three orbital terms against route (a) on a host copy
    orbital = sum(coefs[k] * terms[k] for k in terms if k != "hamiltonian")
    got = torch.autograd.grad(orbital, pred)[0]
    assert got.dtype == pred.dtype
    ms, B = np.diff(op), len(op) - 1
    Hp = blocks(pred.detach().double().cpu().numpy(), ms)
    Sp = blocks(net._asm.pack_targets(plan, batch.overlap).double().cpu().numpy(), ms)
    e_t, D_t, q_t = (targets[k].double().cpu().numpy() for k in ("orbital_energies", "density_matrix", "mulliken_charges"))
    zz, aptr = np.asarray(g["z"], dtype=np.float64), np.concatenate([[0], ends])
    sym = lambda a: np.tril(a) + np.tril(a, -1).T                  # what the solver reads
    for b, m in enumerate(ms):
        n = int(n_occ[b])
        atoms = slice(int(aptr[b]), int(aptr[b + 1]))
        bounds = np.concatenate([[0], np.cumsum(per_atom[atoms])])
        et, Dt = torch.from_numpy(e_t[op[b]:op[b + 1]]), torch.from_numpy(blocks(D_t, ms)[b])
        zt, qt = torch.from_numpy(zz[atoms]), torch.from_numpy(q_t[atoms])

        def mol_loss(eps_, D_, S_, H_):
            rows = (D_ * S_).sum(1)
            pa = torch.stack([rows[i:j].sum() for i, j in zip(bounds[:-1], bounds[1:])])
            return (coefs["orbital_energies"] * (eps_[:n] - et[:n]).abs().mean() + coefs["density_matrix"] * ((D_ - Dt) ** 2).mean()
                    + coefs["mulliken_charges"] * ((zt - pa - qt) ** 2).mean()) / B
        H64, S64 = sym(Hp[b]), sym(Sp[b])
        fH, _, e_ref, _, gH, gS = DR.spread(H64, S64, n, mol_loss)
        uH, _ = DR.units(H64, S64, n, e_ref, gH, gS)
        gd = blocks(got.double().cpu().numpy(), ms)[b]
        fig = float((np.maximum(np.abs(gd - gH) - 2.0 ** -24 * np.abs(gH), 0.0) / uH).max())
        rel = float(np.abs(gd - gH).max() / np.abs(gH).max())       # float32 results: about 2^-24 is all there is to see
        print(f"orbital_density_parity qhnet task gradient at the predicted Hamiltonian molecule {b} m={m} n_occ={n} gap {e_ref[n] - e_ref[n - 1]:.3f} "
              f"gH {fig:.3g} (bound {max(BOUND, 4 * fH):.1f}) beyond the float32 rounding; max error / max|gH| {rel:.2e}")
        assert fig <= max(BOUND, 4.0 * fH), (b, fig)
    # all three coefficients at 0: QHNetLightning's loss, bit for bit, and nothing is solved
    plain = make(nq.QHNetLightning, {"hamiltonian": HamiltonianLoss()}, {"hamiltonian": 1.0})
    zero = make(nq.QHNetDensityLightning, losses, {"hamiltonian": 1.0, "orbital_energies": 0.0, "density_matrix": 0.0, "mulliken_charges": 0.0})
    before = len(solves)
    a, b = plain.training_step(batch, 0), zero.training_step(batch, 0)
    assert a.dtype == b.dtype and torch.equal(a.detach(), b.detach()) and len(solves) == before
    # the energies alone: the parent's step
    only = {"hamiltonian": 1.0, "orbital_energies": 0.25}
    two = {k: losses[k] for k in only}
    c, d = make(nq.QHNetOrbitalLightning, two, only).training_step(batch, 0), make(nq.QHNetDensityLightning, two, only).training_step(batch, 0)
    assert torch.equal(c.detach(), d.detach())
