"""GPU: the weighted Gram kernel and the population kernel (csrc/orbdens.hip) through the C ABI and through nabladft_amd.orbitals / nabladft_amd.orbital_loss:
exact placement, the dot-product bound, bitwise reproducibility, a failed molecule, gradients end to end against the float64 yardstick
(tests/orbital_grad_ref.py, whose own spread tests/test_orbital_loss_cpu.py pins), the loss, densities and populations, the QHNet task and PhiSNet's flag.

Bounds.  Kernel: |X_ij - ref_ij| <= (K + 4) 2^-53 sum_k |w_k c_ki c_kj| with K = hi - lo, the dot-product bound gamma_{K+2} with two spare roundings; it holds
for any summation order.  Gradients: max(10, 4 x the spread of the two reference routes for that case, computed here on the host) in units of
U_H = m 2^-52 |S^-1|_2 max|g| and U_S = U_H |H|_2 |S^-1|_2; ten is the bound the project holds the solver to (test_orbitals_gpu.BOUND).  Densities and
populations: 10 in units of m 2^-52 times the magnitudes involved (D, W: the largest sum of absolute terms; atom_pop: the atom's sum |D||S|; nelec and the
charge sum: 2 n_occ; eband: 2 sum |eps|).  Every figure is printed as an ``orbital_grad_parity ...`` line (kept in
profiles/orbital_grad_parity.txt)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import orbital_grad_ref as G
import orbitals_ref as R
from test_orbitals_gpu import BOUND, DEV, GOLDEN, compare_batch, db_problems, dev, pack, ptrs, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 130]       # the workgroup tile edge is 64: 63, 64 and 65 are among them
SENTINEL = -7.25e300
GUARD = 64


def raw_wgram(orb, w0, w1=None, k_lo=None, k_hi=None, two_outputs=None):
    """nq_orb_wgram into sentinel-filled buffers with a guard band before and after -> (out0, out1 or None) as numpy [P]; asserts that the guards, and out1
    when no second weight vector is given, still hold the sentinel, and that no sentinel survives inside.  The blocks are packed back to back, so there is no
    room for a sentinel between two of them: a stray write into a neighbouring block is caught by the comparison of that block's values (bit for bit in the
    exact-placement and batch-independence tests), not by a guard."""
    from nabladft_amd import _lib
    st = orb.state
    two_outputs = w1 is not None if two_outputs is None else two_outputs
    bufs = [torch.full((st.P + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2 if two_outputs else 1)]
    outs = [b[GUARD:GUARD + st.P] for b in bufs]
    rc = _lib.load().nq_orb_wgram(_lib.ptr(st.buf), *st._dims, _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(k_lo), _lib.ptr(k_hi), _lib.ptr(outs[0]),
                                  _lib.ptr(outs[1]) if two_outputs else None, _lib.stream_ptr())
    assert rc == 0, _lib.load().nq_last_error()
    host = [b.cpu().numpy() for b in bufs]
    for h in host:
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL)
    if two_outputs and w1 is None:
        assert np.all(host[1] == SENTINEL)
    assert not np.any(host[0][GUARD:-GUARD] == SENTINEL)
    return host[0][GUARD:-GUARD].copy(), (host[1][GUARD:-GUARD].copy() if w1 is not None else None)


def blocks(flat, ms):
    out, o = [], 0
    for m in ms:
        out.append(flat[o:o + m * m].reshape(m, m))
        o += m * m
    return out


def state_with(ms, Cs):
    """A solver state of these sizes whose ``coeff`` is written directly (no solve): row k of a block = orbital k."""
    from nabladft_amd.orbitals import BatchedOrbitals
    op = np.concatenate([[0], np.cumsum(ms)])
    orb = BatchedOrbitals(op, DEV)
    orb.state.coeff.copy_(dev(np.concatenate([c.reshape(-1) for c in Cs])))
    return orb, op


def i32(a):
    return dev(np.asarray(a, dtype=np.int32))


def ranges(kind, ms):
    if kind == "full":
        return None, None
    if kind == "first":
        return [0] * len(ms), [1] * len(ms)
    if kind == "ragged_end":                                     # [0, n) with n % 4 != 0
        return [0] * len(ms), [m if m % 4 else max(1, m - 1 - (b % 2)) for b, m in enumerate(ms)]
    if kind == "ragged_start":                                   # [lo, hi) with lo % 4 != 0
        lo = [min(m, 1 + 2 * (b % 2)) for b, m in enumerate(ms)]
        return lo, [max(l, m - (b % 3)) for b, (l, m) in enumerate(zip(lo, ms))]
    return [m // 2 for m in ms], [m // 2 for m in ms]            # empty


# ---- 1. exact placement -------------------------------------------------------------------------------------------------------------------------------
def test_exact_placement_with_small_integers():
    """Small non-zero integers in C and w: every product and every partial sum is exact in float64, so the lane map, the tile offsets and the mirror are
    compared with numpy bit for bit."""
    ms = [5, 1, 65, 17, 130, 64]
    rng = np.random.Generator(np.random.PCG64(1))
    nz = lambda size, top: rng.integers(1, top + 1, size=size).astype(np.float64) * rng.choice([-1.0, 1.0], size=size)
    Cs = [nz((m, m), 3) for m in ms]
    orb, op = state_with(ms, Cs)
    w0, w1 = nz(int(op[-1]), 4), nz(int(op[-1]), 4)
    for kind in ("full", "ragged_start"):
        lo, hi = ranges(kind, ms)
        x0, x1 = raw_wgram(orb, dev(w0), dev(w1), None if lo is None else i32(lo), None if hi is None else i32(hi))
        for b, (m, Cm) in enumerate(zip(ms, Cs)):
            a, e = (0, m) if lo is None else (lo[b], hi[b])
            for x, w in ((x0, w0), (x1, w1)):
                ref = (Cm[a:e].T * w[op[b] + a:op[b] + e]) @ Cm[a:e] + 0.0
                assert same_bits(blocks(x, ms)[b], ref), (kind, b, m)


# ---- 2. the kernel's bound ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_batch():
    rng = np.random.Generator(np.random.PCG64(2))
    ms = [SIZES[i] for i in rng.permutation(len(SIZES))]
    Cs = [rng.normal(size=(m, m)) for m in ms]
    M = sum(ms)
    return ms, Cs, rng.normal(size=M), rng.normal(size=M) * np.exp(rng.normal(size=M))


def check_bound(tag, ms, Cs, op, w, x, lo, hi, wide=True):
    worst = 0.0
    for b, (m, Cm) in enumerate(zip(ms, Cs)):
        a, e = (0, m) if lo is None else (lo[b], hi[b])
        X = blocks(x, ms)[b]
        assert np.array_equal(X, X.T), (tag, b, m)               # exactly symmetric
        wk = w[op[b] + a:op[b] + e]
        if e <= a:
            assert same_bits(X, np.zeros((m, m))), (tag, b, m)     # an empty range: exact zeros
            continue
        ft = np.longdouble if wide else np.float64
        ref = ((Cm[a:e].T.astype(ft) * wk.astype(ft)) @ Cm[a:e].astype(ft)).astype(np.float64)
        mag = (np.abs(Cm[a:e]).T * np.abs(wk)) @ np.abs(Cm[a:e])
        fig = float((np.abs(X - ref) / ((e - a + 4) * 2.0 ** -53 * mag)).max())
        worst = max(worst, fig)
        assert fig <= 1.0, (tag, b, m, a, e, fig)
    print(f"orbital_grad_parity wgram {tag} worst error / bound {worst:.3f}")


@pytest.mark.parametrize("kind", ["full", "first", "ragged_end", "ragged_start", "empty"])
def test_kernel_bound_on_ragged_sizes_and_ranges(kind):
    ms, Cs, w0, w1 = random_batch()
    orb, op = state_with(ms, Cs)
    lo, hi = ranges(kind, ms)
    if lo is not None:
        assert all(0 <= l <= h <= m for l, h, m in zip(lo, hi, ms))
        if kind == "ragged_end":
            assert all(h % 4 for h in hi)
        if kind == "ragged_start":
            assert all(l % 4 for l in lo)
    klo, khi = (None, None) if lo is None else (i32(lo), i32(hi))
    x0, x1 = raw_wgram(orb, dev(w0), dev(w1), klo, khi)
    check_bound(f"{kind} w0", ms, Cs, op, w0, x0, lo, hi)
    check_bound(f"{kind} w1", ms, Cs, op, w1, x1, lo, hi)
    # one weight vector per launch: the same bits, and a second output that is given without a second weight vector stays untouched
    s0, _ = raw_wgram(orb, dev(w0), None, klo, khi, two_outputs=True)
    s1, _ = raw_wgram(orb, dev(w1), None, klo, khi)
    assert same_bits(s0, x0) and same_bits(s1, x1)
    # the Python call is the same launch
    y0, y1 = orb.weighted_gram(dev(w0), dev(w1), klo, khi)
    assert same_bits(y0.cpu().numpy(), x0) and same_bits(y1.cpu().numpy(), x1)


def test_kernel_bound_at_the_largest_size():
    """m = 1024 alone: sixteen tile rows, 136 workgroups, every row of the largest block.  The reference here is plain float64 numpy (an extended-precision
    product of this size takes too long for a test), so its own rounding shares the bound with the kernel's."""
    rng = np.random.Generator(np.random.PCG64(3))
    Cm = rng.normal(size=(1024, 1024))
    w0, w1 = rng.normal(size=1024), rng.normal(size=1024)
    orb, op = state_with([1024], [Cm])
    x0, x1 = raw_wgram(orb, dev(w0), dev(w1))
    check_bound("m=1024 w0", [1024], [Cm], op, w0, x0, None, None, wide=False)
    check_bound("m=1024 w1", [1024], [Cm], op, w1, x1, None, None, wide=False)


# ---- 3. bitwise ---------------------------------------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_batch_independent():
    ms, Cs, w0, w1 = random_batch()
    orb, op = state_with(ms, Cs)
    lo, hi = ranges("ragged_start", ms)
    a0, a1 = raw_wgram(orb, dev(w0), dev(w1), i32(lo), i32(hi))
    b0, b1 = raw_wgram(orb, dev(w0), dev(w1), i32(lo), i32(hi))
    assert same_bits(a0, b0) and same_bits(a1, b1)
    for b, (m, Cm) in enumerate(zip(ms, Cs)):
        alone, _ = state_with([m], [Cm])
        sl = slice(int(op[b]), int(op[b + 1]))
        c0, c1 = raw_wgram(alone, dev(w0[sl]), dev(w1[sl]), i32(lo[b:b + 1]), i32(hi[b:b + 1]))
        assert same_bits(c0.reshape(m, m), blocks(a0, ms)[b]) and same_bits(c1.reshape(m, m), blocks(a1, ms)[b]), (b, m)


# ---- 4. a molecule the solver failed on -----------------------------------------------------------------------------------------------------------------
def test_failed_molecule_gets_nan_and_leaves_its_neighbours_alone():
    from nabladft_amd.orbitals import BatchedOrbitals
    good = [R.case(m, 1e2, 800 + m) for m in (24, 65, 5, 63)]
    Hb, Sb = R.case(64, 1e2, 864)
    w, Q = np.linalg.eigh(Sb)
    w[3] = -0.25
    Sb = (Q * w[None, :]) @ Q.T
    Sb = 0.5 * (Sb + Sb.T)
    Hs, Ss = [g[0] for g in good], [g[1] for g in good]
    rng = np.random.Generator(np.random.PCG64(4))
    wg = rng.normal(size=sum(h.shape[0] for h in Hs))
    clean = BatchedOrbitals(ptrs(Hs)[0], DEV).solve(dev(pack(Hs)), dev(pack(Ss)))
    c0, c1 = raw_wgram(clean, dev(wg), dev(-wg))
    Hs.insert(2, Hb), Ss.insert(2, Sb)
    ms = [h.shape[0] for h in Hs]
    wb = np.concatenate([wg[:24 + 65], rng.normal(size=64), wg[24 + 65:]])
    orb = BatchedOrbitals(ptrs(Hs)[0], DEV).solve(dev(pack(Hs)), dev(pack(Ss)))
    assert orb.status.tolist() == [0, 0, 1, 0, 0]
    x0, x1 = raw_wgram(orb, dev(wb), dev(-wb))
    for x, c in ((x0, c0), (x1, c1)):
        got = blocks(x, ms)
        assert np.isnan(got[2]).all()
        for g, r in zip(got[:2] + got[3:], blocks(c, [24, 65, 5, 63])):
            assert same_bits(g, r)
    # through the differentiable call: NaN energies and a NaN gradient block for that molecule only
    from nabladft_amd.orbital_loss import orbital_energies
    H = dev(pack(Hs)).requires_grad_(True)
    eps, sol = orbital_energies(H, dev(pack(Ss)), ptrs(Hs)[0], return_solution=True)
    torch.nansum(eps).backward()
    gb = blocks(H.grad.cpu().numpy(), ms)
    assert np.isnan(gb[2]).all() and all(np.isfinite(g).all() for g in gb[:2] + gb[3:])
    with pytest.raises(RuntimeError, match="molecule 2"):
        sol.check()


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_gradients(dtype, kind, general=True):
    """Route (a) and the spread of the two routes for every case, once per (dtype, loss): [(H, S, eps, gH, gS, bound_H, bound_S, g)] on the inputs as the device
    sees them (float32: rounded)."""
    out = []
    for H, S in G.cases():
        if dtype == "float32":
            H, S = H.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
        S_ = S if general else None
        fH, fS, eps, gH, gS = G.spread(H, S_, kind)
        out.append((H, S_, eps, gH, gS, max(BOUND, 4.0 * fH), max(BOUND, 4.0 * fS), G.dloss(kind, eps)))
    return out


def batch_loss(kind, eps, op):
    return sum(G.loss_of(kind, eps[int(a):int(b)]) for a, b in zip(op[:-1], op[1:]))


@pytest.mark.parametrize("kind", G.LOSSES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gradients_end_to_end(dtype, kind):
    from nabladft_amd.orbital_loss import orbital_energies
    refs = reference_gradients(dtype, kind)
    Hs, Ss = [r[0] for r in refs], [r[1] for r in refs]
    ms = [h.shape[0] for h in Hs]
    op, _ = ptrs(Hs)
    tdt = getattr(torch, dtype)
    H = dev(pack(Hs), tdt).requires_grad_(True)
    S = dev(pack(Ss), tdt).requires_grad_(True)
    eps, sol = orbital_energies(H, S, op, return_solution=True)
    assert eps.dtype == torch.float64 and eps.requires_grad and not sol.coefficients.requires_grad
    batch_loss(kind, eps, op).backward()
    sol.check()
    assert H.grad.dtype == tdt and S.grad.dtype == tdt and H.grad.shape == H.shape and S.grad.shape == S.shape
    gHs, gSs = blocks(H.grad.double().cpu().numpy(), ms), blocks(S.grad.double().cpu().numpy(), ms)
    out_round = 2.0 ** -24 if dtype == "float32" else 0.0          # the float32 output's own rounding, per element
    for b, (Hm, Sm, e_ref, gH, gS, bH, bS, g) in enumerate(refs):
        uH, uS = G.units(Hm, Sm, g)
        fH = float((np.maximum(np.abs(gHs[b] - gH) - out_round * np.abs(gH), 0.0) / uH).max())
        fS = float((np.maximum(np.abs(gSs[b] - gS) - out_round * np.abs(gS), 0.0) / uS).max())
        print(f"orbital_grad_parity end-to-end {dtype} {kind} m={ms[b]} gH {fH:.3f} (bound {bH:.1f}) gS {fS:.3f} (bound {bS:.1f})")
        assert fH <= bH and fS <= bS, (dtype, kind, ms[b], fH, fS)
        assert np.array_equal(gHs[b], gHs[b].T) and np.array_equal(gSs[b], gSs[b].T)


def test_gradients_without_an_overlap_gradient_and_without_an_overlap():
    from nabladft_amd.orbital_loss import orbital_energies
    refs = reference_gradients("float64", "tanh")
    Hs, Ss = [r[0] for r in refs], [r[1] for r in refs]
    ms = [h.shape[0] for h in Hs]
    op, _ = ptrs(Hs)
    # S without requires_grad: no gS, the same gH bit for bit
    H, S = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss))
    batch_loss("tanh", orbital_energies(H, S, op), op).backward()
    H2, S2 = dev(pack(Hs)).requires_grad_(True), dev(pack(Ss)).requires_grad_(True)
    batch_loss("tanh", orbital_energies(H2, S2, op), op).backward()
    assert S.grad is None and S2.grad is not None and torch.equal(H.grad, H2.grad)
    # S = None: the standard problem against its own two reference routes
    std = reference_gradients("float64", "tanh", general=False)
    H3 = dev(pack(Hs)).requires_grad_(True)
    batch_loss("tanh", orbital_energies(H3, None, op), op).backward()
    for b, (Hm, _, _, gH, _, bH, _, g) in enumerate(std):
        fH = float(np.abs(blocks(H3.grad.cpu().numpy(), ms)[b] - gH).max() / G.units(Hm, None, g)[0])
        print(f"orbital_grad_parity end-to-end standard tanh m={ms[b]} gH {fH:.3f} (bound {bH:.1f})")
        assert fH <= bH, (ms[b], fH)


# ---- 6. the loss ----------------------------------------------------------------------------------------------------------------------------------------
def test_loss_matches_orbital_errors_and_selects_the_frontier():
    from nabladft_amd.orbital_loss import OrbitalEnergyLoss, orbital_energies
    from nabladft_amd.orbitals import OrbitalErrors
    probs = compare_batch()
    acc, terms = OrbitalErrors(), []
    for part in (probs[:5], probs[5:]):
        op, _ = ptrs([p[0] for p in part])
        z, ptr = [], [0]
        for p in part:                                           # helium atoms that give the n_occ of the batch
            z += [2] * p[3]
            ptr.append(len(z))
        Hp, Ht, S = dev(pack([p[1] for p in part])), dev(pack([p[0] for p in part])), dev(pack([p[2] for p in part]))
        acc.update(Hp, Ht, S, op, torch.tensor(z), torch.tensor(ptr))
        loss_fn = OrbitalEnergyLoss("mae", "occupied")
        n_occ = loss_fn.occupied(z, ptr, op)
        assert n_occ.tolist() == [p[3] for p in part]
        e_p, e_t = orbital_energies(Hp, S, op), orbital_energies(Ht, S, op)
        terms.append((float(loss_fn(e_p, e_t, n_occ, op)), len(part)))
        # the other selections, against numpy on the same energies
        ep, et = e_p.cpu().numpy(), e_t.cpu().numpy()
        d = [np.abs(ep[a:b] - et[a:b]) for a, b in zip(op[:-1], op[1:])]
        full = [len(x) for x in d]
        tol = 2 * max(full) * R.EPS
        ref_all = np.mean([x.mean() for x in d])
        ref_fr = np.mean([x[n - 1:n + 1].mean() for x, n in zip(d, n_occ.tolist())])
        ref_mse = np.mean([(x[:n] ** 2).mean() for x, n in zip(d, n_occ.tolist())])
        ref_homo = np.mean([x[-1] for x in d])                   # every orbital occupied: the HOMO alone
        assert abs(float(OrbitalEnergyLoss("mae", "all")(e_p, e_t, n_occ, op)) - ref_all) <= tol * ref_all
        assert abs(float(OrbitalEnergyLoss("mae", "frontier")(e_p, e_t, n_occ, op)) - ref_fr) <= tol * ref_fr
        assert abs(float(OrbitalEnergyLoss("mse", "occupied")(e_p, e_t, n_occ, op)) - ref_mse) <= tol * ref_mse
        assert abs(float(OrbitalEnergyLoss("mae", "frontier")(e_p, e_t, full, op)) - ref_homo) <= tol * ref_homo
    got = acc.compute()["eps_mae_occ"]
    mine = sum(v * n for v, n in terms) / sum(n for _, n in terms)
    print(f"orbital_grad_parity loss eps_mae_occ {got:.15g} OrbitalEnergyLoss {mine:.15g}")
    assert abs(got - mine) <= 2 * 141 * R.EPS * abs(got)


# ---- 7. density and populations -------------------------------------------------------------------------------------------------------------------------
def db_plan(probs):
    """What ``populations`` reads of a plan, for the database molecules: atoms per molecule and orbitals per atom from the database's basis table."""
    from nabladft_amd.data import HamiltonianDatabase
    db = HamiltonianDatabase(os.path.join(GOLDEN, "hamiltonian_db_6.db"))
    per_atom = [int(sum(2 * int(l) + 1 for l in db.get_orbitals(int(a)))) for p in probs for a in p[2]]
    n = [len(p[2]) for p in probs]
    m = [p[0].shape[0] for p in probs]
    plan = SimpleNamespace(B=len(probs), N=sum(n), m_total=sum(m), total=sum(x * x for x in m),
                           mol_ptr=i32(np.concatenate([[0], np.cumsum(n)])), orb_ptr=dev(np.concatenate([[0], np.cumsum(per_atom)]).astype(np.int64)))
    return plan, per_atom


def test_density_and_populations_on_the_database_molecules():
    import nabladft_amd as nq
    probs = db_problems()
    Hs, Ss = [p[0] for p in probs], [p[1] for p in probs]
    ms = [h.shape[0] for h in Hs]
    op, _ = ptrs(Hs)
    plan, per_atom = db_plan(probs)
    assert [sum(per_atom[a:b]) for a, b in zip(np.cumsum([0] + [len(p[2]) for p in probs])[:-1], np.cumsum([len(p[2]) for p in probs]))] == ms
    z = np.concatenate([np.asarray(p[2], dtype=np.int64) for p in probs])
    aptr = np.concatenate([[0], np.cumsum([len(p[2]) for p in probs])])
    n_occ = nq.occupied_counts(z, aptr, 0, op)
    Hd, Sd = dev(pack(Hs)), dev(pack(Ss, poison=1e30))            # only the lower triangle of S is read
    orb = nq.BatchedOrbitals(op, DEV).solve(Hd, Sd)
    assert orb.status.tolist() == [0, 0, 0, 0, 0, 1]               # the last molecule's overlap is indefinite (tests/test_orbitals_cpu.py)
    D, W = orb.density(n_occ, energy_weighted=True)
    assert same_bits(orb.density(n_occ).cpu().numpy(), D.cpu().numpy())
    pop, nelec, eband = orb.populations(D, plan, Sd, dev(pack(Hs, poison=1e30)))
    pop0, nelec0, eband0 = orb.populations(D, plan)
    assert eband0 is None
    # float32 S and H (the database stores float32, so the values are the same): bit for bit what their float64 copies give
    S32, H32 = dev(pack(Ss, np.float32)), dev(pack(Hs, np.float32))
    got32 = orb.populations(D, plan, S32, H32)
    ref32 = orb.populations(D, plan, S32.double(), H32.double())
    for a32, r32 in zip(got32, ref32):
        assert same_bits(a32.cpu().numpy(), r32.cpu().numpy())
    assert same_bits(got32[0].cpu().numpy(), pop.cpu().numpy())
    q = nq.mulliken_charges(z, pop).cpu().numpy()
    eps, coeff = orb.energies.cpu().numpy(), orb.coefficients.cpu().numpy()
    Db, Wb = blocks(D.cpu().numpy(), ms), blocks(W.cpu().numpy(), ms)
    pop, nelec, eband, pop0, nelec0 = (t.cpu().numpy() for t in (pop, nelec, eband, pop0, nelec0))
    o, pp, worst = 0, 0, np.zeros(6)
    for b, (H, S, zs) in enumerate(probs):
        m, n, na = ms[b], int(n_occ[b]), len(zs)
        atoms = slice(int(aptr[b]), int(aptr[b + 1]))
        if b == 5:
            assert np.isnan(Db[b]).all() and np.isnan(Wb[b]).all() and np.isnan(pop[atoms]).all() and np.isnan(nelec[b]) and np.isnan(eband[b])
            continue
        u = m * R.EPS
        Cm = coeff[pp:pp + m * m].reshape(m, m)[:n]                # rows = occupied orbitals, the device's own
        e = eps[o:o + m][:n]
        Dn, Wn = 2.0 * Cm.T @ Cm, 2.0 * (Cm.T * e) @ Cm
        f_d = np.abs(Db[b] - Dn).max() / (u * 2.0 * (np.abs(Cm).T @ np.abs(Cm)).max())
        f_w = np.abs(Wb[b] - Wn).max() / (u * 2.0 * ((np.abs(Cm).T * np.abs(e)) @ np.abs(Cm)).max())
        pop_mu = (Db[b] * S).sum(1)
        mag_mu = (np.abs(Db[b]) * np.abs(S)).sum(1)
        bounds = np.concatenate([[0], np.cumsum(per_atom[atoms])])
        pa = np.array([pop_mu[i:j].sum() for i, j in zip(bounds[:-1], bounds[1:])])
        ma = np.array([mag_mu[i:j].sum() for i, j in zip(bounds[:-1], bounds[1:])])
        f_p = (np.abs(pop[atoms] - pa) / (u * ma)).max()
        f_n = abs(nelec[b] - 2.0 * n) / (u * 2.0 * n)
        f_e = abs(eband[b] - 2.0 * e.sum()) / (u * 2.0 * np.abs(e).sum())
        f_q = abs(q[atoms].sum() - 0.0) / (u * 2.0 * n)
        fig = np.array([f_d, f_w, f_p, f_n, f_e, f_q])
        worst = np.maximum(worst, fig)
        print(f"orbital_grad_parity density db {b} m={m} n_occ={n} D {f_d:.3f} W {f_w:.3f} atom_pop {f_p:.3f} nelec {f_n:.3f} eband {f_e:.3f} charge sum {f_q:.3f}")
        assert np.all(fig <= BOUND), (b, fig)
        assert np.array_equal(Db[b], Db[b].T)
        # S = None: the populations are the diagonal of D, added per atom in order
        diag = np.diag(Db[b])
        assert same_bits(pop0[atoms], np.array([functools.reduce(lambda s, x: s + x, diag[i:j], 0.0) for i, j in zip(bounds[:-1], bounds[1:])]))
        assert abs(nelec0[b] - diag.sum()) <= u * np.abs(diag).sum()
        o, pp = o + m, pp + m * m
    print("orbital_grad_parity density worst D %.3f W %.3f atom_pop %.3f nelec %.3f eband %.3f charge sum %.3f" % tuple(worst))


def test_population_edges_and_the_dimension_mismatch_rule():
    """An atom whose orbital range leaves its molecule gets NaN, the atom before it its value; a call with other dimensions than nq_orb_init sets the header
    status to -2 and touches nothing, for nq_orb_wgram and nq_orb_population alike."""
    from nabladft_amd import _lib
    lib = _lib.load()
    ms, atoms_per = [5, 3], [2, 1]
    rng = np.random.Generator(np.random.PCG64(8))
    Cs = [rng.normal(size=(m, m)) for m in ms]
    orb, op = state_with(ms, Cs)
    st = orb.state
    D = orb.weighted_gram(dev(np.full(8, 2.0)))
    plan = SimpleNamespace(B=2, N=3, m_total=8, total=34, mol_ptr=i32([0, 2, 3]), orb_ptr=dev(np.array([0, 2, 5, 8], dtype=np.int64)))
    pop, nelec, _ = orb.populations(D, plan)
    bad = SimpleNamespace(**{**vars(plan), "orb_ptr": dev(np.array([0, 2, 6, 8], dtype=np.int64))})      # atom 1 runs one orbital into the next molecule
    pop_b, nelec_b, _ = orb.populations(D, bad)
    pop, pop_b = pop.cpu().numpy(), pop_b.cpu().numpy()
    assert same_bits(pop_b[:1], pop[:1]) and np.isnan(pop_b[1]) and np.isfinite(pop_b[2])      # atom 2's range [1, 3) of its own molecule is a valid one
    assert same_bits(nelec_b.cpu().numpy(), nelec.cpu().numpy())                               # the electron counts do not depend on the atom table
    # ---- other dimensions than init: (2, 8, 36) instead of (2, 8, 34) ----
    w = dev(np.ones(8))
    out = torch.full((36,), SENTINEL, dtype=torch.float64, device=DEV)
    assert lib.nq_orb_wgram(_lib.ptr(st.buf), 2, 8, 36, _lib.ptr(w), None, None, None, _lib.ptr(out), None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(st.header_dev[4]) == -2 and bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError, match="other dimensions"):
        st.header()
    st.header_dev[4] = 0
    outs = [torch.full((n,), SENTINEL, dtype=torch.float64, device=DEV) for n in (3, 2, 2)]
    Dd = torch.cat([D, D[:2]])
    rc = lib.nq_orb_population(_lib.ptr(st.buf), 2, 8, 36, _lib.ptr(Dd), _lib.ptr(Dd), 1, _lib.ptr(Dd), 1, 3, _lib.ptr(plan.mol_ptr), _lib.ptr(plan.orb_ptr),
                               _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert int(st.header_dev[4]) == -2 and all(bool((o == SENTINEL).all()) for o in outs)
    st.header_dev[4] = 0
    again = orb.weighted_gram(dev(np.full(8, 2.0)))                   # the right dimensions still work on that state
    assert torch.equal(again, D) and int(st.header_dev[4]) == 0


# ---- 8. the QHNet task and PhiSNet's flag -----------------------------------------------------------------------------------------------------------------
def test_qhnet_orbital_task_adds_the_two_terms():
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
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
    coef, charge = 0.25, [0, -1, 1]                               # the fixture's molecules hold 92, 9 and 31 electrons: closed shells as anion and cation
    make = lambda cls, losses, coefs: cls("QHNet", net, None, None, losses, None, None, coefs)
    both = make(nq.QHNetOrbitalLightning, {"hamiltonian": HamiltonianLoss(), "orbital_energies": nq.OrbitalEnergyLoss("mae", "occupied", charge)},
                {"hamiltonian": 1.0, "orbital_energies": coef})
    params = [p for p in net.parameters() if p.requires_grad]

    def grads(loss, retain=False):
        gs = torch.autograd.grad(loss, params, allow_unused=True, retain_graph=retain)
        return [torch.zeros_like(p) if x is None else x for p, x in zip(params, gs)]

    loss = both.training_step(batch, 0)
    g_both = grads(loss)
    # by hand through the public functions
    pred = net(batch, packed=True)
    plan = net.last_plan
    target = net._asm.pack_targets(plan, batch.hamiltonian)
    S = net._asm.pack_targets(plan, batch.overlap)
    l_h = HamiltonianLoss()(pred, target)
    n_occ = nq.occupied_counts(batch.z, batch.ptr, charge, plan)
    assert n_occ.tolist() == [46, 5, 15]
    eps_p, sol = nq.orbital_energies(pred, S, plan, return_solution=True)
    sol.check()
    eps_t = nq.BatchedOrbitals(plan, devc).solve(target, S).energies
    l_o = nq.OrbitalEnergyLoss("mae", "occupied")(eps_p, eps_t, n_occ, plan)
    assert l_o.dtype == torch.float64 and float(l_o.detach()) > 0.0
    hand = l_h + coef * l_o
    print(f"orbital_grad_parity qhnet task loss {float(loss.detach()):.9g} by hand {float(hand.detach()):.9g} (hamiltonian {float(l_h.detach()):.6g} orbital {float(l_o.detach()):.6g})")
    assert torch.allclose(loss.detach().double(), hand.detach().double(), rtol=1e-6, atol=0.0)
    g_h, g_o = grads(l_h, retain=True), grads(coef * l_o)                # the two terms share the network's graph
    assert any(float(x.abs().max()) > 0.0 for x in g_o)
    for p, a, b, c in zip(params, g_both, g_h, g_o):
        scale = float(torch.maximum(b.abs().max(), c.abs().max()))
        assert torch.allclose(a, b + c, rtol=1e-5, atol=1e-5 * scale), (tuple(p.shape), float((a - b - c).abs().max()), scale)
    # the orbital coefficient at 0: QHNetLightning's loss, bit for bit, and no eigenproblem is solved
    plain = make(nq.QHNetLightning, {"hamiltonian": HamiltonianLoss()}, {"hamiltonian": 1.0})
    zero = make(nq.QHNetOrbitalLightning, {"hamiltonian": HamiltonianLoss(), "orbital_energies": nq.OrbitalEnergyLoss()}, {"hamiltonian": 1.0, "orbital_energies": 0.0})
    a, b = plain.training_step(batch, 0), zero.training_step(batch, 0)
    assert a.dtype == b.dtype and torch.equal(a.detach(), b.detach())
    # no overlap on the batch: the identity
    del batch.overlap
    l_id = both.training_step(batch, 0)
    e_id = nq.orbital_energies(net(batch, packed=True), None, net.last_plan)
    assert torch.isfinite(l_id) and torch.isfinite(e_id).all() and float((l_id - loss).detach().abs()) > 0.0


def test_phisnet_orbital_gradients_flag():
    from nabladft_amd.data import HamiltonianDataset
    from nabladft_amd.phisnet import NeuralNetwork
    ds = HamiltonianDataset(os.path.join(GOLDEN, "hamiltonian_db_6.db"))
    torch.manual_seed(0)
    net = NeuralNetwork(max_orbitals=ds.max_orbitals * 2, order=2, num_features=32, num_basis_functions=8, num_modules=1, num_residual_pre_x=1,
                        num_residual_post_x=1, num_residual_pre_vi=1, num_residual_pre_vj=1, num_residual_post_v=1, num_residual_output=1, num_residual_pc=1,
                        num_residual_pn=1, num_residual_ii=1, num_residual_ij=1, num_residual_full_ii=1, num_residual_full_ij=1, num_residual_core_ii=1,
                        num_residual_core_ij=1, num_residual_over_ij=1, basis_functions="exp-bernstein", cutoff=8.0, activation="swish").cuda()
    with torch.no_grad():                 # a fresh network's output layers are zero (diagonal matrices, nothing to solve): give them small weights
        gen = torch.Generator(device="cuda").manual_seed(5)
        for p in net.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(0.02 * torch.randn(p.shape, generator=gen, device=p.device, dtype=p.dtype))
    b = ds.collate_fn([0, 1])
    batch = {k: (v.cuda() if torch.is_tensor(v) and k != "molecule_size" else v) for k, v in b.items()}
    assert net.orbital_gradients is False
    net.calculate_orbitals = True
    off = net(batch)
    assert not off["orbital_energies"].requires_grad and off["orbital_energies"].grad_fn is None
    net.orbital_gradients = True
    on = net(batch)
    assert on["orbital_energies"].grad_fn is not None and not on["orbital_coefficients"].requires_grad
    assert torch.equal(on["orbital_energies"].detach(), off["orbital_energies"]) and torch.equal(on["orbital_coefficients"], off["orbital_coefficients"])
    on["orbitals"].check()
    on["orbital_energies"].sum().backward()
    got = [p.grad for p in net.parameters() if p.grad is not None]
    assert got and all(bool(torch.isfinite(x).all()) for x in got) and any(float(x.abs().max()) > 0.0 for x in got)
    # orbital_gradients alone asks for nothing
    net.calculate_orbitals = False
    with torch.no_grad():
        none = net(batch)
    assert float(none["orbital_energies"].abs().max()) == 0.0 and "orbitals" not in none
