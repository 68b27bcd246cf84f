"""GPU: the eigensolver-free square roots (csrc/orbsqrt.hip, ``BatchedMatrixRoot``, ``LowdinBasis.of(method="newton_schulz")``) and the SCF target without any
solve (``scf_target_iterative``, ``ScfResidualLoss(target_method="iterative")``, ``scf_target_blocks``).

Single launches are compared with numpy on the SAME operands: bit for bit on small integers, within the dot-product bound (K + 4) 2^-53 sum |terms| on random data
(extended precision up to m = 130, float64 numpy at m = 1024).  End to end the unit is ``u = m 2^-52 kappa_2(S) max|entry|`` (tests/orbital_sqrt_ref.py); the bound
is 10 times the restatement's own worst deviation from ``eigh`` on the same matrices (the project's margin for another summation order; 0.039 u for S^(1/2), 0.036 u
for S^(-1/2): tests/test_orbital_sqrt_cpu.py), floored at 1 u, the yardstick's own error scale.  The target is held to the units of the purification tests
(10 U_D, ``orbital_purify_ref.density_unit``) and its residual to the chain bound of the commutator tests.  Measured figures are printed as
``orbital_sqrt_parity ...`` lines (kept in profiles/orbital_sqrt_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import orbital_density_ref as DR
import orbital_lowdin_ref as LR
import orbital_purify_ref as PR
import orbital_sqrt_ref as R
from test_orbital_bond_gpu import SENTINEL, general, guarded, ld, make_batch, same_values, unguard, worst_ratio
from test_orbital_commutator_gpu import np_solution, residual_bound
from test_orbital_loss_gpu import blocks
from test_orbitals_gpu import BOUND, DEV, db_problems, dev, pack, same_bits

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 130]
E53 = 2.0 ** -53
TINY = np.finfo(np.float64).tiny
CTL = 24


def root_of(ms):
    from nabladft_amd.orbitals import BatchedMatrixRoot
    op = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    return BatchedMatrixRoot(op, DEV)


def one_step(ms, Ys, Zs):
    """Iteration 0 on the given (unsymmetric) operands -> (T, Y', Z', ctl): the iterates are written over what ``prepare`` left."""
    root = root_of(ms).prepare(dev(pack([np.eye(m) for m in ms])), 3)
    root.Y.copy_(dev(pack(Ys)))
    root.Z.copy_(dev(pack(Zs)))
    bufs = {}
    for name in ("T", "Y2", "Z2"):                                   # guarded outputs: nothing outside the packed range is written
        buf, view = guarded(root.state.P)
        bufs[name] = buf
        setattr(root, name, view)
    root.step(0)
    T, Y2, Z2 = (blocks(unguard(bufs[n], n), ms) for n in ("T", "Y2", "Z2"))
    assert same_bits(root.Y.cpu().numpy(), pack(Ys)) and same_bits(root.Z.cpu().numpy(), pack(Zs))      # the operands are not touched
    return T, Y2, Z2, root.ctl.cpu().numpy(), root


def operands(rng, m, integers):
    """Unsymmetric Y and Z with m - tr(Z Y) != 0, so that iteration 0 updates."""
    while True:
        Y, Z = general(rng, m, integers), general(rng, m, integers)
        if m - np.trace(R.mirror(Z @ Y)) != 0.0:
            return Y, Z


# ---- 1. single launches -----------------------------------------------------------------------------------------------------------------------------------------------
def test_one_iteration_exact_placement_with_small_integers():
    """Small integers (|entries| <= 3): Z Y <= 9 x 130, T a multiple of 1/2 below 600, Y T and T Z below 130 x 3 x 600: every partial sum is exact, so tile
    offsets, the orientation of the three operands, the transposed store of Z' and the mirrored T are compared with numpy bit for bit."""
    order = np.random.Generator(np.random.PCG64(900)).permutation(len(SIZES))
    ms = [SIZES[i] for i in order]
    rng = np.random.Generator(np.random.PCG64(1))
    ops = [operands(rng, m, True) for m in ms]
    T, Y2, Z2, ctl, root = one_step(ms, [o[0] for o in ops], [o[1] for o in ops])
    for b, m in enumerate(ms):
        Y, Z = ops[b]
        Tr, tr = R.t_matrix(Y, Z)
        assert same_values(T[b], Tr) and same_bits(T[b], T[b].T), (b, m)
        assert same_values(Y2[b], Y @ Tr) and same_values(Z2[b], Tr @ Z), (b, m)
        assert ctl[b, CTL] == m - tr and ctl[b, 2] == tr and ctl[b, 8:8 + (m + 63) // 64].sum() == tr, (b, m)
    assert root.iterations.cpu().tolist() == [1] * len(ms) and root.log[:, 0].cpu().tolist() == [1] * len(ms)


def test_one_iteration_within_the_dot_product_bound_and_at_the_largest_size():
    ms = [65, 17, 130, 1, 64, 1024, 127, 2]
    rng = np.random.Generator(np.random.PCG64(2))
    ops = [operands(rng, m, False) for m in ms]
    T, Y2, Z2, ctl, _ = one_step(ms, [o[0] for o in ops], [o[1] for o in ops])
    worst = np.zeros(4)
    for b, m in enumerate(ms):
        Y, Z = ops[b]
        cast = ld if m < 1024 else (lambda a: a)
        ZY = cast(Z) @ cast(Y)
        Tref = (0.5 * (3.0 * np.eye(m) - R.mirror(ZY))).astype(np.float64)
        bT = (m + 4) * E53 * 0.5 * R.mirror(np.abs(Z) @ np.abs(Y) + 3.0 * np.eye(m))
        Td = T[b]                                                   # the products are checked on the operand the device used
        Yref, Zref = (cast(Y) @ cast(Td)).astype(np.float64), (cast(Td) @ cast(Z)).astype(np.float64)
        bY, bZ = (m + 4) * E53 * (np.abs(Y) @ np.abs(Td)), (m + 4) * E53 * (np.abs(Td) @ np.abs(Z))
        f = [worst_ratio(T[b], Tref, bT), worst_ratio(Y2[b], Yref, bY), worst_ratio(Z2[b], Zref, bZ)]
        assert same_bits(T[b], T[b].T) and max(f) <= 1.0, (b, m, f)
        # the trace slots: partial sums of the diagonal of Z Y over each 64-wide tile; delta from the slots in slot order
        diag = np.diag(ZY)
        bdiag = (m + 4) * E53 * np.diag(np.abs(Z) @ np.abs(Y))
        nd, total = (m + 63) // 64, 0.0
        for d in range(nd):
            seg = slice(64 * d, min(64 * d + 64, m))
            err = abs(ctl[b, 8 + d] - float(diag[seg].sum()))
            allow = float(bdiag[seg].sum()) + 68 * E53 * float(np.abs(diag[seg]).sum())
            f.append(err / max(allow, TINY))
            assert err <= allow, (b, m, d)
            total += ctl[b, 8 + d]
        assert ctl[b, 2] == total and ctl[b, CTL] == float(m) - total, (b, m)
        assert not ctl[b, 8 + nd:CTL].any()
        worst = np.maximum(worst, [f[0], f[1], f[2], max(f[3:])])
    print("orbital_sqrt_parity one iteration worst error / bound (m <= 130 against extended precision, m = 1024 against float64 numpy): "
          f"T {worst[0]:.3f} Y' {worst[1]:.3f} Z' {worst[2]:.3f} trace slots {worst[3]:.3f}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_init_reads_the_lower_triangle_only(dtype):
    ms = [17, 1, 130, 64]
    Ss = [R.spd(m, 1e2, 50 + m).astype(dtype).astype(np.float64) for m in ms]
    clean = root_of(ms).prepare(dev(pack(Ss, dtype=dtype)), 5)
    dirty = root_of(ms).prepare(dev(pack(Ss, dtype=dtype, poison=float("nan"))), 5)
    for name in ("Y", "Z", "ctl"):
        assert same_bits(getattr(clean, name).cpu().numpy(), getattr(dirty, name).cpu().numpy()), name
    ctl, Y0, Z0 = dirty.ctl.cpu().numpy(), blocks(dirty.Y.cpu().numpy(), ms), blocks(dirty.Z.cpu().numpy(), ms)
    assert dirty.status.cpu().tolist() == [0] * 4 and not dirty.log.cpu().numpy().any() and not ctl[:, 2:].any()
    for b, m in enumerate(ms):
        c = float(np.abs(ld(Ss[b])).sum(axis=1).max())
        assert abs(ctl[b, 0] - c) <= (m + 4) * E53 * c and abs(ctl[b, 1] - np.sqrt(ctl[b, 0])) <= 2.0 * E53 * ctl[b, 1], (b, m)
        assert same_bits(Y0[b], R.mirror(Ss[b]) / ctl[b, 0]) and same_bits(Z0[b], np.eye(m)), (b, m)


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def end_to_end_reference():
    """Per matrix of ``orbital_sqrt_ref.cases`` (shuffled): the restatement, the yardstick, the units, and the restatement's own worst deviation in units."""
    cases = R.cases()
    order = np.random.Generator(np.random.PCG64(901)).permutation(len(cases))
    out, worst = [], np.zeros(2)
    for i in order:
        name, S = cases[i]
        half, inv, sol = R.roots(S)
        eh, ei = R.eigh_roots(S)
        uh, ui = R.unit(S, eh), R.unit(S, ei)
        worst = np.maximum(worst, [np.abs(half - eh).max() / uh, np.abs(inv - ei).max() / ui])
        out.append(dict(name=name, S=S, half=half, inv=inv, iters=sol["iters"], eh=eh, ei=ei, uh=uh, ui=ui))
    return out, worst


def test_roots_against_the_restatement_and_the_decomposition():
    import nabladft_amd as nq
    refs, own = end_to_end_reference()
    bound = np.maximum(10.0 * own, 1.0)                             # (S^(1/2), S^(-1/2)), in units
    ms = [r["S"].shape[0] for r in refs]
    Sd = dev(pack([r["S"] for r in refs], poison=float("nan")))
    root = root_of(ms).run(Sd).check()
    basis = nq.LowdinBasis.of(Sd, root.orb_ptr, method="newton_schulz").check()
    assert same_bits(basis.half.cpu().numpy(), root.half.cpu().numpy()) and same_bits(basis.inv_half.cpu().numpy(), root.inv_half.cpu().numpy())
    assert basis.cond is None and basis.orbitals.state.status.cpu().tolist() == [0] * len(ms)
    with pytest.raises(RuntimeError, match="no levels"):
        basis.s
    eig = nq.LowdinBasis.of(Sd, root.orb_ptr, method="eigh").check()
    old = nq.LowdinBasis.of(Sd, root.orb_ptr).check()
    assert same_bits(eig.half.cpu().numpy(), old.half.cpu().numpy()) and same_bits(eig.inv_half.cpu().numpy(), old.inv_half.cpu().numpy()) and eig.s is not None
    half, inv = blocks(root.half.cpu().numpy(), ms), blocks(root.inv_half.cpu().numpy(), ms)
    dh, di = blocks(eig.half.cpu().numpy(), ms), blocks(eig.inv_half.cpu().numpy(), ms)
    iters, deltas = root.iterations.cpu().numpy(), root.residuals.cpu().numpy()
    assert deltas.shape == (len(ms), 100) and root.status.cpu().tolist() == [0] * len(ms) and root.info.cpu().tolist() == [0] * len(ms)
    worst, lines = np.zeros(6), []
    for b, r in enumerate(refs):
        fig = np.array([np.abs(half[b] - r["half"]).max() / r["uh"], np.abs(inv[b] - r["inv"]).max() / r["ui"], np.abs(half[b] - r["eh"]).max() / r["uh"],
                        np.abs(inv[b] - r["ei"]).max() / r["ui"], np.abs(half[b] - dh[b]).max() / r["uh"], np.abs(inv[b] - di[b]).max() / r["ui"]])
        worst = np.maximum(worst, fig)
        lines.append(f"device {r['name']} m={ms[b]} iterations {int(iters[b])} (restatement {r['iters']}) half / inv_half in u against the restatement {fig[0]:.3g} "
                     f"{fig[1]:.3g}, numpy eigh {fig[2]:.3g} {fig[3]:.3g}, the device decomposition {fig[4]:.3g} {fig[5]:.3g}")
        print("orbital_sqrt_parity " + lines[-1])
        assert np.all(fig[0::2] <= bound[0]) and np.all(fig[1::2] <= bound[1]), (r["name"], fig)
        assert abs(int(iters[b]) - r["iters"]) <= 2, (r["name"], int(iters[b]), r["iters"])
        assert same_bits(half[b], half[b].T) and same_bits(inv[b], inv[b].T), r["name"]
        k = int(iters[b])
        assert np.all(deltas[b, k + 1:] == 0.0) and (k == 0 or np.all(deltas[b, :k] != 0.0)), r["name"]
    lines.append(f"device worst in u (bound {bound[0]:.3g} {bound[1]:.3g}): against the restatement {worst[0]:.3g} {worst[1]:.3g}, numpy eigh {worst[2]:.3g} "
                 f"{worst[3]:.3g}, the device decomposition {worst[4]:.3g} {worst[5]:.3g}")
    print("orbital_sqrt_parity " + lines[-1])
    R.record("device", lines)


# ---- 3. robustness -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_reproducible_batch_independent_and_failed_molecules_stay_alone():
    good = [R.spd(65, 1e3, 60), R.spd(17, 1e2, 61), R.spd(130, 1e4, 62), R.spd(64, 1e1, 63)]

    def run(mats, max_iter=100):
        ms = [a.shape[0] for a in mats]
        root = root_of(ms).run(dev(pack(mats)), max_iter)
        return root, blocks(root.half.cpu().numpy(), ms), blocks(root.inv_half.cpu().numpy(), ms)
    root, half, inv = run(good)
    root2, half2, inv2 = run(good)
    assert all(same_bits(x, y) for x, y in zip(half + inv, half2 + inv2)) and same_bits(root.residuals.cpu().numpy(), root2.residuals.cpu().numpy())
    for b in (0, 2, 3):                                              # alone: the same bits as inside the batch
        ra, ha, ia = run([good[b]])
        assert same_bits(ha[0], half[b]) and same_bits(ia[0], inv[b]) and int(ra.iterations[0]) == int(root.iterations[b]), b
    # an indefinite and a NaN molecule between them
    mixed = [good[0], R.indefinite_case(), good[1], R.nan_case(), good[2], good[3]]
    rm, hm, im = run(mixed, 40)
    status = rm.status.cpu().tolist()
    assert status == [0, 4, 0, 1, 0, 0] and rm.info.cpu().tolist() == [0, 1, 0, 0, 0, 0] and int(rm.iterations[1]) == 40
    for b, g in ((0, 0), (2, 1), (4, 2), (5, 3)):
        assert same_bits(hm[b], half[g]) and same_bits(im[b], inv[g]), b
    for b in (1, 3):
        assert np.isnan(hm[b]).all() and np.isnan(im[b]).all(), b
    with pytest.raises(RuntimeError, match="molecule 1: the Newton-Schulz iteration did not converge in 40"):
        rm.check()
    import nabladft_amd as nq
    basis = nq.LowdinBasis.of(dev(pack(mixed)), rm.orb_ptr, method="newton_schulz", max_iter=40)
    assert basis.info.cpu().tolist() == status
    with pytest.raises(RuntimeError, match="molecule 1"):
        basis.check()
    only_nan = run([good[1], R.nan_case()])[0]
    with pytest.raises(RuntimeError, match="molecule 1: the overlap matrix is not positive definite"):
        only_nan.check()
    # max_iter too small: status 4 for everybody who iterates
    short = run(good, 3)[0]
    assert short.status.cpu().tolist() == [4] * 4 and short.info.cpu().tolist() == [1] * 4


def test_dimension_mismatch_touches_nothing_and_python_refusals():
    from nabladft_amd import _lib
    root = root_of([5, 3]).prepare(dev(pack([np.eye(5), np.eye(3)])), 4)
    st, lib = root.state, _lib.load()
    arrays = [torch.full((40,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(8)]
    log = torch.full((8,), -77, dtype=torch.int32, device=DEV)
    S = torch.ones(40, dtype=torch.float64, device=DEV)
    p = [_lib.ptr(a) for a in arrays]
    wrong = (2, 8, 36)                                               # instead of (2, 8, 34)
    calls = ((lib.nq_orb_sqrt_init, (_lib.ptr(S), 1, 4, p[0], p[1], p[5], _lib.ptr(log))),
             (lib.nq_orb_sqrt_step, (0, 4, p[0], p[1], p[2], p[3], p[4], p[5], _lib.ptr(log))),
             (lib.nq_orb_sqrt_run, (4, p[0], p[1], p[2], p[3], p[4], p[5], _lib.ptr(log))),
             (lib.nq_orb_sqrt_finish, (4, p[0], p[1], p[3], p[4], p[5], _lib.ptr(log), p[6], p[7])))
    for fn, args in calls:
        assert fn(_lib.ptr(st.buf), *wrong, *args, _lib.stream_ptr()) == 0, lib.nq_last_error()
        torch.cuda.synchronize()
        assert int(st.header_dev[4]) == -2 and all(bool((a == SENTINEL).all()) for a in arrays) and bool((log == -77).all())
        with pytest.raises(RuntimeError, match="other dimensions"):
            st.header()
        st.header_dev[4] = 0
    with pytest.raises(ValueError, match="max_iter"):
        root.prepare(S[:34], 0)
    with pytest.raises(ValueError, match="entries"):
        root.prepare(S, 10)
    with pytest.raises(TypeError, match="float32 or float64"):
        root.prepare(S[:34].to(torch.int32), 10)
    with pytest.raises(RuntimeError, match="iteration"):
        root.step(4)
    with pytest.raises(RuntimeError, match="prepare"):
        root_of([2]).finish()
    import nabladft_amd as nq
    with pytest.raises(ValueError, match="method must be"):
        nq.LowdinBasis.of(S[:34], root.orb_ptr, method="sqrtm")
    with pytest.raises(ValueError, match="max_iter"):
        nq.scf_target_iterative(S[:34], S[:34], root.orb_ptr, [1, 1], max_iter=0)


# ---- 4. the target without a solve ----------------------------------------------------------------------------------------------------------------------------------------
def target_problems(which):
    """-> list of (tag, H, S, n_occ, seed)"""
    import nabladft_amd as nq
    if which == "synthetic":
        cases = [c for c in DR.CASES if 1 < c[1] < c[0]][:4]
        return [(f"m={c[0]} n_occ={c[1]} kappa0={c[3]:g}",) + tuple(DR.gapped_case(*c)) + (c[1], c[4]) for c in cases]
    out = []
    for i, (H, S, z) in enumerate(db_problems()[:5]):                 # the sixth molecule's overlap is indefinite (tests/test_orbital_lowdin_gpu.py)
        n_occ = int(nq.occupied_counts(np.asarray(z, dtype=np.int64), [0, len(z)], 0)[0])
        out.append((f"molecule {i} m={H.shape[0]} n_occ={n_occ}", H, S, n_occ, 800 + i))
    return out


@functools.lru_cache(maxsize=None)
def target_reference(which):
    out = []
    for tag, H, S, n_occ, seed in target_problems(which):
        m = H.shape[0]
        eps, _, D = np_solution(H, S, n_occ)
        A, Ai = LR.functions(S)[:2]
        DL = LR.congruence(A, D)[0]
        rng = np.random.Generator(np.random.PCG64(9300 + seed))
        Hp = H + 0.02 * np.abs(H).max() * LR.sym(rng.normal(size=(m, m)))
        out.append(dict(tag=tag, H=H, S=S, D=D, DL=DL, n_occ=n_occ, eps=eps, Hp=Hp, G=rng.normal(size=(m, m)), A=A, Ai=Ai, uD=PR.density_unit(H, S, n_occ, eps, DL)))
    return out


@pytest.mark.parametrize("which", ["synthetic", "database"])
def test_iterative_target_against_the_solved_one(which, monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedPurification, OrbitalState
    refs = target_reference(which)
    ms = [r["H"].shape[0] for r in refs]
    bt = make_batch(ms, [[m] for m in ms])
    nos = [r["n_occ"] for r in refs]
    Hd, Sd = dev(pack([r["H"] for r in refs])), dev(pack([r["S"] for r in refs]))
    solved = nq.scf_target(Hd, Sd, bt.op, nos).check()
    counts = dict(solve=0, orth=0)
    real_solve, real_orth = OrbitalState.solve, BatchedPurification.orthogonalize
    monkeypatch.setattr(OrbitalState, "solve", lambda self, *a, **k: (counts.__setitem__("solve", counts["solve"] + 1), real_solve(self, *a, **k))[1])
    monkeypatch.setattr(BatchedPurification, "orthogonalize", lambda self, *a, **k: (counts.__setitem__("orth", counts["orth"] + 1), real_orth(self, *a, **k))[1])
    target = nq.scf_target_iterative(Hd, Sd, bt.op, nos).check()
    assert counts == dict(solve=0, orth=0)                           # neither nq_orb_solve nor the orthogonaliser
    nq.scf_target(Hd, Sd, bt.op, nos)
    assert counts == dict(solve=2, orth=0)                           # the default is the solved target
    monkeypatch.undo()
    assert target.purification is not None and target.basis.root is not None and solved.purification is None
    DLi, DLs = blocks(target.DL.cpu().numpy(), ms), blocks(solved.DL.cpu().numpy(), ms)
    Hp = dev(pack([r["Hp"] for r in refs]))
    Gd = dev(pack([r["G"] for r in refs]))
    res = {}
    for key, tg in (("iterative", target), ("solve", solved)):
        Hq = Hp.clone().requires_grad_(True)
        Rm = nq.scf_residual_to_target(Hq, tg)
        ((Gd * Rm).sum() + 0.5 * (Rm * Rm).sum()).backward()
        res[key] = (blocks(Rm.detach().cpu().numpy(), ms), blocks(Hq.grad.cpu().numpy(), ms))
    R0 = blocks(nq.scf_residual_to_target(Hd, target).cpu().numpy(), ms)
    iters = target.purification.iterations.cpu().numpy()
    for b, r in enumerate(refs):
        m, n, uD = ms[b], r["n_occ"], r["uD"]
        X = 0.5 * DLi[b]
        Q = 0.5 * r["DL"]
        fig = [np.abs(DLi[b] - DLs[b]).max() / uD, np.abs(DLi[b] - r["DL"]).max() / uD]
        # X = Q + dX with |dX| <= BOUND U_D / 2 per entry: X X - X = Q dX + dX Q - dX to first order
        idem_allow = 0.5 * BOUND * uD * (2.0 * np.abs(Q).sum(axis=1).max() + 1.0)
        fig.append(np.abs(X @ X - X).max() / idem_allow)
        fig.append(abs(np.trace(DLi[b]) - 2.0 * n) / (m * BOUND * uD))
        bound0 = residual_bound(r["H"], r["S"], r["D"], n, r["eps"])[0]
        fig.append(worst_ratio(R0[b], np.zeros((m, m)), bound0 + TINY))
        # the residual of a perturbed H and its gradient: each target's is within its chain bound of the exact one, so the two agree within twice that
        boundp = residual_bound(r["Hp"], r["S"], r["D"], n, r["eps"])[0]
        fig.append(worst_ratio(res["iterative"][0][b], res["solve"][0][b], 2.0 * boundp + TINY))
        Ga = np.abs(0.5 * ((r["G"] + res["solve"][0][b]) - (r["G"] + res["solve"][0][b]).T))
        aAi, aD, J = np.abs(r["Ai"]), np.abs(r["DL"]), np.ones((m, m))
        kap = float(np.linalg.cond(r["S"]))
        gallow = BOUND * m * 2.0 ** -52 * kap * (aAi @ (Ga @ aD + aD @ Ga) @ aAi) + aAi @ (Ga @ (BOUND * uD * J) + (BOUND * uD * J) @ Ga + 2.0 * (boundp @ aD + aD @ boundp)) @ aAi
        fig.append(worst_ratio(res["iterative"][1][b], res["solve"][1][b], 2.0 * gallow + TINY))
        print(f"orbital_sqrt_parity target {which} {r['tag']} SP2 iterations {int(iters[b])}: DL against the solved target {fig[0]:.3g} U_D, against numpy {fig[1]:.3g} U_D "
              f"(bound {BOUND:g}); idempotency {fig[2]:.3g} and trace {fig[3]:.3g} of their allowances; |R| of the target's own H / chain bound {fig[4]:.3g}; "
              f"R and gH of a perturbed H between the two targets {fig[5]:.3g} {fig[6]:.3g} of their allowances")
        assert fig[0] <= BOUND and fig[1] <= BOUND and max(fig[2:]) <= 1.0, (r["tag"], fig)
        assert same_bits(DLi[b], DLi[b].T)


def test_a_gapless_target_and_a_bad_overlap_surface_through_check():
    import nabladft_amd as nq
    rng = np.random.Generator(np.random.PCG64(5))
    m, n = 33, 11
    lev = np.sort(rng.uniform(-5.0, 5.0, size=m))
    lev[n] = lev[n - 1]                                              # two equal levels across the Fermi level
    Qm = np.linalg.qr(rng.normal(size=(m, m)))[0]
    Hgap = LR.sym((Qm * lev[None, :]) @ Qm.T)
    case = [c for c in DR.CASES if 1 < c[1] < c[0]][0]
    Hok, Sok = DR.gapped_case(*case)
    ms = [m, Hok.shape[0], 20]
    op = np.concatenate([[0], np.cumsum(ms)])
    Hs, Ss, nos = [Hgap, Hok, np.diag(np.arange(20.0))], [np.eye(m), Sok, R.indefinite_case()], [n, case[1], 5]
    target = nq.scf_target_iterative(dev(pack(Hs)), dev(pack(Ss)), op, nos)
    DL = blocks(target.DL.cpu().numpy(), ms)
    assert target.purification.status.cpu().tolist()[0] == 4 and target.basis.info.cpu().tolist() == [0, 0, 4]
    assert np.isnan(DL[0]).all() and np.isfinite(DL[1]).all() and np.isnan(DL[2]).all()
    alone = nq.scf_target_iterative(dev(pack(Hs[1:2])), dev(pack(Ss[1:2])), [0, ms[1]], nos[1:2]).check()
    assert same_bits(alone.DL.cpu().numpy().reshape(ms[1], ms[1]), DL[1])
    with pytest.raises(RuntimeError, match="molecule 2"):            # the overlap is reported first
        target.check()
    only_gap = nq.scf_target_iterative(dev(pack(Hs[:2])), dev(pack(Ss[:2])), op[:3], nos[:2])
    with pytest.raises(RuntimeError, match="molecule 0: the purification did not converge"):
        only_gap.check()


# ---- 5. the QHNet task ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_qhnet_commutator_task_without_any_solve(monkeypatch):
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from nabladft_amd.orbitals import BatchedMatrixRoot, BatchedPurification, OrbitalState
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
    coefs = {"hamiltonian": 1.0, "scf_residual": 0.7}
    make = lambda method: nq.QHNetCommutatorLightning("QHNet", net, None, None, {"hamiltonian": HamiltonianLoss(),
                                                                                 "scf_residual": nq.ScfResidualLoss("mse", charge, target_method=method)}, None, None, coefs)
    counts = dict(solve=0, orth=0, root=0)
    for cls, name, key in ((OrbitalState, "solve", "solve"), (BatchedPurification, "orthogonalize", "orth"), (BatchedMatrixRoot, "run", "root")):
        real = getattr(cls, name)
        monkeypatch.setattr(cls, name, (lambda real, key: lambda self, *a, **k: (counts.__setitem__(key, counts[key] + 1), real(self, *a, **k))[1])(real, key))
    params = [p for p in net.parameters() if p.requires_grad]

    def step(task):
        for p in params:
            p.grad = None
        loss = task.training_step(batch, 0)
        loss.backward()
        return loss.detach()
    task = make("iterative")
    loss_it = step(task)
    assert counts == dict(solve=0, orth=0, root=1) and bool(torch.isfinite(loss_it))      # zero solves in the step
    Rit = task._evaluate(batch)[0]["scf_residual"].detach()
    loss_sv = step(make("solve"))
    assert counts["solve"] == 2 and counts["root"] == 2
    Rsv = make("solve")._evaluate(batch)[0]["scf_residual"].detach()
    # the two residuals agree within twice the chain bound of item 4, carried into the mean of squares of the loss term
    op = np.concatenate([[0], np.cumsum(ms)])
    n_occ = nq.occupied_counts(batch.z, batch.ptr, charge, op)
    plan, asm = net.last_plan, net._asm
    Hpred = task._evaluate(batch)[0]["hamiltonian"].detach().double().cpu().numpy()
    allow = []
    for b, m in enumerate(ms):
        h, s = LR.lower_sym(batch.hamiltonian[b].astype(np.float64)), LR.lower_sym(batch.overlap[b].astype(np.float64))
        eps_b, _, Dn = np_solution(h, s, int(n_occ[b]))
        dR = 2.0 * residual_bound(LR.lower_sym(blocks(Hpred, ms)[b]), s, Dn, int(n_occ[b]), eps_b)[0]
        Rb = blocks(Rsv.cpu().numpy(), ms)[b]
        assert worst_ratio(blocks(Rit.cpu().numpy(), ms)[b], Rb, dR + TINY) <= 1.0, b
        allow.append(float((2.0 * np.abs(Rb) * dR + dR * dR).mean()))
    tol = 0.7 * float(np.mean(allow)) + 1e-6 * float(loss_sv.abs())          # the float32 sum of the two terms of the loss
    print(f"orbital_sqrt_parity qhnet task loss with the iterative target {float(loss_it):.9g}, with the solved one {float(loss_sv):.9g} (allowed difference {tol:.3g})")
    assert abs(float(loss_it) - float(loss_sv)) <= tol
    # scf_target_blocks fed back as the cached batch fields: no solve, no square root, the residual of the ScfTarget they came from bit for bit
    target = nq.scf_target_iterative(asm.pack_targets(plan, batch.hamiltonian), asm.pack_targets(plan, batch.overlap), op, n_occ).check()
    fields = nq.scf_target_blocks(target)
    assert set(fields) == set(nq.QHNetCommutatorLightning.CACHED)
    for name, v in fields.items():
        assert [tuple(t.shape) for t in v] == [(m, m) for m in ms] and all(t.dtype == torch.float64 and t.device.type == "cpu" for t in v)
        setattr(batch, name, v)
    before = dict(counts)
    preds = task._evaluate(batch)[0]
    assert counts == before
    want = nq.scf_residual_to_target(preds["hamiltonian"].detach(), target)
    assert same_bits(preds["scf_residual"].detach().cpu().numpy(), want.cpu().numpy())
    assert same_bits(preds["scf_residual"].detach().cpu().numpy(), Rit.cpu().numpy())       # and it is the uncached step's
