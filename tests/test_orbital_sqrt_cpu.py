"""CPU: the numpy restatement of the eigensolver-free square roots (tests/orbital_sqrt_ref.py) against ``np.linalg.eigh`` and ``scipy.linalg.sqrtm``, its
failure cases, the divergence of the symmetrised variants (the reason for the kernels' layout), and the public surface and host-side refusals of
``BatchedMatrixRoot`` / ``LowdinBasis.of(method=)`` / ``scf_target_iterative`` / ``scf_target_blocks`` / ``nq_orb_sqrt_*``.

Unit: ``u = m 2^-52 kappa_2(S) max|entry|`` (``orbital_sqrt_ref.unit``), the error any route to a function of S may leave; the yardsticks themselves are only
good to a fraction of it.  Bound of the restatement against either yardstick: 1 u.  Measured here: S^(1/2) <= 0.039 u, S^(-1/2) <= 0.036 u (worst at m = 2, 3;
<= 5e-3 u from m = 15 on), against sqrtm <= 0.05 u; 0..20 iterations for kappa <= 1e4, 23 at 1e6, 30 at 1e8.

A A = S and A^- S A^- = I: with dA, dA^- the errors above (<= 1 u each), A A - S = A dA + dA A and A^- S A^- - I = dA^- (S A^-) + (A^- S) dA^- up to second order,
so both are held to 2 m max|A| times the bound of the factor that carries the error."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.linalg
import torch

import orbital_sqrt_ref as R

BOUND = 1.0
EXPECTED_ITERS = {"m1": (0, 0), "identity": (0, 0), "kappa1e6": (20, 27), "kappa1e8": (27, 34)}


def test_restatement_against_eigh_and_sqrtm():
    worst = dict(half=0.0, inv=0.0, sqrtm=0.0, aa=0.0, asa=0.0)
    lines = []
    for name, S in R.cases():
        m = S.shape[0]
        half, inv, sol = R.roots(S)
        assert sol["status"] == 0 and sol["iters"] < 100, name       # the condition of the issue: every matrix but the deliberately bad ones converges
        eh, ei = R.eigh_roots(S)
        sq = scipy.linalg.sqrtm(S).real
        uh, ui = R.unit(S, eh), R.unit(S, ei)
        fig = dict(half=np.abs(half - eh).max() / uh, inv=np.abs(inv - ei).max() / ui, sqrtm=np.abs(half - sq).max() / uh,
                   aa=np.abs(half @ half - S).max() / (2.0 * m * np.abs(eh).max() * uh),
                   asa=np.abs(inv @ S @ inv - np.eye(m)).max() / (2.0 * m * np.abs(eh).max() * ui))
        for k, v in fig.items():
            worst[k] = max(worst[k], float(v))
            assert v <= BOUND, (name, k, v)
        assert np.array_equal(half, half.T) and np.array_equal(inv, inv.T), name
        d = np.array(sol["deltas"])
        assert len(d) == sol["iters"] + 1 and (sol["iters"] == 0 or np.all(d[:-1] != 0.0))
        lo, hi = EXPECTED_ITERS.get(name, (1, 22))
        assert lo <= sol["iters"] <= hi, (name, sol["iters"])
        lines.append(f"restatement {name} m={m} kappa={np.linalg.cond(S):.3g} iterations {sol['iters']} half {fig['half']:.3g} u inv_half {fig['inv']:.3g} u "
                     f"sqrtm {fig['sqrtm']:.3g} u |A A - S| {np.abs(half @ half - S).max():.3g}")
    lines.append("restatement worst: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for line in lines:
        print("orbital_sqrt_parity " + line)
    R.record("restatement", lines)
    # m = 1 and the identity stop at iteration 0 with exact results; a diagonal S gives diagonal roots
    assert np.array_equal(R.roots(R.identity_case())[0], np.eye(9)) and R.roots(np.array([[1.7]]))[0][0, 0] == np.sqrt(1.7)
    hd = R.roots(R.diagonal_case())[0]
    assert np.all(hd[~np.eye(12, dtype=bool)] == 0.0)


def test_an_indefinite_and_a_nan_overlap_do_not_converge():
    for S in (R.indefinite_case(), R.nan_case()):
        half, inv, sol = R.roots(S)
        assert sol["status"] in (1, 4) and np.isnan(half).all() and np.isnan(inv).all()
    assert R.roots(R.indefinite_case())[2]["status"] == 4 and R.roots(R.indefinite_case())[2]["iters"] == 100
    assert R.roots(np.zeros((3, 3)))[2]["status"] == 1                # c = 0
    assert R.roots(R.spd(12, 1e2, 3), max_iter=4)[2]["status"] == 4   # max_iter too small


def test_symmetrising_the_iterates_diverges():
    """Why the kernels keep Y and Z as general matrices: with the lower triangle of Y T and T Z mirrored, or with (X + X^T) / 2, the iteration leaves its rounding
    floor a few steps after reaching it and overflows, where the unsymmetrised iteration on the same matrix stops at the floor."""
    for kappa in (1e4, 1e6):
        S = R.spd(40, kappa, 7)
        plain = R.roots(S)[2]
        assert plain["status"] == 0
        for variant in ("mirror", "average"):
            sol = R.roots(S, symmetrize=variant)[2]
            d = np.abs(np.array(sol["deltas"]))
            assert sol["status"] == 4 and not np.isfinite(d[-1]), (kappa, variant)
            if kappa == 1e4:
                assert np.nanmin(d) < 1e-6, variant                   # it reached the neighbourhood of its floor (2e-8) and left it again
            else:
                assert np.nanmin(d) > R.TOL * 40, variant             # it never came near (0.04 and 1.7)
    for kappa in (1e1, 1e2):                                          # below that the variants are harmless: the finding is about ill-conditioned S
        assert all(R.roots(R.spd(40, kappa, 7), symmetrize=v)[2]["status"] == 0 for v in ("mirror", "average"))


def test_public_surface():
    import nabladft_amd as nq
    from nabladft_amd import _lib, orbital_loss as OL, orbitals as O
    assert nq.BatchedMatrixRoot is O.BatchedMatrixRoot and nq.scf_target_blocks is OL.scf_target_blocks
    for name in ("BatchedMatrixRoot", "scf_target_blocks", "scf_target_iterative"):
        assert name in nq.__all__ and name in OL.__all__
    assert "BatchedMatrixRoot" in O.__all__
    sig = inspect.signature(O.BatchedMatrixRoot.__init__).parameters
    assert list(sig)[:3] == ["self", "orb_ptr", "device"]
    for name, names in (("prepare", ["self", "S_packed", "max_iter"]), ("run", ["self", "S_packed", "max_iter"]), ("step", ["self", "k"])):
        sig = inspect.signature(getattr(O.BatchedMatrixRoot, name)).parameters
        assert list(sig) == names and ("max_iter" not in sig or sig["max_iter"].default == 100), name
    for name in ("iterations", "status", "info", "residuals"):
        assert isinstance(getattr(O.BatchedMatrixRoot, name), property), name
    assert callable(O.BatchedMatrixRoot.check) and callable(O.BatchedMatrixRoot.finish)
    sig = inspect.signature(O.LowdinBasis.of).parameters
    assert list(sig) == ["S_packed", "plan_or_orb_ptr", "method", "max_iter"] and sig["method"].default == "eigh" and sig["max_iter"].default == 100
    assert list(inspect.signature(OL.scf_target).parameters) == ["H_target", "S", "plan", "n_occ"]           # unchanged
    sig = inspect.signature(OL.scf_target_iterative).parameters
    assert list(sig) == ["H_target", "S", "plan", "n_occ", "max_iter"] and sig["max_iter"].default == 100 and nq.scf_target_iterative is OL.scf_target_iterative
    sig = inspect.signature(OL.ScfResidualLoss.__init__).parameters
    assert list(sig) == ["self", "kind", "charge", "target_method"] and sig["target_method"].default == "solve"
    assert OL.ScfResidualLoss("mse", 0, "iterative").target_method == "iterative" and OL.ScfResidualLoss().target_method == "solve"
    assert OL.ScfTarget._fields == ("basis", "DL") and callable(OL.ScfTarget.check)
    lib = _lib.load()
    for sym in ("nq_orb_sqrt_init", "nq_orb_sqrt_step", "nq_orb_sqrt_run", "nq_orb_sqrt_finish"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert lib.nq_abi_version() == 17
    assert "1e8" in " ".join(O.BatchedMatrixRoot.__doc__.split()) and "Newton-Schulz" in O.__doc__ and "a later piece" not in O.__doc__


def test_cpu_tensors_and_bad_arguments_are_refused():
    import nabladft_amd as nq
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.BatchedMatrixRoot([0, 2], "cpu")
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.LowdinBasis.of(torch.zeros(4, dtype=torch.float64), [0, 2], method="newton_schulz")
    with pytest.raises(RuntimeError, match="MI355X only"):
        nq.scf_target_iterative(torch.zeros(4), torch.zeros(4), [0, 2], [1])
    with pytest.raises(ValueError, match="target_method"):
        nq.ScfResidualLoss("mse", 0, "newton")


def test_scf_target_blocks_on_the_host():
    """The helper only slices and copies: a stand-in target on the CPU shows the layout it hands to a data pipeline."""
    from types import SimpleNamespace
    import nabladft_amd as nq
    ms = [2, 3]
    op, pp = np.array([0, 2, 5]), np.array([0, 4, 13])
    inv, half, DL = (torch.arange(13, dtype=torch.float64) + o for o in (0.0, 100.0, 200.0))
    basis = SimpleNamespace(inv_half=inv, half=half, orbitals=SimpleNamespace(pack_ptr=pp, orb_ptr=op))
    out = nq.scf_target_blocks(nq.ScfTarget(basis, DL))
    assert set(out) == set(nq.QHNetCommutatorLightning.CACHED)
    for name, src in (("lowdin_inv_half", inv), ("lowdin_half", half), ("target_density_lowdin", DL)):
        assert [tuple(t.shape) for t in out[name]] == [(m, m) for m in ms]
        assert all(t.dtype == torch.float64 and t.device.type == "cpu" for t in out[name])
        assert torch.equal(torch.cat([t.reshape(-1) for t in out[name]]), src)


def test_host_side_argument_checks():
    """Every entry point checks its arguments on the host before any device work: no GPU is needed to be refused, and a refused call touches nothing."""
    from nabladft_amd import _lib
    lib = _lib.load()
    B, M, P = 2, 5, 13
    buf = (C.c_double * 128)()
    a = [C.c_void_p(C.addressof(buf) + 64 * i) for i in range(12)]
    st, S, Y, Z, T, Y2, Z2, ctl, log, half, inv = a[:11]
    err = lambda: lib.nq_last_error().decode()
    bad = _lib.NQ_ERR_ARG
    assert lib.nq_orb_sqrt_init(None, B, M, P, S, 1, 100, Y, Z, ctl, log, None) == bad and "null" in err()
    assert lib.nq_orb_sqrt_init(st, B, M, P, None, 1, 100, Y, Z, ctl, log, None) == bad and "null" in err()
    assert lib.nq_orb_sqrt_init(st, B, M, P, S, 1, 100, S, Z, ctl, log, None) == bad and "different arrays" in err()
    assert lib.nq_orb_sqrt_init(st, B, M, P, S, 1, 100, Y, Y, ctl, log, None) == bad and "different arrays" in err()
    assert lib.nq_orb_sqrt_init(st, B, M, P, S, 1, 0, Y, Z, ctl, log, None) == bad and "max_iter" in err()
    assert lib.nq_orb_sqrt_init(st, B, M, P, S, 1, 10001, Y, Z, ctl, log, None) == bad and "max_iter" in err()
    assert lib.nq_orb_sqrt_init(st, 0, M, P, S, 1, 100, Y, Z, ctl, log, None) == bad and "empty batch" in err()
    assert lib.nq_orb_sqrt_init(st, B, M, 3, S, 1, 100, Y, Z, ctl, log, None) == bad and "does not fit" in err()
    assert lib.nq_orb_sqrt_step(st, B, M, P, 5, 5, Y, Z, T, Y2, Z2, ctl, log, None) == bad and "iteration" in err()
    assert lib.nq_orb_sqrt_step(st, B, M, P, -1, 5, Y, Z, T, Y2, Z2, ctl, log, None) == bad and "iteration" in err()
    assert lib.nq_orb_sqrt_step(st, B, M, P, 0, 5, Y, Z, None, Y2, Z2, ctl, log, None) == bad and "null" in err()
    assert lib.nq_orb_sqrt_step(st, B, M, P, 0, 5, Y, Z, T, Y, Z2, ctl, log, None) == bad and "different arrays" in err()
    assert lib.nq_orb_sqrt_step(st, B, M, P, 0, 5, Y, Z, Z, Y2, Z2, ctl, log, None) == bad and "different arrays" in err()
    assert lib.nq_orb_sqrt_run(st, B, M, P, 5, Y, Z, T, Y2, Z2, None, log, None) == bad and "null" in err()
    assert lib.nq_orb_sqrt_run(st, B, M, P, 5, Y, Z, T, Y2, Y2, ctl, log, None) == bad and "different arrays" in err()
    assert lib.nq_orb_sqrt_run(st, B, M, P, 0, Y, Z, T, Y2, Z2, ctl, log, None) == bad and "max_iter" in err()
    assert lib.nq_orb_sqrt_run(st, 3, 2, P, 5, Y, Z, T, Y2, Z2, ctl, log, None) == bad
    assert lib.nq_orb_sqrt_finish(st, B, M, P, 5, Y, Z, Y2, Z2, ctl, log, None, inv, None) == bad and "null" in err()
    assert lib.nq_orb_sqrt_finish(st, B, M, P, 5, Y, Z, Y2, Z2, ctl, log, half, half, None) == bad and "different arrays" in err()
    assert lib.nq_orb_sqrt_finish(st, B, M, P, 5, Y, Z, Y2, Z2, ctl, log, Y, inv, None) == bad and "different arrays" in err()
    assert lib.nq_orb_sqrt_finish(st, B, M, P, 5, None, Z, Y2, Z2, ctl, log, half, inv, None) == bad and "null" in err()
    assert all(v == 0.0 for v in buf)
