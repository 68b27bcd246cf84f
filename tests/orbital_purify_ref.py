"""Float64 numpy restatement of the eigensolver-free density route (nabladft_amd/csrc/orbpurify.hip, ``BatchedPurification``,
``purified_density_matrix``); test infrastructure shared by tests/test_orbital_purify_cpu.py and tests/test_orbital_purify_gpu.py.

Per molecule, H and S symmetric m x m, n_occ doubly occupied orbitals:

  orthogonaliser  S = L L^T, Z = L^-1 (lower triangular), Ht = Z H Z^T taken from its lower triangle (exactly symmetric); S = None: Z = I, Ht = H.
  bounds          Gershgorin e_min <= spec(Ht) <= e_max, X_0 = (e_max I - Ht) / (e_max - e_min).  n_occ <= 0: X = 0; n_occ >= m or e_max = e_min: X = I.
  iteration k     Y = X_k X_k, t = tr X_k, t2 = tr Y, delta_k = t - t2.  Stop with X = X_k when delta_k = 0, or when k >= 2 and |delta_k| >= |delta_k-1| and
                  |delta_k-1| < 1e-6 max(1, n_occ).  Otherwise X_k+1 = Y if |t2 - n_occ| <= |2 t - t2 - n_occ| (branch 1), else 2 X_k - Y (branch 2).
                  Not stopped after max_iter iterations: status 4.
  density         D = 2 Z^T X Z.
  gradient        Gt = 2 Z (G + G^T) / 2 Z^T; X1_0 = -Gt / (e_max - e_min); along the logged branches P = X_k X1_k, X1_k+1 = P + P^T (branch 1) or
                  2 X1_k - (P + P^T) (branch 2); g = the last X1; gH = Z^T g Z; gS = -Z^T (M + M^T + X Gt X) Z with M = g X Ht.
"""
import numpy as np

STOPPED = 3          # the log entry of the iteration that stopped (1, 2: the branch taken)


def lower_sym(A):
    """The symmetric matrix whose lower triangle is A's."""
    L = np.tril(A)
    return L + np.tril(A, -1).T


def orthogonalizer(S):
    """Z = L^-1 of S = L L^T, upper triangle zero; None for S = None."""
    if S is None:
        return None
    L = np.linalg.cholesky(np.asarray(S, dtype=np.float64))
    return np.tril(np.linalg.solve(L, np.eye(L.shape[0])))


def congruence(Z, A, trans, alpha=1.0):
    """alpha sym(Z A Z^T) (trans False) or alpha sym(Z^T A Z) (trans True), the lower triangle mirrored; Z None: alpha A."""
    if Z is None:
        return alpha * np.asarray(A, dtype=np.float64)
    return alpha * lower_sym(Z.T @ A @ Z if trans else Z @ A @ Z.T)


def bounds(Ht):
    """Gershgorin (e_min, e_max)."""
    d = np.diag(Ht)
    r = np.abs(Ht).sum(1) - np.abs(d)
    return float((d - r).min()), float((d + r).max())


def start(Ht, n_occ):
    """-> (X_0, e_min, e_max, kind): kind 0 iterate, 1 X = 0, 2 X = I."""
    m = Ht.shape[0]
    e_min, e_max = bounds(Ht)
    if n_occ <= 0:
        return np.zeros((m, m)), e_min, e_max, 1
    if n_occ >= m or e_max == e_min:
        return np.eye(m), e_min, e_max, 2
    return (e_max * np.eye(m) - Ht) / (e_max - e_min), e_min, e_max, 0


def step(X, n_occ, k, delta_prev):
    """One iteration -> (X_next, log entry, t, t2): the entry is 1 (Y), 2 (2 X - Y) or STOPPED (X unchanged)."""
    Y = lower_sym(X @ X)
    t, t2 = float(np.trace(X)), float(np.trace(Y))
    delta = t - t2
    if delta == 0.0 or (k >= 2 and abs(delta) >= abs(delta_prev) and abs(delta_prev) < 1e-6 * max(1, n_occ)):
        return X, STOPPED, t, t2
    if abs(t2 - n_occ) <= abs(2.0 * t - t2 - n_occ):
        return Y, 1, t, t2
    return 2.0 * X - Y, 2, t, t2


def purify(Ht, n_occ, max_iter=100):
    """-> dict(X, log, iters, status (0 or 4), e_min, e_max, kind, traces [(t, t2) per iteration])."""
    X, e_min, e_max, kind = start(Ht, n_occ)
    out = dict(e_min=e_min, e_max=e_max, kind=kind, log=[], traces=[], status=0, iters=0)
    if kind == 0:
        delta_prev, stopped = 0.0, False
        for k in range(max_iter):
            X, entry, t, t2 = step(X, n_occ, k, delta_prev)
            out["log"].append(entry)
            out["traces"].append((t, t2))
            delta_prev = t - t2
            if entry == STOPPED:
                stopped = True
                break
        out["iters"] = sum(1 for e in out["log"] if e != STOPPED)
        if not stopped:
            out["status"] = 4
            X = np.full_like(X, np.nan)
    out["X"] = X
    return out


def response(Ht, sol, Gt):
    """The final X1 = g for the symmetric upstream Gt in the orthonormal basis, along the logged branches (no traces, no decisions)."""
    m = Ht.shape[0]
    if sol["kind"] != 0:
        return np.zeros((m, m))
    X = (sol["e_max"] * np.eye(m) - Ht) / (sol["e_max"] - sol["e_min"])
    X1 = -Gt / (sol["e_max"] - sol["e_min"])
    for entry in sol["log"]:
        if entry == STOPPED:
            break
        Y = lower_sym(X @ X)
        P = X @ X1
        Q = lower_sym(P + P.T)
        if entry == 1:
            X, X1 = Y, Q
        else:
            X, X1 = 2.0 * X - Y, 2.0 * X1 - Q
    return X1


def density_and_gradients(H, S, n_occ, G=None, max_iter=100):
    """The whole route -> (D, gH, gS, sol): gH / gS None without G, gS None without S."""
    H = np.asarray(H, dtype=np.float64)
    Z = orthogonalizer(S)
    Ht = congruence(Z, lower_sym(H), False)
    sol = purify(Ht, n_occ, max_iter)
    D = congruence(Z, sol["X"], True, 2.0)
    if G is None or sol["status"] != 0:
        return D, None, None, sol
    Gt = congruence(Z, 0.5 * (G + G.T), False, 2.0)
    g = response(Ht, sol, Gt)
    gH = congruence(Z, g, True)
    gS = None
    if S is not None:
        M = g @ sol["X"] @ Ht
        gS = congruence(Z, 0.5 * ((2.0 * M + sol["X"] @ Gt @ sol["X"]) + (2.0 * M + sol["X"] @ Gt @ sol["X"]).T), True, -1.0)
    return D, gH, gS, sol


def density_unit(H, S, n_occ, eps, D):
    """U_D = m 2^-52 kappa_2(S) (eps_max - eps_min) / (eps_LUMO - eps_HOMO) max|D|, gap factor 1 when n_occ = m."""
    m = H.shape[0]
    kap = 1.0 if S is None else float(np.linalg.cond(S))
    gapf = 1.0 if n_occ >= m else (eps[-1] - eps[0]) / (eps[n_occ] - eps[n_occ - 1])
    return m * 2.0 ** -52 * kap * gapf * max(float(np.abs(D).max()), np.finfo(np.float64).tiny)
