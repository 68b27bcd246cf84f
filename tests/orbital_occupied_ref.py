"""Float64 numpy restatement of the occupied levels without a full solve (nabladft_amd/csrc/orbocc.hip, ``BatchedPurification.occupied``,
``purified_occupied_energies``); test infrastructure shared by tests/test_orbital_occupied_cpu.py and tests/test_orbital_occupied_gpu.py.

Per molecule: Ht symmetric m x m (the orthogonalised Hamiltonian), X the projector on its n_occ lowest levels.

  factor   left-looking pivoted Cholesky of X for exactly n_occ steps: p = the largest remaining diagonal entry (the first on ties),
           q_j = (X[p, :] - sum_{k<j} q_k[p] q_k) / sqrt(pivot) with the entries of earlier pivots exactly 0, diag -= q_j^2.  A pivot < 1/(2m) or not finite,
           or a left-over diagonal entry >= 1/(2m) in magnitude after the last step (the rank exceeds n_occ): status 5, NaN.  An exact projector of rank r gives X = Q^T Q with Q Q^T = I and every pivot >= (remaining rank) / m.
  reduce   Hs = Q Ht Q^T, n_occ x n_occ, the lower triangle mirrored (n_occ = 0: the 1 x 1 block [0])
  solve    Hs V = V diag(eps)  (``np.linalg.eigh``; the kernels run the batched solver on the reduced blocks)
  back     C = V^T Q W (rows = orbitals; W = Z of the orthogonaliser, S^(-1/2), or nothing), the largest-magnitude component of every row positive, the first on
           ties; NaN in every slot k >= n_occ
  gradients  d eps_k / dH = c_k c_k^T,  d eps_k / dS = -eps_k c_k c_k^T
"""
import numpy as np

import orbital_purify_ref as pref

STATUS_NOT_A_PROJECTOR = 5


def factor(X, n_occ):
    """-> dict(Q [n_occ, m], pivots [n_occ], min_pivot, defect, status, diag): status 5 and NaN where a pivot is < 1/(2m) or not finite."""
    X = np.asarray(X, dtype=np.float64)
    m = X.shape[0]
    d = np.diag(X).copy()
    done = np.zeros(m, dtype=bool)
    Q = np.zeros((n_occ, m))
    piv = np.full(n_occ, -1, dtype=np.int64)
    pmin = np.inf
    for j in range(n_occ):
        cand = np.where(done, -np.inf, np.where(np.isnan(d), -np.inf, d))
        p = int(np.argmax(cand))                      # the first on ties
        pv = cand[p]
        if not (pv >= 0.5 / m) or not (pv < np.inf):
            return dict(Q=np.full((n_occ, m), np.nan), pivots=np.full(n_occ, -1, dtype=np.int64), min_pivot=np.nan, defect=np.nan,
                        status=STATUS_NOT_A_PROJECTOR, diag=d)
        x = (X[p] - Q[:j, p] @ Q[:j]) / np.sqrt(pv)    # the kernel subtracts in the order of k with fma(): the same number to rounding
        x[done] = 0.0
        Q[j] = x
        d = np.where(done, d, d - x * x)
        done[p] = True
        piv[j] = p
        pmin = min(pmin, float(pv))
    left = float(np.abs(d).max()) if not np.isnan(d).any() else np.nan
    if not (left < 0.5 / m):                          # a step more would find a pivot: the rank exceeds n_occ
        return dict(Q=np.full((n_occ, m), np.nan), pivots=np.full(n_occ, -1, dtype=np.int64), min_pivot=np.nan, defect=np.nan,
                    status=STATUS_NOT_A_PROJECTOR, diag=d)
    return dict(Q=Q, pivots=piv, min_pivot=pmin, defect=left, status=0, diag=d)


def reduce(Q, Ht):
    n = Q.shape[0]
    if n == 0:
        return np.zeros((1, 1))
    return pref.lower_sym(Q @ pref.lower_sym(Ht) @ Q.T)


def sign_rows(C):
    """The solver's sign rule on rows: the largest-magnitude component positive, the first on ties."""
    C = C.copy()
    for k in range(C.shape[0]):
        at = int(np.argmax(np.abs(C[k])))
        if C[k, at] < 0.0:
            C[k] = -C[k]
    return C


def back(V, Q, W=None):
    """V: columns = the vectors of the reduced problem -> C [n_occ, m], rows = orbitals."""
    U = V.T @ Q
    return sign_rows(U if W is None else U @ W)


def occupied(Ht, X, n_occ, W=None):
    """Factor, reduce, solve, back -> dict(eps [m] and C [m, m] with NaN in the slots k >= n_occ, factor, Hs, status)."""
    m = Ht.shape[0]
    f = factor(X, n_occ)
    eps, C = np.full(m, np.nan), np.full((m, m), np.nan)
    out = dict(eps=eps, C=C, factor=f, Hs=None, status=f["status"])
    if f["status"] != 0 or n_occ == 0:
        return out
    Hs = reduce(f["Q"], Ht)
    ev, V = np.linalg.eigh(Hs)
    eps[:n_occ] = ev
    C[:n_occ] = back(V, f["Q"], W)
    out["Hs"] = Hs
    return out


def from_matrices(H, S, n_occ, max_iter=100):
    """The whole route from (H, S): the orthogonaliser, SP2, occupied -> (result, purification)."""
    H = np.asarray(H, dtype=np.float64)
    Z = pref.orthogonalizer(S)
    Ht = pref.congruence(Z, pref.lower_sym(H), False)
    sol = pref.purify(Ht, n_occ, max_iter)
    if sol["status"] != 0:
        m = H.shape[0]
        return dict(eps=np.full(m, np.nan), C=np.full((m, m), np.nan), factor=None, Hs=None, status=sol["status"]), sol
    return occupied(Ht, sol["X"], n_occ, Z), sol


def gradients(res, g, n_occ):
    """(gH, gS) = (sum_k g_k c_k c_k^T, -sum_k g_k eps_k c_k c_k^T) over k < n_occ."""
    m = res["C"].shape[0]
    gH, gS = np.zeros((m, m)), np.zeros((m, m))
    for k in range(n_occ):
        cc = np.outer(res["C"][k], res["C"][k])
        gH += g[k] * cc
        gS -= g[k] * res["eps"][k] * cc
    return gH, gS


def q_unit(m):
    """u_Q = m^(3/2) 2^-52."""
    return m ** 1.5 * 2.0 ** -52


def csc_unit(m, kappa=1.0):
    """The unit of ``C S C^T - I``: ``(u_Q + 2 m 2^-52) kappa_2(S)``.  ``u_Q kappa`` is what the factor's own defect ``Q Q^T - I`` becomes under the congruence
    with ``W``; ``2 m 2^-52 kappa`` is the rounding of the check itself, two products with m-term sums (``C S``, then ``(C S) C^T``).  ``u_Q kappa`` alone is under
    two ulps at m <= 2, below what evaluating the check costs (the restatement then measures 1.06 of it at m = 2)."""
    return (q_unit(m) + 2.0 * m * 2.0 ** -52) * kappa


def level_unit(m, spread, kappa=1.0):
    """U_eps = m 2^-52 kappa_2(S) (eps_max - eps_min)."""
    return m * 2.0 ** -52 * kappa * spread
