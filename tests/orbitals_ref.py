"""Float64 numpy yardstick of the batched orbital solver (nabladft_amd/orbitals.py, csrc/orbitals.hip); test infrastructure shared by
tests/test_orbitals_cpu.py, tests/test_orbitals_gpu.py and scripts/bench_orbitals.py.

``solve`` is the textbook route: ``np.linalg.cholesky``, two triangular solves written with numpy, symmetrise, ``np.linalg.eigh``, back-substitute.
``case`` generates conditioned generalized problems; ``errors`` measures a solution in units of u = m 2^-52.  The standard problem (S = None) is measured
with ``vib_ref.eig_errors``.  ``occupied_counts`` / ``frontier`` / ``compare`` restate the small kernels and the host helper.
"""
import numpy as np

from vib_ref import eig_errors  # noqa: F401  (the standard problem's figures, verbatim)

EPS = 2.0 ** -52
SIZES = [1, 2, 3, 5, 24, 63, 64, 65, 141, 255, 256, 257, 412]
KAPPAS = [1.0, 1e2, 1e4]
FIGURES = ("eps_mae_occ", "eps_mae_all", "psi_sim_occ", "homo_abs_err", "lumo_abs_err", "gap_abs_err", "psi_sim_min_occ")


def lower_solve(L, B):
    """X with L X = B, L lower triangular: forward substitution row by row."""
    X = np.array(B, dtype=np.float64)
    for k in range(L.shape[0]):
        X[k] = (X[k] - L[k, :k] @ X[:k]) / L[k, k]
    return X


def upper_solve(U, B):
    """X with U X = B, U upper triangular: back substitution."""
    X = np.array(B, dtype=np.float64)
    for k in range(U.shape[0] - 1, -1, -1):
        X[k] = (X[k] - U[k, k + 1:] @ X[k + 1:]) / U[k, k]
    return X


def solve(H, S=None):
    """-> (eps ascending [m], C [m, m] with the orbitals as columns, C^T S C = I)."""
    H = np.asarray(H, dtype=np.float64)
    if S is None:
        return np.linalg.eigh(0.5 * (H + H.T))
    L = np.linalg.cholesky(np.asarray(S, dtype=np.float64))
    X = lower_solve(L, H)                    # L^-1 H
    A = lower_solve(L, X.T).T                # (L^-1 H) L^-T
    w, Y = np.linalg.eigh(0.5 * (A + A.T))
    return w, upper_solve(L.T, Y)


def case(m, kappa0, seed):
    """A conditioned generalized problem -> (H, S), both exactly symmetric float64: S0 = Q diag(logspace(0, -log10 kappa0, m)) Q^T scaled to unit diagonal,
    F = diag(sort(U(-20, 2))) + 0.3 (M + M^T), H = (S F + F S) / 2."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    S0 = (Q * np.logspace(0.0, -np.log10(kappa0), m)[None, :]) @ Q.T
    s = 1.0 / np.sqrt(np.diag(S0))
    S = S0 * s[:, None] * s[None, :]
    S = 0.5 * (S + S.T)
    M = rng.normal(size=(m, m))
    F = np.diag(np.sort(rng.uniform(-20.0, 2.0, size=m))) + 0.3 * (M + M.T)
    H = 0.5 * (S @ F + F @ S)
    return 0.5 * (H + H.T), S


def spectral(H, S):
    """(|H|_2, |S^-1|_2, kappa_2(S))."""
    sv = np.linalg.eigvalsh(S)
    return np.linalg.norm(H, 2), 1.0 / sv[0], sv[-1] / sv[0]


def errors(H, S, eps, C, ref=None):
    """(e_val, e_res, e_orth) in units of u = m 2^-52; C holds the orbitals as columns; ``ref``: eigenvalues to compare with (default: ``solve``'s)."""
    m = H.shape[0]
    u = m * EPS
    nH, nSi, kap = spectral(H, S)
    nH = max(nH, np.finfo(np.float64).tiny)
    ref = solve(H, S)[0] if ref is None else ref
    e_val = np.abs(eps - ref).max() / (u * nH * nSi)
    e_res = np.abs(H @ C - (S @ C) * eps[None, :]).max() / (u * nH * np.linalg.norm(C, 2))
    e_orth = np.abs(C.T @ S @ C - np.eye(m)).max() / (u * kap)
    return e_val, e_res, e_orth


def clustered(m, seed):
    """A symmetric matrix whose eigenvalues come in groups of four equal ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    w = np.repeat(rng.normal(size=(m + 3) // 4), 4)[:m]
    A = (Q * w[None, :]) @ Q.T
    return 0.5 * (A + A.T)


def standard(kind, m, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "zero":
        return np.zeros((m, m))
    if kind == "diagonal":
        return np.diag(rng.normal(size=m))
    if kind == "clustered":
        return clustered(m, seed)
    M = rng.normal(size=(m, m))
    return 0.5 * (M + M.T)


def sign_fixed(C):
    """Columns flipped so that the largest-magnitude component of each (the first on ties) is positive."""
    C = np.array(C, dtype=np.float64)
    at = np.argmax(np.abs(C), axis=0)
    flip = C[at, np.arange(C.shape[1])] < 0.0
    C[:, flip] = -C[:, flip]
    return C


def occupied_counts(z, ptr, charge=0):
    z, ptr = np.asarray(z, dtype=np.int64), np.asarray(ptr, dtype=np.int64)
    ne = np.array([z[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])], dtype=np.int64) - np.asarray(charge, dtype=np.int64)
    if np.any(ne % 2 != 0) or np.any(ne < 2):
        raise ValueError("odd or empty electron count")
    return (ne // 2).astype(np.int32)


def frontier(eps, n_occ):
    """-> (homo, lumo, gap); lumo and gap are NaN when every orbital is occupied."""
    homo = eps[n_occ - 1]
    lumo = eps[n_occ] if n_occ < len(eps) else np.nan
    return homo, lumo, lumo - homo


def compare(eps, C, eps_t, C_t, S, n_occ):
    """The seven figures of one molecule (FIGURES), predicted (eps, C) against target (eps_t, C_t); orbitals as columns; S = None: the identity."""
    m = len(eps)
    S = np.eye(m) if S is None else S
    df = np.abs(eps - eps_t)
    ov = np.abs(np.einsum("ik,ik->k", C[:, :n_occ], S @ C_t[:, :n_occ]))
    h, l, g = frontier(eps, n_occ)
    ht, lt, gt = frontier(eps_t, n_occ)
    return np.array([df[:n_occ].mean(), df.mean(), ov.mean(), abs(h - ht), abs(l - lt), abs(g - gt), ov.min()])
