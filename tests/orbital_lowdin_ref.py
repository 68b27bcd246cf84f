"""Float64 numpy restatement of the Löwdin analysis (nabladft_amd/csrc/orblowdin.hip, ``BatchedOrbitals.overlap_functions`` / ``sym_congruence`` /
``matfun_response``, ``nabladft_amd.orbital_loss.lowdin_*``) and its torch yardstick; test infrastructure shared by tests/test_orbital_lowdin_cpu.py and
tests/test_orbital_lowdin_gpu.py.

With ``S = U diag(s) U^T``, ``a = sqrt(s)``, ``A = S^(1/2) = U diag(a) U^T``, ``A^- = S^(-1/2) = U diag(1 / a) U^T``:

    congruence   Y = M X,  M^L = sym(X Y)                                   (X = A or A^-, M = D or H, both symmetric)
    reverse      dL/dM = sym(X (G X)),  dL/dX = Y G + G Y^T = 2 sym(Y G)    (G = dL/dM^L symmetric)
    functions    dL/dS = U [K o (U^T sym(g) U)] U^T,  K_ij = 1 / (a_i + a_j) (kind 0: A),  -1 / (a_i a_j (a_i + a_j)) (kind 1: A^-), the diagonal included
    Löwdin       D^L = A D A,  q_A = sum_{mu in A} D^L_mu,mu,  W_AB = sum_{mu in A, nu in B} (D^L_mu,nu)^2,  V_A = sum_{B != A} W_AB

No difference of levels is divided.  ``ptr`` [n + 1]: the first orbital of every atom of ONE molecule (the convention of tests/orbital_bond_ref.py).

Bounds, U = 2^-53: the dot-product bound of the sibling suites, (K + 4) U sum |terms|.  ``product_bound`` K = m; ``symprod_bound`` K = 2 m for the two contractions
that share an accumulator (the halving and alpha = 1, 2 are exact); ``mo_bound``: the bound of W times |K|, plus ``K_ROUNDINGS[kind] + 1`` half-ulp roundings of |K W|:
K of kind 0 is one sum and one division (2 roundings), of kind 1 a product, a sum, a product and a division (4), and K W is one more product; the square roots
themselves are compared exactly (``np.sqrt`` is correctly rounded, as the device's is).
"""
import numpy as np
import torch

import orbital_bond_ref as BR

U = BR.U
K_ROUNDINGS = (2, 4)
sym = lambda X: 0.5 * (X + X.T)
lower_sym = BR.lower_sym


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------------------
def decompose(S):
    """-> (s ascending, U with the eigenvectors as columns) of the symmetric S."""
    return np.linalg.eigh(sym(np.asarray(S, dtype=np.float64)))


def weights(s):
    """-> (a, 1 / a, cond, info): NaN and info 1 unless every level is finite and positive."""
    s = np.asarray(s, dtype=np.float64)
    if not (np.all(np.isfinite(s)) and np.all(s > 0.0)):
        return np.full_like(s, np.nan), np.full_like(s, np.nan), np.nan, 1
    a = np.sqrt(s)
    return a, 1.0 / a, float(s.max() / s.min()), 0


def functions(S):
    """-> (A, A^-, s, U)"""
    s, Uv = decompose(S)
    a, ia, _, _ = weights(s)
    return sym((Uv * a[None, :]) @ Uv.T), sym((Uv * ia[None, :]) @ Uv.T), s, Uv


def product(M, X):
    """Y = M X from the LOWER triangles of both, as the kernel reads them."""
    return lower_sym(M) @ lower_sym(X)


def symprod(E, X, side, alpha=1.0):
    """alpha sym(X E) (side 0) or alpha sym(E X) (side 1); X from its lower triangle.  The lower triangle is computed and mirrored: exactly symmetric."""
    Xs = lower_sym(X)
    Z = alpha * (0.5 * (Xs @ E + E.T @ Xs if side == 0 else E @ Xs + Xs @ E.T))
    return np.tril(Z) + np.tril(Z, -1).T


def congruence(X, M):
    """-> (M^L, Y)"""
    Y = product(M, X)
    return symprod(Y, X, 0), Y


def congruence_backward(G, X, Y):
    """-> (dL/dM, dL/dX) for a symmetric G"""
    return symprod(product(G, X), X, 0), symprod(Y, G, 1, 2.0)


def kernel_K(a, kind):
    """K in the kernel's order of operations."""
    ai, aj = a[:, None], a[None, :]
    return 1.0 / (ai + aj) if kind == 0 else -1.0 / ((ai * aj) * (ai + aj))


def matfun_response(g, s, Uv, kind):
    """dL/dS for dL/dX = g, X = S^(1/2) (kind 0) or S^(-1/2) (kind 1)."""
    W = Uv.T @ sym(g) @ Uv
    return sym(Uv @ (kernel_K(np.sqrt(s), kind) * W) @ Uv.T)


def populations(DL, ptr):
    d = np.diag(DL)
    return np.array([d[ptr[A]:ptr[A + 1]].sum() for A in range(len(ptr) - 1)])


def lowdin(D, S, ptr):
    """-> (D^L, q [n], W [n, n], V [n])"""
    A = functions(S)[0]
    DL = congruence(A, D)[0]
    W = BR.bond_orders(DL, ptr)
    return DL, populations(DL, ptr), W, BR.valence(W)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------------------------------------
def product_bound(M, X):
    return (M.shape[0] + 4) * U * (np.abs(lower_sym(M)) @ np.abs(lower_sym(X)))


def symprod_bound(E, X, side, alpha=1.0):
    m = E.shape[0]
    Ea, Xa = np.abs(E), np.abs(lower_sym(X))
    mag = (Xa @ Ea + Ea.T @ Xa) if side == 0 else (Ea @ Xa + Xa @ Ea.T)
    return (2 * m + 4) * U * 0.5 * abs(alpha) * mag


def mo_bound(Ct, T, a, kind):
    """Ct: the state's coefficient block (row k = u_k); |K o (Ct T) - device|."""
    m = T.shape[0]
    K = np.abs(kernel_K(a, kind))
    return K * ((m + 4) * U * (np.abs(Ct) @ np.abs(T))) + (K_ROUNDINGS[kind] + 1) * U * K * np.abs(Ct @ T)


# ---- the torch yardstick: eigh -> U f(s) U^T -> congruence -> populations / Wiberg table, autograd through all of it --------------------------------------------------
def torch_functions(St):
    s, Uv = torch.linalg.eigh(0.5 * (St + St.mT))
    a = torch.sqrt(s)
    return (Uv * a) @ Uv.mT, (Uv / a) @ Uv.mT


def indicator(ptr, m):
    A = np.zeros((len(ptr) - 1, m))
    for k in range(len(ptr) - 1):
        A[k, ptr[k]:ptr[k + 1]] = 1.0
    return A


def torch_lowdin(D, S, H, ptr):
    """Dense torch tensors -> (q, W, V, H^L) with autograd."""
    m = S.shape[0]
    At = torch.from_numpy(indicator(ptr, m))
    A, Ai = torch_functions(S)
    DL = A @ D @ A
    DL = 0.5 * (DL + DL.mT)
    q = At @ torch.diagonal(DL)
    W = At @ (DL * DL) @ At.mT
    V = W.sum(1) - torch.diagonal(W)
    HL = Ai @ H @ Ai
    return q, W, V, 0.5 * (HL + HL.mT)


def min_relative_gap(s):
    """The smallest gap between neighbouring levels over the largest level: what the backward of ``eigh`` divides by."""
    s = np.sort(np.asarray(s, dtype=np.float64))
    return float(np.diff(s).min() / s.max()) if s.shape[0] > 1 else float("inf")
