"""Float64 numpy restatement of the SCF-residual kernels (nabladft_amd/csrc/orbcomm.hip, ``BatchedOrbitals.commutator`` / ``antisymmetrize`` /
``commutator_norms``, ``nabladft_amd.orbital_loss.commutator`` / ``scf_residual``) and its torch yardstick; test infrastructure shared by
tests/test_orbital_commutator_cpu.py and tests/test_orbital_commutator_gpu.py.

    product      C = alpha (X Y - Y X);  Y from its lower triangle;  x_anti 0: X from its lower triangle, C antisymmetric, diagonal +0.0;
                 x_anti 1: X from its STRICT lower triangle, the mirrored element negated, diagonal 0, C symmetric
    reverse      G_a = (G - G^T) / 2,  dL/dX = [G_a, Y],  dL/dY = [X, G_a] = -[G_a, X]
    residual     R^L = [A^- H A^-, A D A],  A = S^(1/2), A^- = S^(-1/2) (tests/orbital_lowdin_ref.py)
    identity     D^L = 2 Q, Q = sum_{i occ} q_i q_i^T a projector:  sum_ij (R^L_ij)^2 = 8 sum_{i occ, a virt} (q_i^T H^L q_a)^2

Bounds, U = 2^-53: an entry of the product is a sum of 2 m terms that share an accumulator, so the dot-product bound of the sibling suites is
(2 m + 4) U |alpha| (|X| |Y| + |Y| |X|) (``product_bound``; alpha = +-1, 2 is exact).  ``norms_bound``: m^2 U sum R^2 for the sum of squares against numpy's
pairwise sum; the maximum is exact.
"""
import numpy as np
import torch

import orbital_lowdin_ref as LR

U = LR.U
sym = LR.sym
lower_sym = LR.lower_sym


def lower_anti(X):
    """The antisymmetric matrix whose strict lower triangle is X's; the diagonal and the upper triangle of X are ignored."""
    L = np.tril(np.asarray(X, dtype=np.float64), -1)
    return L - L.T


def operand(X, x_anti):
    return lower_anti(X) if x_anti else lower_sym(X)


def product(X, Y, x_anti=0, alpha=1.0):
    """alpha (X Y - Y X) as the kernel forms it: the lower triangle is computed and mirrored with the sign of the result's symmetry; +0.0 diagonal for x_anti 0."""
    Xs, Ys = operand(X, x_anti), lower_sym(Y)
    C = alpha * (Xs @ Ys - Ys @ Xs)
    low = np.tril(C, -1)
    if x_anti:
        return low + low.T + np.diag(np.diag(C))
    return low - low.T


def antisymmetrize(G):
    G = np.asarray(G, dtype=np.float64)
    out = 0.5 * (G - G.T)
    np.fill_diagonal(out, 0.0)
    return out


def norms(R):
    """-> (sum R_ij^2, max |R_ij|)"""
    R = np.asarray(R, dtype=np.float64)
    return float((R * R).sum()), float(np.abs(R).max())


def commutator_backward(G, X, Y):
    """-> (dL/dX, dL/dY) of C = X Y - Y X for symmetric X, Y and any upstream G, both symmetric."""
    Ga = antisymmetrize(G)
    return product(Ga, Y, 1, 1.0), product(Ga, X, 1, -1.0)


def scf_residual(H, D, S):
    """-> (R^L, H^L, D^L)"""
    A, Ai = LR.functions(S)[:2]
    HL, DL = LR.congruence(Ai, H)[0], LR.congruence(A, D)[0]
    return product(HL, DL), HL, DL


def ov_identity(HL, Q_occ, Q_virt):
    """8 sum_ia h_ia^2 for orthonormal columns Q_occ, Q_virt spanning the occupied space of D^L = 2 Q_occ Q_occ^T and its complement."""
    h = Q_occ.T @ HL @ Q_virt
    return 8.0 * float((h * h).sum())


def errors(residuals):
    """What ``ScfResidualErrors`` reports for a list of residual blocks (a non-finite block is counted and left out)."""
    rms, top, failed = [], [], 0
    for R in residuals:
        if not np.all(np.isfinite(R)):
            failed += 1
            continue
        s, t = norms(R)
        rms.append(np.sqrt(s) / R.shape[0])
        top.append(t)
    return {"scf_residual_rms": float(np.mean(rms)), "scf_residual_max": float(np.mean(top)), "molecules": len(rms), "failed": failed}


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------------------------------------
def product_bound(X, Y, x_anti=0, alpha=1.0):
    m = np.asarray(Y).shape[0]
    Xa, Ya = np.abs(operand(X, x_anti)), np.abs(lower_sym(Y))
    return (2 * m + 4) * U * abs(alpha) * (Xa @ Ya + Ya @ Xa)


def norms_bound(R):
    R = np.asarray(R, dtype=np.float64)
    return R.shape[0] ** 2 * U * float((R * R).sum())


# ---- the torch yardstick: the dense expression on symmetrised leaves, autograd through all of it -------------------------------------------------------------------------
def torch_commutator(Xt, Yt):
    Xs, Ys = 0.5 * (Xt + Xt.mT), 0.5 * (Yt + Yt.mT)
    return Xs @ Ys - Ys @ Xs


def torch_scf_residual(Ht, Dt, St):
    """Dense float64 tensors -> R^L through ``torch.linalg.eigh`` of S, with autograd to all three."""
    A, Ai = LR.torch_functions(St)
    Hs, Ds = 0.5 * (Ht + Ht.mT), 0.5 * (Dt + Dt.mT)
    HL, DL = Ai @ Hs @ Ai, A @ Ds @ A
    return torch_commutator(HL, DL)
