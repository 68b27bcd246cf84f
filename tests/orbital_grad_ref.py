"""Float64 yardstick of the orbital-energy gradients (nabladft_amd/orbital_loss.py, csrc/orbdens.hip); test infrastructure shared by
tests/test_orbital_loss_cpu.py and tests/test_orbital_loss_gpu.py.

Two independent routes to ``dL/dH`` and ``dL/dS`` of a loss on the eigenvalues of ``H C = S C diag(eps)``, both in the convention of a symmetric input
(the symmetric matrix, what ``torch.linalg.eigh`` returns):

  (a) ``autograd``     torch.linalg ``cholesky`` / ``solve_triangular`` / ``eigvalsh`` with autograd through the whole Cholesky -> reduce -> eigenvalue route;
  (b) ``closed_form``  ``sum_k g_k c_k c_k^T`` and ``-sum_k g_k eps_k c_k c_k^T`` from ``orbitals_ref.solve`` (numpy) on a row/column-PERMUTED copy of the
                       problem, permuted back: another elimination order, another eigenvector basis, no autograd.

``units`` are what a figure is measured in: ``U_H = m 2^-52 |S^-1|_2 max|g|`` and ``U_S = U_H |H|_2 |S^-1|_2``.
"""
import numpy as np
import torch

import orbitals_ref as R

SIZES = [1, 3, 17, 65, 130]
LOSSES = ("tanh", "mae")


def cases():
    """The generalized problems of the end-to-end check: ``orbitals_ref.case(m, 1e2, 7 + m)`` -> [(H, S)]."""
    return [R.case(m, 1e2, 7 + m) for m in SIZES]


def mae_target(m):
    return np.sort(np.random.Generator(np.random.PCG64(500 + m)).uniform(-20.0, 2.0, size=m))


def loss_of(kind, eps, m=None):
    """A loss of one molecule's eigenvalues (a torch tensor) -> scalar tensor.  "tanh": sum tanh(0.1 eps), smooth and insensitive to gaps; "mae": the mean
    absolute error against sort(U(-20, 2))."""
    if kind == "tanh":
        return torch.tanh(0.1 * eps).sum()
    m = eps.shape[0] if m is None else m
    return (eps - torch.from_numpy(mae_target(m)).to(eps.device)).abs().mean()


def dloss(kind, eps):
    """g = dL/d eps of one molecule (numpy [m]) by autograd on the eigenvalues alone."""
    e = torch.tensor(np.asarray(eps, dtype=np.float64), requires_grad=True)
    loss_of(kind, e).backward()
    return e.grad.numpy()


def autograd(H, S, kind):
    """Route (a) -> (eps, gH, gS), numpy float64; ``S = None``: the standard problem (gS None)."""
    Ht = torch.tensor(np.asarray(H, dtype=np.float64), requires_grad=True)
    if S is None:
        A = Ht
        St = None
    else:
        St = torch.tensor(np.asarray(S, dtype=np.float64), requires_grad=True)
        L = torch.linalg.cholesky(St)
        X = torch.linalg.solve_triangular(L, Ht, upper=False)
        A = torch.linalg.solve_triangular(L, X.mT, upper=False).mT
    eps = torch.linalg.eigvalsh(0.5 * (A + A.mT))
    loss_of(kind, eps).backward()
    sym = lambda g: 0.5 * (g + g.T)
    return eps.detach().numpy(), sym(Ht.grad.numpy()), None if St is None else sym(St.grad.numpy())


def closed_form(H, S, kind, seed=0):
    """Route (b) -> (eps, gH, gS) from the numpy solution of the permuted problem."""
    m = H.shape[0]
    perm = np.random.Generator(np.random.PCG64(900 + seed + m)).permutation(m)
    ix = np.ix_(perm, perm)
    eps, C = R.solve(H[ix], None if S is None else S[ix])
    g = dloss(kind, eps)
    gHp = (C * g[None, :]) @ C.T
    gSp = -(C * (g * eps)[None, :]) @ C.T
    gH, gS = np.empty_like(gHp), np.empty_like(gSp)
    gH[ix], gS[ix] = gHp, gSp
    return eps, gH, (None if S is None else gS)


def units(H, S, g):
    """(U_H, U_S) of one molecule."""
    m = H.shape[0]
    nH = np.linalg.norm(H, 2)
    nSi = 1.0 if S is None else 1.0 / np.linalg.eigvalsh(S)[0]
    uH = m * R.EPS * nSi * max(np.abs(g).max(), np.finfo(np.float64).tiny)
    return uH, uH * max(nH, np.finfo(np.float64).tiny) * nSi


def spread(H, S, kind):
    """Route (a) against route (b) -> (figure on gH, figure on gS) in units, plus route (a)'s results for reuse: (fH, fS, eps, gH, gS)."""
    eps, gH, gS = autograd(H, S, kind)
    _, bH, bS = closed_form(H, S, kind)
    uH, uS = units(H, S, dloss(kind, eps))
    fS = 0.0 if S is None else float(np.abs(gS - bS).max() / uS)
    return float(np.abs(gH - bH).max() / uH), fS, eps, gH, gS
