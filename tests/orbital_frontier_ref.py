"""Float64 numpy restatement of the frontier levels without a solve (nabladft_amd/csrc/orbfrontier.hip, ``BatchedPurification.frontier``,
``purified_frontier``); test infrastructure shared by tests/test_orbital_frontier_cpu.py and tests/test_orbital_frontier_gpu.py.

Per molecule: Ht symmetric m x m (the orthogonalised Hamiltonian), X the projector on its n_occ lowest levels, e_min <= spec(Ht) <= e_max.  With P = X on
the HOMO side (side 0) and P = I - X on the LUMO side (side 1):

  operator   A y = P ((Ht - e_min I) (P y))  or  P ((e_max I - Ht) (P y)): the projector on both sides of every application
  start      v_0 = P r / |P r|,  r_i = 0.5 + ((2654435761 i + 12345) mod 2^32) / 2^32
  step j     w = A v_j; alpha_j = v_j . w; w -= alpha_j v_j + beta_{j-1} v_{j-1}; two passes of w -= V^T (V w) over all stored vectors; beta_j = |w|;
             (theta, s) the top eigenpair of the tridiagonal T_j (here: ``np.linalg.eigh`` of the dense T_j; the kernel bisects and uses a twisted
             factorisation); stop when beta_j |s_last| <= tol (e_max - e_min), or after min(m, k_max) steps (not converged)
  result     y = P (V^T s) normalised; the level = y^T Ht y with the unshifted Ht (not theta); c = W^T y (W = Z of the orthogonaliser, or S^(-1/2))
  gradients  d eps / dH = c c^T,  d eps / dS = -eps c c^T
"""
import numpy as np

import orbital_purify_ref as pref

HOMO, LUMO = 0, 1


def start_vector(m):
    i = np.arange(m, dtype=np.uint64)
    h = (np.uint64(2654435761) * i + np.uint64(12345)) % np.uint64(2 ** 32)
    return 0.5 + h.astype(np.float64) / 4294967296.0


def side(Ht, X, e_min, e_max, n_occ, which, k_max=256, tol=2.0 ** -44, W=None):
    """One side -> dict(eps, vec, coef, iters, res, conv, theta): conv 1 converged, 0 not converged (NaN outputs), -1 the level does not exist (NaN)."""
    Ht = np.asarray(Ht, dtype=np.float64)
    m = Ht.shape[0]
    nanv = np.full(m, np.nan)
    out = dict(eps=np.nan, vec=nanv, coef=nanv, iters=0, res=np.nan, conv=0, theta=np.nan)
    if (which == HOMO and n_occ < 1) or (which == LUMO and n_occ >= m):
        out["conv"] = -1
        return out
    if which == HOMO:
        proj = lambda y: X @ y
        a0 = lambda y: Ht @ y - e_min * y
    else:
        proj = lambda y: y - X @ y
        a0 = lambda y: e_max * y - Ht @ y
    w = proj(start_vector(m))
    nrm = np.sqrt(w @ w)
    if not (nrm > 0.0 and np.isfinite(nrm)):
        return out
    kk = min(m, k_max)
    V = np.zeros((kk, m))
    V[0] = w / nrm
    al, be = [], []
    beta_prev, done, s = 0.0, False, None
    for j in range(kk):
        v = V[j]
        w = proj(a0(proj(v)))
        alpha = float(v @ w)
        w = w - alpha * v
        if j > 0:
            w = w - beta_prev * V[j - 1]
        for _ in range(2):
            w = w - V[:j + 1].T @ (V[:j + 1] @ w)
        beta = float(np.sqrt(w @ w))
        al.append(alpha)
        be.append(beta)
        T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
        ev, es = np.linalg.eigh(T)
        s = es[:, -1]
        out["iters"], out["theta"] = j + 1, float(ev[-1])
        res = beta * abs(s[-1])
        if res <= tol * (e_max - e_min):
            done, out["res"] = True, res
            break
        if j + 1 == kk:
            break
        V[j + 1] = w / beta
        beta_prev = beta
    if not done:
        return out
    y = proj(V[:out["iters"]].T @ s)
    y = y / np.sqrt(y @ y)
    out["eps"] = float(y @ (Ht @ y))
    out["vec"] = y
    out["coef"] = y if W is None else W.T @ y
    out["conv"] = 1
    return out


def frontier(H, S, n_occ, k_max=256, tol=2.0 ** -44, max_iter=100):
    """The whole route from (H, S): the orthogonaliser, SP2, both sides -> (homo side, lumo side, purification)."""
    H = np.asarray(H, dtype=np.float64)
    Z = pref.orthogonalizer(S)
    Ht = pref.congruence(Z, pref.lower_sym(H), False)
    sol = pref.purify(Ht, n_occ, max_iter)
    sides = [side(Ht, sol["X"], sol["e_min"], sol["e_max"], n_occ, w, k_max, tol, Z) for w in (HOMO, LUMO)]
    return sides[0], sides[1], sol


def gradients(sides, g):
    """(gH, gS) = (sum g c c^T, -sum g eps c c^T) over the existing sides."""
    m = sides[0]["coef"].shape[0]
    gH, gS = np.zeros((m, m)), np.zeros((m, m))
    for sd, gg in zip(sides, g):
        if sd["conv"] == -1:
            continue
        cc = np.outer(sd["coef"], sd["coef"])
        gH += gg * cc
        gS -= gg * sd["eps"] * cc
    return gH, gS


def exact_projector(Ht, n_occ):
    ev, U = np.linalg.eigh(Ht)
    return U[:, :n_occ] @ U[:, :n_occ].T, ev, U


def level_unit(m, spread, kappa=1.0):
    """U_eps = m 2^-52 kappa_2(S) (eps_max - eps_min)."""
    return m * 2.0 ** -52 * kappa * spread


def separation(ev, k):
    """The distance from level k to its nearest neighbour (the whole spread for m = 1)."""
    d = [abs(ev[k] - ev[i]) for i in (k - 1, k + 1) if 0 <= i < len(ev)]
    return min(d) if d else 1.0


def random_hamiltonian(rng, m, n_occ, gap=0.3, spread=22.0):
    """A symmetric matrix with a `spread`-unit spectrum and `gap` between level n_occ - 1 and level n_occ (where both exist); not diagonal."""
    ev = np.sort(rng.uniform(0.0, 1.0, m))
    if 0 < n_occ < m:
        lo, hi = ev[:n_occ], ev[n_occ:]
        lo = lo - lo.max()
        hi = hi - hi.min() + gap / spread
        ev = np.concatenate([lo, hi])
    ev = ev - ev.min()
    if m > 1:
        ev = ev / max(ev.max(), 1e-300) * spread
        if 0 < n_occ < m:        # keep the gap at `gap` after the rescale
            ev[n_occ:] += gap - (ev[n_occ] - ev[n_occ - 1])
    ev = ev - 0.4 * (ev.max() - ev.min())
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    return pref.lower_sym((Q * ev) @ Q.T), ev
