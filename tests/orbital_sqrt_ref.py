"""Float64 numpy restatement of the eigensolver-free square roots of csrc/orbsqrt.hip: the coupled Newton-Schulz iteration, init / step / finish as the
kernels split it, with their stopping rule.  The summation orders are numpy's, not the kernels'.

    c = max_i sum_j |S_ij|;  Y_0 = S / c, Z_0 = I
    T_k = (3 I - sym(Z_k Y_k)) / 2  (sym: the lower triangle of the product mirrored),  delta_k = m - tr(Z_k Y_k)
    stop at k when delta_k == 0, or k >= 1 and |delta_k| < 1e-9 m and |delta_k| >= |delta_k-1|;  else Y_k+1 = Y_k T_k, Z_k+1 = T_k Z_k (general matrices)
    half = sqrt(c) mirror(Y), inv_half = mirror(Z) / sqrt(c)

Status 0: stopped; 1: c not finite or <= 0; 4: not stopped after max_iter iterations (an indefinite S, a NaN): NaN outputs.

Also here: the matrices every test of the feature uses (``CASES`` and ``spd``), the unit ``u = m 2^-52 kappa_2(S) max|entry|`` the accuracy is measured in, the
yardstick (``eigh_roots``), and the variant that symmetrises Y and Z between iterations, kept to document why the kernels do not."""
import os

import numpy as np

PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "orbital_sqrt_parity.txt")
TOL = 1e-9
EPS = 2.0 ** -52


def mirror(A):
    """The lower triangle of ``A`` on both sides of the diagonal."""
    L = np.tril(A)
    return L + np.tril(A, -1).T


def init(S):
    S = mirror(np.asarray(S, dtype=np.float64))
    c = np.abs(S).sum(axis=1).max() if not np.isnan(S).any() else np.nan
    if not (np.isfinite(c) and c > 0.0):
        return None
    m = S.shape[0]
    return dict(c=float(c), Y=S / c, Z=np.eye(m), k=0, deltas=[], log=[], m=m)


def t_matrix(Y, Z):
    """-> (T, tr(Z Y)) of one iteration: what the first launch leaves."""
    ZY = mirror(Z @ Y)
    return 0.5 * (3.0 * np.eye(Y.shape[0]) - ZY), float(np.trace(ZY))


def step(st, symmetrize=None):
    """Iteration ``st["k"]`` in place -> True if it stopped.  ``symmetrize``: None (the kernels), "mirror" or "average" (the two variants that diverge)."""
    m, k = st["m"], st["k"]
    with np.errstate(all="ignore"):
        T, tr = t_matrix(st["Y"], st["Z"])
        delta = m - tr
        st["deltas"].append(delta)
        prev = st["deltas"][k - 1] if k >= 1 else 0.0
        stop = delta == 0.0 or (k >= 1 and abs(delta) < TOL * m and abs(delta) >= abs(prev))
        st["log"].append(3 if stop else 1)
        if stop:
            return True
        Y, Z = st["Y"] @ T, T @ st["Z"]
        if symmetrize == "mirror":
            Y, Z = mirror(Y), mirror(Z)
        elif symmetrize == "average":
            Y, Z = 0.5 * (Y + Y.T), 0.5 * (Z + Z.T)
    st["Y"], st["Z"], st["k"] = Y, Z, k + 1
    return False


def finish(st, stopped):
    m = st["m"]
    if not stopped:
        return np.full((m, m), np.nan), np.full((m, m), np.nan)
    r = np.sqrt(st["c"])
    return r * mirror(st["Y"]), mirror(st["Z"]) / r


def roots(S, max_iter=100, symmetrize=None):
    """-> (half, inv_half, sol): sol = dict(status, iters, deltas, c)."""
    S = np.asarray(S, dtype=np.float64)
    m = S.shape[0]
    st = init(S)
    if st is None:
        return np.full((m, m), np.nan), np.full((m, m), np.nan), dict(status=1, iters=0, deltas=[], c=np.nan)
    stopped = False
    for _ in range(max_iter):
        if step(st, symmetrize):
            stopped = True
            break
    half, inv = finish(st, stopped)
    return half, inv, dict(status=0 if stopped else 4, iters=st["k"], deltas=st["deltas"], c=st["c"])


def eigh_roots(S):
    """The yardstick: ``S^(1/2)`` and ``S^(-1/2)`` from ``np.linalg.eigh``."""
    s, U = np.linalg.eigh(mirror(np.asarray(S, dtype=np.float64)))
    a = np.sqrt(s)
    return (U * a[None, :]) @ U.T, (U / a[None, :]) @ U.T


def unit(S, X):
    """``u = m 2^-52 kappa_2(S) max|X_ij|``: the size of the rounding error any route to a function ``X`` of ``S`` may leave."""
    S = mirror(np.asarray(S, dtype=np.float64))
    return S.shape[0] * EPS * np.linalg.cond(S) * np.abs(X).max()


def spd(m, kappa, seed):
    """A random symmetric positive definite matrix with levels log-spaced in [1 / kappa, 1] times 1.7 (exactly symmetric)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    lev = 1.7 * np.logspace(-np.log10(kappa), 0.0, m) if m > 1 else np.array([1.7])
    A = (Q * lev[None, :]) @ Q.T
    return mirror(0.5 * (A + A.T))


# (name, m, kappa, seed): the ragged sizes around the 16-wide instruction tile and the 64-wide workgroup tile, kappa from 10 to 1e4
RAGGED = [("m1", 1, 1.0, 11), ("m2", 2, 1e1, 12), ("m3", 3, 1e2, 13), ("m15", 15, 1e3, 14), ("m16", 16, 1e4, 15), ("m17", 17, 1e1, 16), ("m63", 63, 1e2, 17),
          ("m64", 64, 1e3, 18), ("m65", 65, 1e4, 19), ("m127", 127, 1e2, 20), ("m128", 128, 1e3, 21), ("m130", 130, 1e4, 22)]
HARD = [("kappa1e6", 40, 1e6, 31), ("kappa1e8", 40, 1e8, 32)]


def identity_case(m=9):
    return np.eye(m)


def diagonal_case(m=12):
    return np.diag(np.linspace(0.05, 2.5, m))


def cases():
    """-> list of (name, S): every matrix that must converge."""
    out = [(name, spd(m, kappa, seed)) for name, m, kappa, seed in RAGGED + HARD]
    out.append(("identity", identity_case()))
    out.append(("diagonal", diagonal_case()))
    return out


def indefinite_case(m=20, seed=41):
    rng = np.random.Generator(np.random.PCG64(seed))
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    lev = np.linspace(0.2, 1.5, m)
    lev[0] = -0.3
    A = (Q * lev[None, :]) @ Q.T
    return mirror(0.5 * (A + A.T))


def nan_case(m=18, seed=42):
    S = spd(m, 1e2, seed)
    S[5, 3] = np.nan                                         # in the lower triangle, which is what the kernels read
    return S


def pack(blocks):
    return np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1) for b in blocks])


def orb_ptr(blocks):
    return np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int64)


def record(section, lines):
    """Keeps ``lines`` as the ``section`` lines of profiles/orbital_sqrt_parity.txt (the other sections stay); a tree that cannot be written is left alone."""
    keep = []
    try:
        with open(PARITY) as f:
            keep = [l.rstrip("\n") for l in f if not l.startswith(section + " ")]
    except OSError:
        pass
    try:
        with open(PARITY, "w") as f:
            f.write("\n".join(sorted(keep + [l if l.startswith(section + " ") else f"{section} {l}" for l in lines], key=lambda l: l.split(" ", 1)[0])) + "\n")
    except OSError:
        pass
