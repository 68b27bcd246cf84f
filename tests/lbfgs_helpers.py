"""Shared by the L-BFGS tests, the fixture generator (scripts/make_golden_lbfgs.py) and scripts/bench_optimize.py (test infrastructure).

* a per-molecule Morse potential over a fixed pair list, as a padded neighbour table, so that numpy (float64, host) and torch (float64, device) evaluate the
  same gather-and-sum formula without any atomic: V = sum_pairs D (1 - exp(-a (d - d0)))^2;
* ``LbfgsNumpy``: a float64 numpy restatement of ONE optimiser step of nablaDFT/optimization/optimizers.py:437-605 (no line search), vectorised over the
  batch with segment sums -- the yardstick the kernel is compared with on random inputs.
"""
import numpy as np

MORSE_D, MORSE_A, MORSE_CUT = 0.1, 1.0, 3.0


def morse_table(ref_pos, ptr):
    """Padded neighbour table of the pairs closer than MORSE_CUT in the reference geometry: nbr int64 [N, K] (own index where padded), d0 [N, K], mask."""
    ref_pos = np.asarray(ref_pos, dtype=np.float64)
    N = ref_pos.shape[0]
    lists = [[] for _ in range(N)]
    for a, b in zip(ptr[:-1], ptr[1:]):
        p = ref_pos[a:b]
        d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        ii, jj = np.nonzero((d < MORSE_CUT) & ~np.eye(b - a, dtype=bool))
        for i, j in zip(ii, jj):
            lists[a + i].append((a + j, d[i, j]))
    K = max(1, max(len(l) for l in lists))
    nbr = np.repeat(np.arange(N)[:, None], K, 1)
    d0 = np.ones((N, K))
    mask = np.zeros((N, K), dtype=bool)
    for i, l in enumerate(lists):
        for k, (j, dd) in enumerate(l):
            nbr[i, k], d0[i, k], mask[i, k] = j, dd, True
    return nbr, d0, mask


def permute_table(table, perm):
    """The table of the same molecules with atoms renumbered: new atom i is old atom perm[i]."""
    nbr, d0, mask = table
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    return inv[nbr[perm]], d0[perm], mask[perm]


def morse_np(pos, table, ptr=None):
    """-> (forces [N, 3], energy per molecule or None), float64."""
    nbr, d0, mask = table
    rij = pos[:, None, :] - pos[nbr]
    d = np.sqrt((rij ** 2).sum(-1))
    d = np.where(mask, d, 1.0)
    e = np.exp(-MORSE_A * (d - d0))
    g = np.where(mask, 2.0 * MORSE_D * MORSE_A * (1.0 - e) * e / d, 0.0)
    forces = -(g[:, :, None] * rij).sum(1)
    energy = None
    if ptr is not None:
        per_atom = 0.5 * np.where(mask, MORSE_D * (1.0 - e) ** 2, 0.0).sum(1)
        energy = np.add.reduceat(per_atom, ptr[:-1])
    return forces, energy


def morse_torch(pos, table_dev):
    """Forces of float64 device positions; table_dev = the table as device tensors.  Gathers and a dense sum over K: bitwise reproducible."""
    import torch
    nbr, d0, mask = table_dev
    rij = pos[:, None, :] - pos[nbr]
    d = torch.where(mask, rij.pow(2).sum(-1).sqrt(), torch.ones_like(d0))
    e = torch.exp(-MORSE_A * (d - d0))
    g = torch.where(mask, 2.0 * MORSE_D * MORSE_A * (1.0 - e) * e / d, torch.zeros_like(d0))
    return -(g[:, :, None] * rij).sum(1)


class LbfgsNumpy:
    """One object per run; ``step(r, f)`` returns the new positions.  r float64 [N, 3]; f any float dtype (converted to float64 first, as the kernel does)."""

    def __init__(self, ptr, memory=100, maxstep=0.2, damping=1.0, alpha=1.0, fixed=None):
        self.ptr = np.asarray(ptr, dtype=np.int64)
        self.sizes = np.diff(self.ptr)
        self.B, self.N = self.sizes.shape[0], int(self.ptr[-1])
        self.memory, self.maxstep, self.damping, self.H0 = memory, maxstep, damping, 1.0 / alpha
        self.fixed = None if fixed is None else np.asarray(fixed)
        self.iteration, self.n_normalizations = 0, 0
        self.s, self.y, self.rho = [], [], []
        self.r0 = self.f0 = None
        self.mask = None

    def _dot(self, a, b):
        return np.add.reduceat((a * b).sum(1), self.ptr[:-1])

    def _atoms(self, per_mol):
        return np.repeat(per_mol, self.sizes)[:, None]

    def forces(self, f):
        f = np.array(f, dtype=np.float64)
        if self.fixed is not None:
            f[self.fixed] = 0.0
        return f

    def converged_mask(self, f, fmax):
        return np.maximum.reduceat((self.forces(f) ** 2).sum(1), self.ptr[:-1]) < fmax ** 2

    def step(self, r, f, fmax):
        r = np.array(r, dtype=np.float64)            # own copies: r0 / f0 outlive the caller's buffers
        f = self.forces(f)
        mask = self.mask = np.maximum.reduceat((f ** 2).sum(1), self.ptr[:-1]) < fmax ** 2
        if self.iteration > 0:
            s0, y0 = r - self.r0, self.f0 - f
            ys = self._dot(y0, s0)
            self.s.append(s0), self.y.append(y0), self.rho.append(np.where(ys > 1e-8, 1.0 / np.where(ys > 1e-8, ys, 1.0), 1.0))
        if self.iteration > self.memory:
            self.s.pop(0), self.y.pop(0), self.rho.pop(0)
        L = min(self.memory, self.iteration)
        a = [None] * L
        q = -f
        for i in range(L - 1, -1, -1):
            a[i] = self.rho[i] * self._dot(self.s[i], q)
            q = q - self._atoms(a[i]) * self.y[i]
        z = self.H0 * q
        for i in range(L):
            b = self.rho[i] * self._dot(self.y[i], z)
            z = z + self.s[i] * self._atoms(a[i] - b)
        p = np.where(self._atoms(mask), 0.0, -z)
        longest = np.maximum.reduceat(np.sqrt((p ** 2).sum(1)), self.ptr[:-1])
        clamp = longest >= self.maxstep
        self.n_normalizations += int(clamp.sum())
        scale = np.where(clamp, self.maxstep / np.where(clamp, longest, 1.0), 1.0)
        dr = np.where(self._atoms(clamp), p * self._atoms(scale), p) * self.damping
        self.iteration += 1
        self.r0, self.f0 = r, f
        return r + dr
