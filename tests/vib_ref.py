"""Float64 numpy restatement of the normal-mode arithmetic of nabladft_amd/vibrations.py, operation by operation (test infrastructure; shared by
tests/test_vib_cpu.py, tests/test_vib_gpu.py, scripts/make_golden_vib.py and scripts/bench_vib.py).

ase is not available: this restates ``ase.vibrations.Vibrations(atoms, delta=0.01, nfree=2)`` from memory, with the two departures the module documents
(the realised float32 step divides the difference; fixed atoms are not displaced).  The eigen-decomposition leg is ``np.linalg.eigh``; ``jacobi`` emulates
the kernel's parallel cyclic Jacobi scheme (round-robin ordering, three phases per round, stopping rule) to pin the scheme itself on a host.
"""
import numpy as np

SIZES = [1, 2, 3, 5, 17, 42, 48]
EPS = 2.0 ** -52


def compact_molecule(n, seed, spacing=1.5, jitter=0.08):
    """The n points of a cubic grid nearest to an off-centre point, jittered: a compact cluster, so that with the Morse pair list of tests/lbfgs_helpers.py
    (cutoff 3.0) and equal masses the softest vibration sits above 5e-2 of the stiffest (a slab-by-slab filling leaves floppy layers below 1e-2)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    side = int(np.ceil(n ** (1.0 / 3.0))) + 2
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    centre = grid.mean(0) + np.array([0.13, 0.07, 0.03])
    pick = np.sort(np.argsort(((grid - centre) ** 2).sum(1), kind="stable")[:n])
    return grid[pick] * spacing + rng.normal(0.0, jitter, size=(n, 3))


def molecules(sizes, seed=5):
    """Compact jittered-grid molecules -> (ptr int64 [B+1], x0 float64 [N, 3]); molecule b uses seed + b."""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x0 = np.concatenate([compact_molecule(int(n), seed + b) for b, n in enumerate(sizes)])
    return ptr, x0


def collinear_molecule(stretch=0.2, a=1.4):
    """A collinear triatomic that is a true minimum of a Morse pair list: the two bonds are stretched by ``stretch`` and the end-to-end pair is compressed
    by exactly what balances them, so the net forces vanish while the tension gives the two bends a restoring force (with every pair at its own equilibrium
    distance a pair potential has no bending stiffness and the molecule seven zero modes, not five).  -> (ptr, x0, Morse table)."""
    from lbfgs_helpers import MORSE_A, morse_table
    u = np.array([0.9, 1.0, 0.4])
    x0 = np.outer(np.arange(3) * a, u / np.linalg.norm(u)) + 7.0
    ptr = np.array([0, 3])
    nbr, d0, mask = morse_table(x0, ptr)
    e = np.exp(-MORSE_A * stretch)
    e2 = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * (1.0 - e) * e))            # (1 - e2) e2 = -(1 - e) e: the compressed pair pushes as hard as a bond pulls
    for i in range(3):
        for k in range(nbr.shape[1]):
            if mask[i, k]:
                d0[i, k] = 2.0 * a + np.log(e2) / MORSE_A if abs(nbr[i, k] - i) == 2 else a - stretch
    return ptr, x0, (nbr, d0, mask)


def plan(ptr, fixed=None):
    ptr = np.asarray(ptr, dtype=np.int64)
    N, B = int(ptr[-1]), len(ptr) - 1
    free = np.ones(N, dtype=bool)
    if fixed is not None:
        free[np.asarray(fixed)] = False
    disp = []                                   # (molecule, atom, axis), molecule-major over the free degrees of freedom
    dof_ptr, hess_ptr = [0], [0]
    for b in range(B):
        atoms = [a for a in range(ptr[b], ptr[b + 1]) if free[a]]
        disp += [(b, a, d) for a in atoms for d in range(3)]
        dof_ptr.append(dof_ptr[-1] + 3 * len(atoms))
        hess_ptr.append(hess_ptr[-1] + 9 * len(atoms) ** 2)
    return dict(free=free, disp=disp, dof_ptr=np.array(dof_ptr), hess_ptr=np.array(hess_ptr), ptr=ptr, B=B, N=N)


def images(x0, pl, c0, c1, delta):
    """Chunk [c0, c1) of the displacement list -> (float32 [image atoms, 3]: per displacement the "-" image then the "+" image of its molecule,
    realised steps float64 [c1 - c0])."""
    x0 = np.asarray(x0, dtype=np.float64)
    out, steps = [], []
    for b, a, d in pl["disp"][c0:c1]:
        mol = slice(int(pl["ptr"][b]), int(pl["ptr"][b + 1]))
        xm, xp = x0[mol].astype(np.float32), x0[mol].astype(np.float32)
        xm[a - mol.start, d] = np.float32(x0[a, d] - delta)
        xp[a - mol.start, d] = np.float32(x0[a, d] + delta)
        steps.append(np.float64(xp[a - mol.start, d]) - np.float64(xm[a - mol.start, d]))
        out += [xm, xp]
    return np.concatenate(out), np.array(steps)


def rows(forces, steps, pl, c0, c1):
    """Forces on the images of chunk [c0, c1) (any float dtype, converted to float64 first) -> list of ((molecule, row), (F- - F+)[free] / h)."""
    forces = np.asarray(forces).astype(np.float64)
    out, at = [], 0
    for i, (b, a, d) in enumerate(pl["disp"][c0:c1]):
        n = int(pl["ptr"][b + 1] - pl["ptr"][b])
        fr = pl["free"][pl["ptr"][b]:pl["ptr"][b + 1]]
        fm, fp = forces[at:at + n][fr].ravel(), forces[at + n:at + 2 * n][fr].ravel()
        out.append(((b, c0 + i - int(pl["dof_ptr"][b])), (fm - fp) / steps[i]))
        at += 2 * n
    return out


def finish(G, im):
    """G [m, m] raw rows -> (H = (G + G^T) / 2, asymmetry max |G - G^T|, A = (im_i H_ij) im_j evaluated on i <= j and mirrored)."""
    H = 0.5 * (G + G.T)
    asym = np.abs(G - G.T).max() if G.size else 0.0
    A = np.triu((im[:, None] * H) * im[None, :])
    return H, asym, A + np.triu(A, 1).T


class VibNumpy:
    """The whole calculation for a batch.  ``forces_of(pos float64 [N, 3]) -> forces [N, 3]`` evaluates the full batch (the molecules are independent);
    ``cast``: the dtype the forces are rounded to before the difference (the model's output dtype).  ``nominal=True`` divides by 2 delta instead of the
    realised step (what ase does; kept to show the difference)."""

    def __init__(self, ptr, x0, masses, fixed=None, delta=0.01):
        self.pl = plan(ptr, fixed)
        self.x0, self.masses, self.delta = np.asarray(x0, dtype=np.float64), np.asarray(masses, dtype=np.float64), delta

    def run(self, forces_of, cast=np.float64, nominal=False):
        pl = self.pl
        x32 = self.x0.astype(np.float32)
        G = [np.zeros((m, m)) for m in np.diff(pl["dof_ptr"])]
        for j, (b, a, d) in enumerate(pl["disp"]):
            xm, xp = x32.copy(), x32.copy()
            xm[a, d] = np.float32(self.x0[a, d] - self.delta)
            xp[a, d] = np.float32(self.x0[a, d] + self.delta)
            h = 2.0 * self.delta if nominal else np.float64(xp[a, d]) - np.float64(xm[a, d])
            mol = slice(int(pl["ptr"][b]), int(pl["ptr"][b + 1]))
            fr = pl["free"][mol]
            fm = np.asarray(forces_of(xm.astype(np.float64)))[mol].astype(cast).astype(np.float64)[fr].ravel()
            fp = np.asarray(forces_of(xp.astype(np.float64)))[mol].astype(cast).astype(np.float64)[fr].ravel()
            G[b][j - pl["dof_ptr"][b]] = (fm - fp) / h
        self.hessian, self.asymmetry, self.omega2, self.modes, self.A = [], [], [], [], []
        for b, g in enumerate(G):
            im = np.repeat(1.0 / np.sqrt(self.masses[pl["ptr"][b]:pl["ptr"][b + 1]][pl["free"][pl["ptr"][b]:pl["ptr"][b + 1]]]), 3)
            H, asym, A = finish(g, im)
            w, U = np.linalg.eigh(A) if A.size else (np.zeros(0), np.zeros((0, 0)))
            self.hessian.append(H), self.asymmetry.append(asym), self.A.append(A), self.omega2.append(w), self.modes.append(U.T * im[None, :])
        return self


def jacobi(A, max_sweeps=30):
    """The kernel's scheme in numpy: round-robin tournament over m padded to even; per round the rotation parameters of all pairs, then all row updates,
    then all column updates (and the eigenvector columns); a sweep starts with off(A)^2 summed directly and stops at off <= m eps |A|_F.
    -> (eigenvalues ascending, eigenvectors as columns, sweeps, status)."""
    A = np.array(A, dtype=np.float64)
    m = A.shape[0]
    V = np.eye(m)
    mp = m + (m & 1)
    fro2 = (A * A).sum()
    thr2 = (m * EPS) ** 2 * fro2
    sweeps, status = 0, 1
    for sweep in range(max_sweeps + 1):
        off2 = ((A - np.diag(np.diag(A))) ** 2).sum()
        if off2 <= thr2:
            status = 0
            break
        if sweep == max_sweeps:
            break
        for r in range(mp - 1):
            t = np.arange(1, mp // 2)
            p = np.concatenate([[mp - 1], (r + t) % (mp - 1)])
            q = np.concatenate([[r], (r - t + (mp - 1)) % (mp - 1)])
            p, q = np.minimum(p, q), np.maximum(p, q)
            keep = q < m
            p, q = p[keep], q[keep]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            rot = apq != 0.0
            p, q, app, aqq, apq = p[rot], q[rot], app[rot], aqq[rot], apq[rot]
            tau = (aqq - app) / (2.0 * apq)
            tt = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            c = 1.0 / np.sqrt(1.0 + tt * tt)
            s = tt * c
            live = s != 0.0
            p, q, c, s = p[live], q[live], c[live], s[live]
            x, y = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
            x, y = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c[None, :] * x - s[None, :] * y, s[None, :] * x + c[None, :] * y
            A[p, q] = 0.0
            A[q, p] = 0.0
            x, y = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c[None, :] * x - s[None, :] * y, s[None, :] * x + c[None, :] * y
        sweeps += 1
    order = np.argsort(np.diag(A), kind="stable")
    return np.diag(A)[order], V[:, order], sweeps, status


def eig_errors(A, w, V):
    """The three figures of the eigensolver check in units of m eps: sorted eigenvalues against np.linalg.eigh and max |A V - V diag(w)|, both relative to
    |A|_2, and max |V^T V - I|.  V holds the eigenvectors as columns."""
    m = A.shape[0]
    ref = np.linalg.eigh(A)[0]
    norm2 = max(np.abs(ref).max(), np.finfo(np.float64).tiny)
    unit = m * EPS
    return (np.abs(w - ref).max() / norm2 / unit, np.abs(A @ V - V * w[None, :]).max() / norm2 / unit, np.abs(V.T @ V - np.eye(m)).max() / unit)


def count_near_zero(w):
    """(number of eigenvalues below 1e-4 of the largest in magnitude, the next one relative to the largest)."""
    w = np.sort(np.asarray(w))
    top = np.abs(w).max()
    if top == 0.0:
        return len(w), np.inf
    k = int((np.abs(w) < 1e-4 * top).sum())
    rest = np.abs(w)[np.abs(w) >= 1e-4 * top]
    return k, float(rest.min() / top)
