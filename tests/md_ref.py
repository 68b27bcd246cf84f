"""Shared by the MD tests and scripts/bench_md.py (test infrastructure): a float64 numpy restatement of the equations nabladft_amd/md.py lists (velocity
Verlet, Langevin with fix_com, fixed atoms, MaxwellBoltzmann + Stationary + ZeroRotation, the observables), vectorised over the batch with
``np.add.reduceat``, and a numpy Philox4x32-10 + Box-Muller with the counter layout of csrc/md.hip.

``MDNumpy.launch`` mirrors one ``nq_md_step`` launch: (a) the pending second half-kick, (c) the next first half-kick and drift, with the operations in the
order the kernel uses (md.hip is compiled without a * b + c contraction).  ``dtype=np.longdouble`` evaluates the same formulae in extended precision; a
permuted atom order (``inner_perm``) changes the order of every per-molecule sum: the two together measure the restatement's own spread."""
import numpy as np

E_H_SI, AMU_SI, K_SI = 4.359744650e-18, 1.660539040e-27, 1.38064852e-23          # CODATA 2014
KAPPA = E_H_SI * (1e-15 * 1e-15) / (AMU_SI * (1e-10 * 1e-10))
KB = K_SI / E_H_SI
SIZES = [1, 2, 3, 63, 64, 65, 192, 193, 512]


def inner_perm(sizes, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    return np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])])


class MDNumpy:
    def __init__(self, ptr, masses, x, v=None, fixed=None, dtype=np.float64):
        self.ptr = np.asarray(ptr, dtype=np.int64)
        self.sizes = np.diff(self.ptr)
        self.dtype = dtype
        self.m = np.asarray(masses, dtype=dtype)[:, None]
        self.x = np.array(x, dtype=dtype)
        self.v = np.zeros_like(self.x) if v is None else np.array(v, dtype=dtype)
        self.fixed = np.zeros(self.x.shape[0], dtype=bool)
        if fixed is not None:
            self.fixed[np.asarray(fixed)] = True
        self.pending, self.step, self.rnd_vel = False, 0, None

    def seg(self, a):
        return np.add.reduceat(a, self.ptr[:-1], axis=0)

    def atoms(self, per_mol):
        return np.repeat(per_mol, self.sizes, axis=0)

    def acc(self, f):
        return KAPPA * np.asarray(f).astype(self.dtype) / self.m

    def noise(self, xi, eta, dt, kT, fr):
        d = self.dtype
        dt, kT, fr = d(dt), d(kT), d(fr)
        sdt = np.sqrt(dt)
        dt15 = dt * sdt
        sigma = np.sqrt(2.0 * KAPPA * kT * fr / self.m)
        c3 = sdt * sigma / 2.0 - dt15 * fr * sigma / 8.0
        c5 = dt15 * sigma / (2.0 * np.sqrt(d(3.0)))
        c4 = fr / 2.0 * c5
        rp = c5 * np.asarray(eta, dtype=d)
        rv = c3 * np.asarray(xi, dtype=d) - c4 * np.asarray(eta, dtype=d)
        n = self.atoms(self.sizes.astype(d))[:, None]
        rp = rp - self.atoms(self.seg(rp)) / n
        rv = rv - self.atoms(self.seg(self.m * rv)) / (self.m * n)
        return rp, rv

    def launch(self, f, mode=0, dt=0.5, kT=0.0, fr=0.0, xi=None, eta=None, finish_only=False):
        d = self.dtype
        a = self.acc(f)
        dt_, fr_ = d(dt), d(fr if mode else 0.0)
        hdt = d(0.5) * dt_
        c1 = dt_ / 2.0 - dt_ * dt_ * fr_ / 8.0
        c2 = dt_ * fr_ / 2.0 - dt_ * dt_ * fr_ * fr_ / 8.0
        free = ~self.fixed[:, None]
        if self.pending:
            self.v = np.where(free, self.v + hdt * a if mode == 0 else self.v + ((c1 * a - c2 * self.v) + self.rnd_vel), 0.0)
            self.pending = False
        if finish_only:
            return
        if mode == 0:
            vh = self.v + hdt * a
            self.v = np.where(free, vh, 0.0)
            self.x = np.where(free, self.x + dt_ * vh, self.x)
        else:
            rp, rv = self.noise(xi, eta, dt, kT, fr)
            vh = self.v + ((c1 * a - c2 * self.v) + rv)
            xn = (self.x + dt_ * vh) + rp
            self.v = np.where(free, ((xn - self.x) - rp) / dt_, 0.0)
            self.x = np.where(free, xn, self.x)
            self.rnd_vel = rv
        self.pending = True
        self.step += 1

    # ---- velocity initialisation -------------------------------------------------------------------------------------------------------------
    def init_velocities(self, zeta, kT, remove_translation=True, remove_rotation=True):
        d = self.dtype
        free = ~self.fixed[:, None]
        v = np.where(free, np.asarray(zeta, dtype=d) * np.sqrt(KAPPA * d(kT) / self.m), 0.0)
        if remove_translation:
            v = np.where(free, v - self.atoms(self.seg(self.m * v) / self.seg(self.m)), 0.0)
        if remove_rotation:
            dd = self.x - self.atoms(self.seg(self.m * self.x) / self.seg(self.m))
            L = self.seg(self.m * np.cross(dd, v))
            r2 = (dd ** 2).sum(1, keepdims=True)
            I = self.seg((self.m * (r2 * np.eye(3, dtype=d)[None].reshape(1, 9) - (dd[:, :, None] * dd[:, None, :]).reshape(-1, 9)))).reshape(-1, 3, 3)
            omega = np.zeros_like(L)
            for b in range(L.shape[0]):
                w, V = np.linalg.eigh(I[b].astype(np.float64))
                for e in range(3):
                    if w[e] > 1e-10 * np.trace(I[b]):
                        omega[b] += (V[:, e] @ L[b]) / w[e] * V[:, e]
            v = np.where(free, v - np.cross(self.atoms(omega), dd), 0.0)
        self.v = v
        self.pending = False

    # ---- observables -------------------------------------------------------------------------------------------------------------------------
    def observables(self, epot=None):
        m, x, v = self.m, self.x, self.v
        ekin = 0.5 * self.seg(m * (v ** 2).sum(1, keepdims=True))[:, 0] / KAPPA
        dof = 3.0 * self.seg((~self.fixed).astype(self.dtype))
        T = np.where(dof > 0, 2.0 * ekin / (np.where(dof > 0, dof, 1.0) * KB), 0.0)
        dd = x - self.atoms(self.seg(m * x) / self.seg(m))
        P = self.seg(m * v)
        L = self.seg(m * np.cross(dd, v))
        epot = np.zeros_like(ekin) if epot is None else np.asarray(epot, dtype=self.dtype)
        return {"ekin": ekin, "temperature": T, "epot": epot, "etot": epot + ekin, "P": P, "L": L, "p_norm": np.sqrt((P ** 2).sum(1)), "l_norm": np.sqrt((L ** 2).sum(1))}


# ---- Philox4x32-10 + Box-Muller ---------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Arrays of uint64 holding 32-bit words -> the four output words after 10 rounds."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
    return c0, c1, c2, c3


def normals(seed, step, draw, ptr, mol_key=None):
    """float64 [N, 3]: what nq_md_normals writes.  Counter (key low, key high, step, atom << 8 | group << 2 | component), key = (seed low, seed high);
    u = (52 bits + 1/2) 2^-52; z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = ... sin(...); even draws take z0, odd draws z1, group = draw // 2."""
    ptr = np.asarray(ptr, dtype=np.int64)
    sizes = np.diff(ptr)
    B, N = sizes.shape[0], int(ptr[-1])
    key = (np.arange(B, dtype=np.int64) if mol_key is None else np.asarray(mol_key, dtype=np.int64)).view(np.uint64)
    key = np.repeat(key, sizes)
    atom = (np.arange(N, dtype=np.int64) - np.repeat(ptr[:-1], sizes)).astype(np.uint64)
    seed = np.array([seed], dtype=np.int64).view(np.uint64)[0]
    out = np.empty((N, 3))
    for c in range(3):
        w = philox4x32(key & _M32, key >> np.uint64(32), np.full(N, np.int64(step) & 0xFFFFFFFF, dtype=np.uint64),
                       (atom << np.uint64(8)) | np.uint64(((draw >> 1) << 2) | c), seed & _M32, seed >> np.uint64(32))
        u1 = (((w[0] << np.uint64(20)) | (w[1] >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
        u2 = (((w[2] << np.uint64(20)) | (w[3] >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
        out[:, c] = rad * np.sin(ang) if draw & 1 else rad * np.cos(ang)
    return out


# ---- shared set-ups ---------------------------------------------------------------------------------------------------------------------------
def random_system(sizes, seed):
    """ptr, masses (H / C / N / O weights), positions, velocities of a random batch."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(ptr[-1])
    masses = rng.choice([1.008, 12.011, 14.007, 15.999], size=N)
    return ptr, masses, rng.normal(0.0, 2.0, size=(N, 3)), rng.normal(0.0, 0.01, size=(N, 3))


def lattice_molecule(n, seed, spacing=1.5):
    """n atoms on a jittered cubic lattice: every atom has Morse partners inside the cutoff of tests/lbfgs_helpers.py."""
    rng = np.random.Generator(np.random.PCG64(seed))
    side = int(np.ceil(n ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    return grid * spacing + rng.normal(0.0, 0.08, size=(n, 3))


def replay(ptr, masses, x0, v0, forces, mode, dt, kT, fr, xi, eta, fixed, dtype=np.float64, perm=None):
    """Teacher-forced: one launch per entry of ``forces``; -> (r after every launch, v after every launch), in the caller's atom order."""
    sel = slice(None) if perm is None else perm
    fx = None
    if fixed is not None:
        mask = np.zeros(len(masses), dtype=bool)
        mask[np.asarray(fixed)] = True
        fx = mask[sel]
    md = MDNumpy(ptr, masses[sel], x0[sel], v0[sel], fx, dtype)
    inv = slice(None) if perm is None else np.argsort(perm)
    rs, vs = [], []
    for k, f in enumerate(forces):
        md.launch(f[sel], mode, dt, kT, fr, None if xi is None else xi[k][sel], None if eta is None else eta[k][sel])
        rs.append(md.x[inv].copy()), vs.append(md.v[inv].copy())
    return np.array(rs), np.array(vs)


def spread_and_tolerance(ptr, masses, x0, v0, forces, mode, dt, kT, fr, xi, eta, fixed):
    """The restatement's own spread (permuted summation order, np.longdouble) and the tolerance rule of the L-BFGS tests: 1000 x spread, floor 1e-13."""
    sizes = np.diff(ptr)
    base = replay(ptr, masses, x0, v0, forces, mode, dt, kT, fr, xi, eta, fixed)
    perm = replay(ptr, masses, x0, v0, forces, mode, dt, kT, fr, xi, eta, fixed, perm=inner_perm(sizes, 5))
    ld = replay(ptr, masses, x0, v0, forces, mode, dt, kT, fr, xi, eta, fixed, dtype=np.longdouble)
    out = {}
    for name, i in (("r", 0), ("v", 1)):
        sp = float(np.abs(perm[i] - base[i]).max())
        sl = float(np.abs(ld[i].astype(np.float64) - base[i]).max())
        out[name] = {"spread_permuted": sp, "spread_longdouble": sl, "tolerance": max(1000.0 * max(sp, sl), 1e-13)}
    return base, out
