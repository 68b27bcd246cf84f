"""Batched molecular dynamics with the whole state on the GPU: NVE (velocity Verlet) and Langevin NVT, hundreds or thousands of independent trajectories per
kernel launch (csrc/md.hip, ``nq_md_*`` of include/nablaq.h).

Mirrors ``nablaDFT.optimization.PYGAseInterface`` (nablaDFT/optimization/pyg_ase_interface.py:119-335), which drives ase one molecule at a time and copies
device -> host -> device every step.  Parity status: **restated, unpinned** -- ase is neither in the reference tree nor a dependency here, so the integrators
below are a restatement of ase 3.22.1 (the version the reference's setup.py pins) from memory; the kernels are tested against a float64 numpy restatement
of the same equations (tests/md_ref.py) and against physical invariants, not against ase.

Units: Hartree, Angstrom, amu, fs, K (the models' native units stay the only ones, as in optimization.py).  Derived from CODATA 2014 SI values, the set ase
3.22.1's default ``units`` uses:
    KAPPA = E_h (1e-15 s)^2 / (amu (1e-10 m)^2)   (Hartree / Angstrom) / amu -> Angstrom / fs^2     ~ 0.26255
    KB    = k / E_h                               Hartree / K                                      ~ 3.16681e-6

Equations (all state float64; per atom a = KAPPA F / m, dt in fs, friction fr in 1/fs, kT = KB T):
  NVE (ase VelocityVerlet, pyg_ase_interface.py:239):   v += dt/2 a(x);  x += dt v;  forces;  v += dt/2 a(x)
  NVT (ase Langevin with fix_com=True, :241-246):       sigma = sqrt(2 KAPPA kT fr / m), c1 = dt/2 - dt^2 fr/8, c2 = dt fr/2 - dt^2 fr^2/8,
      c3 = sqrt(dt) sigma/2 - dt^1.5 fr sigma/8, c5 = dt^1.5 sigma/(2 sqrt 3), c4 = fr/2 c5;  xi, eta ~ N(0,1) [n,3];  rnd_pos = c5 eta, rnd_vel = c3 xi - c4 eta;
      per molecule rnd_pos -= mean(rnd_pos), rnd_vel -= sum(m rnd_vel) / (m n);  v += c1 a - c2 v + rnd_vel;  x' = x + dt v + rnd_pos;  v = (x' - x - rnd_pos)/dt;
      forces;  v += c1 a' - c2 v + rnd_vel (the same rnd_vel)
  Fixed atoms (ase FixAtoms, :159-162): positions never change, v = 0 after every half step, dof = 3 (n - n_fixed)
  Velocities (_init_velocities, :265-282): v = zeta sqrt(KAPPA kT_init / m);  Stationary: v -= sum(m v)/sum(m);  ZeroRotation: I omega = L about the centre of
      mass in the eigenbasis of I, omega = 0 along eigenvalues <= 1e-10 trace(I) (atoms, diatomics, linear molecules), v -= omega x (x - x_com)
  Observables per molecule: E_kin = sum(m |v|^2) / (2 KAPPA) [Hartree], T = 2 E_kin / (dof KB), E_pot (model), E_tot, |P|, |L|

One ``nq_md_step`` launch = one MD step: it finishes the previous step's second half-kick with the new forces, samples the now consistent (x, v, F) into the
device log / frame rings, and does the next first half-kick and drift.  Random numbers are generated on the device (Philox4x32-10 keyed by ``seed``, counter
(mol_key, step, atom inside the molecule, draw), Box-Muller in float64): a trajectory rerun alone reproduces the one it had inside a batch, bit for bit.

Limits (each raises, nothing degrades silently): Hartree / Angstrom only; molecules of at most 512 atoms; ase's binary ``.traj`` is not written (frames go to
``<name>.npz`` and the last frame to ``<name>.extxyz``); ``compute_normal_modes`` is vibrations.py and has its own limits; ``optimize`` runs the device L-BFGS of optimization.py, not ase's
``QuasiNewton`` (BFGS + line search), and ``optimizer_class`` is accepted and ignored; no periodic cells, no thermostat but Langevin, no barostat, one time
step and one temperature per batch.
"""
import ctypes as C
import os
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._devstate import DeviceState, batch_ptr_host, fixed_to_uint8, require_forces, require_positions
from .optimization import ASEBatchwiseLBFGS, PyGBatchwiseCalculator
from .trainer import Batch

# ---- units: the one table --------------------------------------------------------------------------------------------------------------------------
E_H_SI = 4.359744650e-18      # J      CODATA 2014 Hartree energy
AMU_SI = 1.660539040e-27      # kg     CODATA 2014 atomic mass constant
K_SI = 1.38064852e-23         # J / K  CODATA 2014 Boltzmann constant
# a [Angstrom/fs^2] = F [Hartree/Angstrom] / m [amu] * KAPPA:  Hartree / (amu Angstrom) = E_h / (amu_kg 1e-10 m) m/s^2, and 1 m/s^2 = 1e10 Angstrom / (1e15 fs)^2
KAPPA = E_H_SI * (1e-15 * 1e-15) / (AMU_SI * (1e-10 * 1e-10))
KB = K_SI / E_H_SI

SYMBOLS = ("X", "H", "He", "Li", "Be", "B", "C", "N", "O", "F", "Ne", "Na", "Mg", "Al", "Si", "P", "S", "Cl", "Ar", "K", "Ca", "Sc", "Ti", "V", "Cr", "Mn", "Fe",
           "Co", "Ni", "Cu", "Zn", "Ga", "Ge", "As", "Se", "Br", "Kr")
# standard atomic weights, Z = 1..36 (typed from memory: unpinned; pass ``masses=`` to override)
ATOMIC_MASSES = (0.0, 1.008, 4.002602, 6.94, 9.0121831, 10.81, 12.011, 14.007, 15.999, 18.998403163, 20.1797, 22.98976928, 24.305, 26.9815385, 28.085,
                 30.973761998, 32.06, 35.45, 39.948, 39.0983, 40.078, 44.955908, 47.867, 50.9415, 51.9961, 54.938044, 55.845, 58.933194, 58.6934, 63.546, 65.38,
                 69.723, 72.630, 74.921595, 78.971, 79.904, 83.798)

_HDR = ("step", "status", "pending", "log_rows", "frames", "overflow", "N", "B", "n_small", "log_capacity", "frame_capacity", "flags", "last_sampled")
LOG_COLUMNS = ("step", "etot", "epot", "ekin", "temperature", "p_norm", "l_norm", "reserved")
_FLAG_LOG, _FLAG_FRAMES, _FLAG_VEL = 1, 2, 4


def masses_for(z, masses=None) -> np.ndarray:
    """float64 [N] masses in amu: ``masses`` if given, else the table; a Z outside the table raises ValueError (a mass is never guessed)."""
    z = np.asarray(z.cpu() if isinstance(z, torch.Tensor) else z).astype(np.int64).reshape(-1)
    if masses is not None:
        m = np.asarray(masses.cpu() if isinstance(masses, torch.Tensor) else masses, dtype=np.float64).reshape(-1)
        if m.shape[0] != z.shape[0]:
            raise ValueError(f"masses has {m.shape[0]} entries for {z.shape[0]} atoms")
        return np.ascontiguousarray(m)
    bad = (z < 1) | (z >= len(ATOMIC_MASSES))
    if bad.any():
        raise ValueError(f"no atomic mass for Z={sorted(set(z[bad].tolist()))}: the table covers Z=1..{len(ATOMIC_MASSES) - 1}, pass masses= for other elements")
    return np.asarray(ATOMIC_MASSES, dtype=np.float64)[z]


# ---- device state -----------------------------------------------------------------------------------------------------------------------
class MDState(DeviceState):
    """One caller-owned device buffer behind ``nq_md_init`` / ``nq_md_step`` plus typed views of its parts (include/nablaq.h; entry points added under ABI 17).
    ``log_capacity`` / ``frame_capacity``: rows of the device rings, 0 or None = that ring is not kept."""

    def __init__(self, ptr_host: Sequence[int], pos: torch.Tensor, masses, fixed=None, mol_key=None, velocities: Optional[torch.Tensor] = None,
                 log_capacity: Optional[int] = 0, frame_capacity: Optional[int] = 0, store_velocities: bool = False):
        require_positions(pos, "md")
        ptr_host = np.ascontiguousarray(np.asarray(ptr_host, dtype=np.int32))
        self.B, self.N = int(ptr_host.shape[0]) - 1, int(pos.shape[0])
        self.ptr_host = ptr_host
        self.log_capacity, self.frame_capacity = int(log_capacity or 0), int(frame_capacity or 0)
        self.flags = (_FLAG_LOG if log_capacity else 0) | (_FLAG_FRAMES if frame_capacity else 0) | (_FLAG_VEL if store_velocities else 0)
        masses = np.ascontiguousarray(np.asarray(masses, dtype=np.float64).reshape(-1))
        if masses.shape[0] != self.N:
            raise ValueError(f"masses has {masses.shape[0]} entries for {self.N} atoms")
        fixed_host = fixed_to_uint8(fixed, self.N)
        key_host = None if mol_key is None else np.ascontiguousarray(np.asarray(mol_key, dtype=np.int64).reshape(-1))
        if key_host is not None and key_host.shape[0] != self.B:
            raise ValueError(f"mol_key has {key_host.shape[0]} entries for {self.B} molecules")
        self.mol_key = np.arange(self.B, dtype=np.int64) if key_host is None else key_host
        N, B, lc, fc, i32, f64 = self.N, self.B, self.log_capacity, self.frame_capacity, torch.int32, torch.float64
        self.frame_velocities = None
        nbytes = self._allocate("md", (N, B, lc, fc, self.flags), (
            ("header_dev", i32, (32,)), ("ptr_dev", i32, (B + 1,)), (None, i32, (B,)), ("key_dev", torch.int64, (B,)), ("mass", f64, (N,)),
            (None, torch.uint8, (N,)), ("r", f64, (N, 3)), ("v", f64, (N, 3)), (None, f64, (N, 3)), ("log", f64, (lc, B, 8)), ("frames", f64, (fc, N, 3)),
            ("frame_velocities" if store_velocities else None, f64, (fc, N, 3))), pos.device)
        self.pos32 = torch.empty(self.N, 3, dtype=torch.float32, device=pos.device)      # what the model reads; written by the step kernel
        pos = pos.contiguous()
        if velocities is not None:
            velocities = velocities.to(device=pos.device, dtype=torch.float64).contiguous()
            if tuple(velocities.shape) != (self.N, 3):
                raise ValueError(f"velocities must be [{self.N}, 3]")
        n_small = C.c_int32(0)
        hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.load().nq_md_init(_lib.ptr(self.buf), nbytes, hp(ptr_host), hp(key_host), hp(masses), hp(fixed_host), *self._dims, _lib.ptr(pos),
                                          int(pos.dtype == torch.float64), _lib.ptr(velocities), _lib.ptr(self.pos32), C.byref(n_small), _lib.stream_ptr()))
        self.n_small = n_small.value
        self.masses_host, self.fixed_host = masses, fixed_host

    def _args(self):
        return (_lib.ptr(self.buf), self.N, self.B, self.n_small, self.log_capacity, self.frame_capacity, self.flags)

    def init_velocities(self, temp_init: float = 300.0, seed: int = 0, remove_translation: bool = True, remove_rotation: bool = True):
        _lib.check(_lib.load().nq_md_init_velocities(*self._args(), float(temp_init), int(seed), int(remove_translation), int(remove_rotation), _lib.stream_ptr()))

    def step(self, forces: torch.Tensor, energies: Optional[torch.Tensor] = None, mode: int = 0, dt: float = 0.5, kT: float = 0.0, friction: float = 0.0,
             interval: int = 1, seed: int = 0, xi: Optional[torch.Tensor] = None, eta: Optional[torch.Tensor] = None, finish_only: bool = False):
        dev = self.buf.device
        forces = require_forces(forces, self.N, dev)
        if energies is not None:
            energies = energies.reshape(-1).contiguous()
            if energies.dtype not in (torch.float32, torch.float64) or energies.shape[0] != self.B or energies.device != dev:
                raise ValueError(f"energies must be a float32 / float64 [{self.B}] tensor on {dev}")
        for name, t in (("xi", xi), ("eta", eta)):
            if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (self.N, 3) or t.device != dev or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 [{self.N}, 3] tensor on {dev}")
        _lib.check(_lib.load().nq_md_step(*self._args(), _lib.ptr(forces), int(forces.dtype == torch.float64), _lib.ptr(energies),
                                          int(energies is not None and energies.dtype == torch.float64), _lib.ptr(self.pos32), int(mode), float(dt), float(kT),
                                          float(friction), int(interval), int(seed), _lib.ptr(xi), _lib.ptr(eta), int(finish_only), _lib.stream_ptr()))
        # the kernel wrote pos32 through a raw pointer: move its version counter, so that a prepared batch (net.prepare(data), _lib.geometry_key) built for
        # the previous geometry is refused instead of silently reused
        if not finish_only:
            torch.autograd.graph.increment_version(self.pos32)

    def normals(self, seed: int, step: int, draw: int) -> torch.Tensor:
        """float64 [N, 3]: exactly the normals the kernels draw at (seed, step); draw 0 = xi, 1 = eta, 2 = zeta of the velocity initialisation."""
        out = torch.empty(self.N, 3, dtype=torch.float64, device=self.buf.device)
        _lib.check(_lib.load().nq_md_normals(int(seed), int(step), int(draw), _lib.ptr(self.ptr_dev), _lib.ptr(self.key_dev), self.N, self.B, _lib.ptr(out),
                                             _lib.stream_ptr()))
        return out

    def header(self) -> dict:
        """The header words (one small device->host copy, synchronises the stream)."""
        h = self._read_header()
        if h[1] < 0:
            raise RuntimeError("nq_md_step was called with other dimensions than nq_md_init prepared the state for")
        return dict(zip(_HDR, h))

    def drain(self):
        """-> (log rows [rows, B, 8], frames [frames, N, 3], frame velocities or None) as host arrays; empties both rings (stream-ordered)."""
        h = self.header()
        rows, frames = h["log_rows"], h["frames"]
        log = self.log[:rows].cpu().numpy()
        fr = self.frames[:frames].cpu().numpy()
        fv = self.frame_velocities[:frames].cpu().numpy() if self.frame_velocities is not None else None
        self.header_dev[3:5].zero_()
        return log, fr, fv


# ---- the integrator ---------------------------------------------------------------------------------------------------------------------
class BatchedMD:
    """Batched NVE / Langevin dynamics driven by a ``PyGBatchwiseCalculator`` (any of the engines, or a callable ``Batch -> (energy, forces)``).

    ``temp_bath=None``: NVE; a temperature in K: Langevin NVT with ``friction`` in 1/fs (the reference uses 1/(100 fs), pyg_ase_interface.py:245).
    ``interval``: every interval-th step is sampled into the log ring and, if ``frames`` (a ring capacity) is given, into the frame ring.
    ``run(batch, steps)``: one model call on the start geometry, then steps x (step kernel + model call), then the finishing call (second half-kick and sample
    of the last step).  The host reads the header only every ``check_every`` steps and drains the rings when the next sample would not fit.  Afterwards:
    ``positions`` / ``velocities`` (float64 device tensors), ``log`` [rows, B, 8] (LOG_COLUMNS) and ``trajectory`` [frames, N, 3] (host arrays, everything since
    the state was created), ``nsteps``.  A second ``run`` continues the trajectory; ``time_step``, ``temp_bath``, ``friction`` and ``interval`` may be changed
    between runs (equilibration, then production)."""

    def __init__(self, calculator, time_step: float = 0.5, temp_bath: Optional[float] = None, friction: float = 0.01, fixed_atoms_mask=None, masses=None,
                 seed: int = 0, interval: int = 1, frames: Optional[int] = None, store_velocities: bool = False, check_every: int = 50, log_capacity: Optional[int] = 128,
                 mol_key=None):
        if check_every < 1 or interval < 1:
            raise ValueError("check_every and interval must be >= 1")
        if frames is not None and frames < 1:
            raise ValueError("frames is a ring capacity of at least 1, or None for no frames")
        self.calculator, self.time_step, self.temp_bath, self.friction = calculator, time_step, temp_bath, friction
        self.fixed_atoms_mask, self.masses, self.seed, self.interval = fixed_atoms_mask, masses, int(seed), int(interval)
        self.frame_capacity, self.store_velocities, self.check_every, self.log_capacity, self.mol_key = frames, store_velocities, int(check_every), int(log_capacity or 0), mol_key
        self.state = self._work = None
        self.nsteps = 0

    def _ensure_state(self, batch) -> MDState:
        if self.state is not None:
            if self.state.N != int(batch.pos.shape[0]):
                raise ValueError("this BatchedMD holds the state of another batch")
            return self.state
        m = masses_for(batch.z, self.masses)
        st = self.state = MDState(batch_ptr_host(batch), batch.pos, m, self.fixed_atoms_mask, self.mol_key, None, self.log_capacity, self.frame_capacity, self.store_velocities)
        # the model's batch: same z / batch / ptr tensors, positions = the float32 tensor the step kernel rewrites
        self._work = Batch(st.pos32, batch.z, batch.batch, getattr(batch, "y", None), getattr(batch, "forces", None), batch.ptr if getattr(batch, "ptr", None) is not None else None)
        self._log, self._frames, self._fvel = [], [], []
        self._rows_dev = self._frames_dev = 0
        self._last_sampled = -1
        self.nsteps = 0
        return st

    def init_velocities(self, batch, temp_init: float = 300.0, remove_translation: bool = True, remove_rotation: bool = True):
        self._ensure_state(batch).init_velocities(temp_init, self.seed, remove_translation, remove_rotation)

    def _drain(self):
        log, fr, fv = self.state.drain()
        if log.shape[0]:
            self._log.append(log)
        if fr.shape[0]:
            self._frames.append(fr)
            if fv is not None:
                self._fvel.append(fv)
        self._rows_dev = self._frames_dev = 0

    def _launch(self, finish_only):
        st, calc = self.state, self.calculator
        if self.nsteps % self.interval == 0 and self._last_sampled != self.nsteps:      # this launch samples: make room first
            if self._rows_dev == st.log_capacity and st.log_capacity or self._frames_dev == st.frame_capacity and st.frame_capacity:
                self._drain()
            self._rows_dev += 1
            self._frames_dev += 1
            self._last_sampled = self.nsteps
        nvt = self.temp_bath is not None
        st.step(calc.forces, calc.energy, 1 if nvt else 0, self.time_step, KB * self.temp_bath if nvt else 0.0, self.friction if nvt else 0.0, self.interval,
                self.seed, finish_only=finish_only)
        if not finish_only:
            self.nsteps += 1

    def _check(self):
        h = self.state.header()
        if h["overflow"]:
            raise RuntimeError("an MD sample was dropped: a device ring was full (the host-side drain schedule and the kernel disagree)")
        return h

    def run(self, batch, steps: int):
        st = self._ensure_state(batch)
        calc = self.calculator
        calc.calculate(self._work)
        for k in range(int(steps)):
            self._launch(False)
            calc.calculate(self._work)
            if (k + 1) % self.check_every == 0:
                self._check()
        self._launch(True)
        h = self._check()
        assert h["step"] == self.nsteps, (h, self.nsteps)
        self._drain()
        return st

    @property
    def positions(self):
        return None if self.state is None else self.state.r

    @property
    def velocities(self):
        return None if self.state is None else self.state.v

    @property
    def log(self) -> np.ndarray:
        B = self.state.B if self.state is not None else 0
        return np.concatenate(self._log) if self.state is not None and self._log else np.zeros((0, B, 8))

    @property
    def trajectory(self) -> np.ndarray:
        N = self.state.N if self.state is not None else 0
        return np.concatenate(self._frames) if self.state is not None and self._frames else np.zeros((0, N, 3))

    @property
    def trajectory_velocities(self) -> np.ndarray:
        N = self.state.N if self.state is not None else 0
        return np.concatenate(self._fvel) if self.state is not None and self._fvel else np.zeros((0, N, 3))


# ---- geometry files (standard library only) -----------------------------------------------------------------------------------------------
def read_xyz(path: str):
    """-> list of (z int64 [n], positions float64 [n, 3]), one per frame of an .xyz / .extxyz file (species, then x y z; further columns are ignored)."""
    number = {s: i for i, s in enumerate(SYMBOLS)}
    out = []
    with open(path) as fh:
        lines = fh.read().splitlines()
    i = 0
    while i < len(lines):
        if not lines[i].strip():
            i += 1
            continue
        n = int(lines[i].split()[0])
        z, pos = [], []
        for ln in lines[i + 2:i + 2 + n]:
            tok = ln.split()
            if tok[0].isdigit():
                z.append(int(tok[0]))
            elif tok[0].capitalize() in number:
                z.append(number[tok[0].capitalize()])
            else:
                raise ValueError(f"{path}: unknown element {tok[0]!r} (the symbol table covers Z=1..{len(SYMBOLS) - 1}; atomic numbers are accepted)")
            pos.append([float(t) for t in tok[1:4]])
        if len(z) != n:
            raise ValueError(f"{path}: a frame announces {n} atoms and holds {len(z)}")
        out.append((np.asarray(z, dtype=np.int64), np.asarray(pos, dtype=np.float64).reshape(-1, 3)))
        i += 2 + n
    if not out:
        raise ValueError(f"{path}: no frame")
    return out


def write_xyz(path: str, z, ptr, pos, file_format: str = "xyz", append: bool = False, energies=None, forces=None):
    """One frame per molecule.  ``xyz``: symbol x y z; ``extxyz``: a Properties comment line (energy, pbc="F F F") and force columns when given."""
    if file_format not in ("xyz", "extxyz"):
        raise ValueError(f"file_format={file_format!r}: xyz or extxyz")
    with open(path, "a" if append else "w") as fh:
        for b in range(len(ptr) - 1):
            a, e = int(ptr[b]), int(ptr[b + 1])
            fh.write(f"{e - a}\n")
            if file_format == "extxyz":
                props = "species:S:1:pos:R:3" + (":forces:R:3" if forces is not None else "")
                fh.write(f'Properties={props}' + (f" energy={float(energies[b]):.10f}" if energies is not None else "") + ' pbc="F F F"\n')
            else:
                fh.write((f"energy={float(energies[b]):.10f}" if energies is not None else "") + "\n")
            for i in range(a, e):
                zi = int(z[i])
                sym = SYMBOLS[zi] if 0 < zi < len(SYMBOLS) else str(zi)
                line = f"{sym:<2s} {pos[i, 0]:20.12f} {pos[i, 1]:20.12f} {pos[i, 2]:20.12f}"
                if file_format == "extxyz" and forces is not None:
                    line += f" {forces[i, 0]:18.10e} {forces[i, 1]:18.10e} {forces[i, 2]:18.10e}"
                fh.write(line + "\n")


# ---- the reference's interface class ----------------------------------------------------------------------------------------------------
class PYGAseInterface:
    """nablaDFT/optimization/pyg_ase_interface.py:119-335 without ase, batched: same constructor keywords (:136-150) and method names.

    ``molecule_path``: an ``.xyz`` / ``.extxyz`` file (every frame is one molecule of the batch; the reference reads one molecule) or an ASE-sqlite energy
    database (every row is one molecule, ``read_energy_database``).  ``config`` is kept for signature parity and not read (the reference stores it on its
    calculator).  ``optimizer_class`` is accepted and ignored: ``optimize`` runs the device L-BFGS (``ASEBatchwiseLBFGS``), the reference ase's QuasiNewton.
    ``fixed_atoms``: indices inside a molecule, applied to every molecule of the batch (:159-162).  Units other than Hartree / Angstrom raise.
    ``init_md`` / ``run_md`` (:207-294) write ``<name>.log`` in MDLogger's column layout (Time[ps] Etot Epot Ekin [Hartree] T[K]; one block per molecule, mode
    "a"), ``<name>.npz`` (``positions`` [frames, N, 3], ``ptr``, ``z``, ``steps``) and ``<name>.extxyz`` (last frame); ase's binary ``.traj`` is not written.
    Steps are counted from the first ``init_md`` on; Time[ps] is the step number times the current ``time_step``.  A step both runs would sample (the last of
    one run, the first of the next) is written once, by the earlier run.
    ``compute_normal_modes`` (:317-334) runs ``vibrations.BatchedVibrations`` (on a device that is not a GPU it raises NotImplementedError: no CPU path)."""

    def __init__(self, molecule_path: str, working_dir: str, config, model, energy_key: str = "energy", force_key: str = "forces",
                 energy_unit: Union[str, float] = "Hartree", position_unit: Union[str, float] = "Angstrom", device: Union[str, torch.device] = "cpu",
                 dtype: torch.dtype = torch.float32, optimizer_class: Optional[type] = None, fixed_atoms: Optional[List[int]] = None, seed: int = 0,
                 friction: float = 0.01, frame_capacity: int = 64, check_every: int = 50):
        self.working_dir = working_dir
        os.makedirs(working_dir, exist_ok=True)
        self.config, self.optimizer_class = config, optimizer_class          # optimizer_class: accepted and ignored (see optimize)
        self.calculator = PyGBatchwiseCalculator(model, device, energy_key, force_key, energy_unit, position_unit, dtype)      # raises for other units
        self.device = self.calculator.device
        if str(molecule_path).endswith((".xyz", ".extxyz")):
            mols = read_xyz(molecule_path)
            z, pos = [m[0] for m in mols], [m[1] for m in mols]
        else:
            from .data import read_energy_database
            arena = read_energy_database(molecule_path)
            p = arena.ptr.numpy()
            z = [arena.z[a:b].numpy().astype(np.int64) for a, b in zip(p[:-1], p[1:])]
            pos = [arena.pos[a:b].numpy().astype(np.float64) for a, b in zip(p[:-1], p[1:])]
        sizes = np.array([len(a) for a in z])
        self.ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.z, self.positions = np.concatenate(z), np.concatenate(pos)
        self.velocities = None
        self.fixed_mask = None
        if fixed_atoms:
            self.fixed_mask = np.zeros(len(self.z), dtype=bool)
            for a, n in zip(self.ptr[:-1], sizes):
                idx = np.asarray(fixed_atoms, dtype=np.int64)
                if (idx >= n).any() or (idx < -n).any():
                    raise IndexError(f"fixed_atoms {fixed_atoms} outside a molecule of {n} atoms")
                self.fixed_mask[a + idx % n] = True
        self.seed, self.friction, self.frame_capacity, self.check_every = seed, friction, frame_capacity, check_every
        self.energy = self.forces = None
        self.dynamics = None
        self._md_name = None

    def _batch(self) -> Batch:
        dev = self.device
        B = len(self.ptr) - 1
        return Batch(torch.from_numpy(self.positions).to(dev), torch.from_numpy(self.z).to(dev), torch.from_numpy(np.repeat(np.arange(B), np.diff(self.ptr))).to(dev),
                     None, None, torch.from_numpy(self.ptr).to(dev))

    def save_molecule(self, name: str, file_format: str = "xyz", append: bool = False):
        write_xyz(os.path.join(self.working_dir, f"{name:s}.{file_format:s}"), self.z, self.ptr, self.positions, file_format, append, self.energy, self.forces)

    def calculate_single_point(self):
        b = self._batch()
        self.calculator.calculate(Batch(b.pos.float(), b.z, b.batch, ptr=b.ptr))
        self.energy = self.calculator.energy.double().cpu().numpy()
        self.forces = self.calculator.forces.double().cpu().numpy()
        self.save_molecule("single_point", file_format="xyz")

    def init_md(self, name: str, time_step: float = 0.5, temp_init: float = 300, temp_bath: Optional[float] = None, reset: bool = False, interval: int = 1):
        fresh = self.dynamics is None
        if fresh:
            self.dynamics = BatchedMD(self.calculator, time_step, temp_bath, self.friction, self.fixed_mask, None, self.seed, interval, self.frame_capacity,
                                      check_every=self.check_every)
        md = self.dynamics
        md.time_step, md.temp_bath, md.interval = time_step, temp_bath, int(interval)
        # a previous dynamics run keeps its velocities unless reset is asked for (:232-235)
        if fresh or reset:
            self._init_velocities(temp_init=temp_init)
        self._md_name = name
        self._md_frames_from = md.trajectory.shape[0]
        self._md_rows_from = md.log.shape[0]

    def _init_velocities(self, temp_init: float = 300, remove_translation: bool = True, remove_rotation: bool = True):
        self.dynamics.init_velocities(self._batch(), temp_init, remove_translation, remove_rotation)

    def run_md(self, steps: int):
        if not self.dynamics:
            raise AttributeError("no dynamics yet: call init_md(name, ...) before run_md")
        md, name = self.dynamics, self._md_name
        rows_before = md.log.shape[0]
        md.run(self._batch(), steps)
        self.positions = md.positions.cpu().numpy()
        self.velocities = md.velocities.cpu().numpy()
        self.energy = self.calculator.energy.double().cpu().numpy()
        self.forces = self.calculator.forces.double().cpu().numpy()
        log = md.log[rows_before:]
        with open(os.path.join(self.working_dir, f"{name:s}.log"), "a") as fh:
            for b in range(len(self.ptr) - 1):
                fh.write(f"# molecule {b}\n")
                fh.write("%-10s %16s %16s %16s  %8s\n" % ("Time[ps]", "Etot[Hartree]", "Epot[Hartree]", "Ekin[Hartree]", "T[K]"))
                for row in log[:, b]:
                    fh.write("%-10.4f %16.8f %16.8f %16.8f  %8.2f\n" % (row[0] * md.time_step / 1000.0, row[1], row[2], row[3], row[4]))
        np.savez(os.path.join(self.working_dir, f"{name:s}.npz"), positions=md.trajectory[self._md_frames_from:], ptr=self.ptr, z=self.z,
                 steps=md.log[self._md_rows_from:, 0, 0].astype(np.int64))
        self.save_molecule(name, file_format="extxyz")

    def optimize(self, fmax: float = 1.0e-2, steps: int = 1000):
        """Device L-BFGS (optimization.py) instead of ase's QuasiNewton (BFGS + line search): another optimiser, the same stopping rule (max |f| < fmax)."""
        opt = ASEBatchwiseLBFGS(self.calculator, logfile=None, fixed_atoms_mask=self.fixed_mask)
        converged = opt.run(self._batch(), fmax=fmax, steps=steps)
        self.positions = opt.positions.cpu().numpy()
        self.energy = self.calculator.energy.double().cpu().numpy()
        self.forces = self.calculator.forces.double().cpu().numpy()
        self.dynamics = None            # the MD state belonged to the old geometry
        self.save_molecule("optimization", file_format="extxyz")
        return converged

    def compute_normal_modes(self, write_jmol: bool = True):
        """Normal modes at ``self.positions`` with the interface's fixed atoms (vibrations.py: batched finite-difference Hessians and the device eigensolver
        instead of ase.vibrations).  Writes ``normal_modes.npz``, ``normal_modes.txt`` (ase's summary layout, one block per molecule) and, when ``write_jmol``,
        ``normal_modes.xyz`` (one frame per mode) into ``working_dir``; the driver stays in ``self.vibrations``."""
        if self.device.type != "cuda":
            raise NotImplementedError("compute_normal_modes runs on MI355X only (no CPU path): construct the interface with device='cuda'")
        from .vibrations import BatchedVibrations, write_normal_modes
        vib = self.vibrations = BatchedVibrations(self.calculator, fixed_atoms_mask=self.fixed_mask)
        vib.run(self._batch())
        write_normal_modes(self.working_dir, vib, self.z, self.ptr, self.positions, write_jmol)


__all__ = ["BatchedMD", "MDState", "PYGAseInterface", "KAPPA", "KB", "masses_for", "read_xyz", "write_xyz"]
