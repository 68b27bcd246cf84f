"""Batched normal modes with everything on the GPU: finite-difference Hessians of hundreds or thousands of molecules per model call and a batched symmetric
eigensolver (csrc/vib.hip, ``nq_vib_*`` of include/nablaq.h).

Mirrors what ``PYGAseInterface.compute_normal_modes`` (nablaDFT/optimization/pyg_ase_interface.py:317-334) asks of ``ase.vibrations.Vibrations``.  Parity
status: **restated, unpinned** -- ase is neither in the reference tree nor a dependency here, so the arithmetic below is a restatement of
``Vibrations(atoms, delta=0.01, nfree=2)`` from memory; the kernels are tested against a float64 numpy restatement of the same equations (tests/vib_ref.py)
and against ``numpy.linalg.eigh``, not against ase.

Arithmetic (Hartree, Angstrom, amu; everything float64 but the positions the model reads):
  for every free atom a of a molecule, axis d, and each sign: forces F-+ at x0 -+ delta e_{a,d};
  G[3a+d, :] = (F- - F+)[free].ravel() / h;   H = (G + G^T) / 2   (ase: rows / (4 delta), then H += H^T);   A = im[:, None] H im,  im = repeat(m^-1/2, 3);
  omega^2, U = eigh(A);  h nu = hbar sqrt(omega^2) as a complex number;  modes = rows of U^T scaled by m^-1/2;  frequencies = h nu / (h c) in cm^-1;
  zero-point energy = 1/2 sum Re h nu.
Units: CODATA 2014 (the set ase 3.22.1 uses); omega^2 = 1 Hartree Angstrom^-2 amu^-1 is 2720.2 cm^-1 (``CM1_PER_SQRT_UNIT``).

Two deliberate departures from ase:
  1. Realised step.  The models read float32 positions, so float32(x0 +- delta) is not x0 +- delta.  The quotient divides by the step actually applied,
     h = (double) x32+ - (double) x32-, not by 2 delta: on an exactly quadratic model the Hessian error drops from 2e-5 to 1e-15 of the largest entry.
  2. Fixed atoms are left out of ``indices``: the result is the partial Hessian of the free atoms (ase would displace them too and halve their couplings).

Eigensolver: one 256-thread workgroup per molecule, parallel cyclic Jacobi with a round-robin ordering; the matrix lives in LDS up to 3 n_free = 141, above
that in global memory.  It does not depend on what eigensolver the torch build links.

Limits (each raises, nothing degrades silently): ``nfree=2`` only; Hartree / Angstrom only; at most ``MAX_DOF`` = 576 free degrees of freedom per molecule
(192 free atoms); no infrared intensities, no projection of translations and rotations, no thermochemistry; ase's cache directory is not written.
"""
import ctypes as C
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._devstate import DeviceState, batch_ptr_host, fixed_to_uint8, require_forces, require_positions
from .md import AMU_SI, E_H_SI, SYMBOLS, masses_for
from .trainer import Batch

# ---- units (CODATA 2014, beside E_H_SI / AMU_SI of md.py) -------------------------------------------------------------------------------------------
HBAR_SI = 1.054571800e-34     # J s
C_SI = 299792458.0            # m / s
E_SI = 1.6021766208e-19       # C
# omega [rad/s] = sqrt(omega^2 [Hartree / (Angstrom^2 amu)]) * RAD_S_PER_SQRT_UNIT
RAD_S_PER_SQRT_UNIT = math.sqrt(E_H_SI / (AMU_SI * (1e-10 * 1e-10)))
HARTREE_PER_SQRT_UNIT = HBAR_SI * RAD_S_PER_SQRT_UNIT / E_H_SI                  # h nu [Hartree] of sqrt(omega^2) = 1
CM1_PER_SQRT_UNIT = RAD_S_PER_SQRT_UNIT / (2.0 * math.pi * C_SI * 100.0)        # ~ 2720.2 cm^-1
HARTREE_TO_EV = E_H_SI / E_SI

MAX_DOF = 576                 # 3 n_free per molecule; AT it the one-workgroup global-memory eigensolver takes 4 s per molecule (profiles/vib_step.json)
LDS_MAX_DOF = 141             # the matrix and the rotation parameters fit one workgroup's 160 KiB of LDS


def plan(ptr, fixed=None):
    """Host plan of a batch: dict of ``n`` [B] atoms, ``m`` [B] free degrees of freedom, ``dof_ptr`` / ``hess_ptr`` [B+1], ``free_atom`` [D/3], ``disp_mol`` [D],
    ``disp_off`` [D+1] (image atoms before each displacement), ``D``, ``P``."""
    ptr = np.asarray(ptr, dtype=np.int64)
    N, B = int(ptr[-1]), ptr.shape[0] - 1
    free = np.ones(N, dtype=bool) if fixed is None else fixed_to_uint8(fixed, N) == 0
    n = np.diff(ptr)
    mol = np.repeat(np.arange(B), n)
    nf = np.bincount(mol[free], minlength=B)
    m = 3 * nf
    dof_ptr = np.concatenate([[0], np.cumsum(m)])
    hess_ptr = np.concatenate([[0], np.cumsum(m * m)])
    disp_mol = np.repeat(np.arange(B), m)
    disp_off = np.concatenate([[0], np.cumsum(2 * n[disp_mol])])
    return dict(n=n, m=m, dof_ptr=dof_ptr, hess_ptr=hess_ptr, free_atom=np.nonzero(free)[0], free=free, disp_mol=disp_mol, disp_off=disp_off,
                D=int(dof_ptr[-1]), P=int(hess_ptr[-1]), N=N, B=B, ptr=ptr)


def chunks(pl, images_per_call: int):
    """[(c0, c1)] over the displacement list: at most ``images_per_call`` images (two per displacement, a pair is never split) per chunk."""
    per = max(1, int(images_per_call) // 2)
    return [(c0, min(c0 + per, pl["D"])) for c0 in range(0, pl["D"], per)]


# ---- device state -----------------------------------------------------------------------------------------------------------------------
class VibState(DeviceState):
    """One caller-owned device buffer behind ``nq_vib_*`` plus typed views of its parts (include/nablaq.h)."""

    def __init__(self, ptr_host: Sequence[int], pos: torch.Tensor, masses, fixed=None):
        require_positions(pos, "vibrations")
        ptr32 = np.ascontiguousarray(np.asarray(ptr_host, dtype=np.int32))
        self.plan = pl = plan(ptr32, fixed)
        self.B, self.N, self.D, self.P = pl["B"], int(pos.shape[0]), pl["D"], pl["P"]
        if int(pl["m"].max()) > MAX_DOF:
            b = int(pl["m"].argmax())
            raise _lib.NablaqError(_lib.NQ_ERR_MOL_TOO_LARGE, f"molecule {b} has {int(pl['m'][b])} free degrees of freedom, the limit is {MAX_DOF}")
        masses = np.ascontiguousarray(np.asarray(masses, dtype=np.float64).reshape(-1))
        if masses.shape[0] != self.N:
            raise ValueError(f"masses has {masses.shape[0]} entries for {self.N} atoms")
        fixed_host = np.ascontiguousarray((~pl["free"]).astype(np.uint8)) if fixed is not None else None
        N, B, D, P, i32, i64, f64 = self.N, self.B, self.D, self.P, torch.int32, torch.int64, torch.float64
        nbytes = self._allocate("vib", (N, B, D, P), (
            ("header_dev", i32, (16,)), ("mol_ptr", i32, (B + 1,)), ("dof_ptr", i32, (B + 1,)), ("hess_ptr", i64, (B + 1,)), ("order", i32, (B,)),
            ("free_atom", i32, (D // 3,)), ("disp_mol", i32, (D,)), ("disp_off", i64, (D + 1,)), ("im", f64, (D,)), ("r", f64, (N, 3)), ("h", f64, (D,)),
            ("asymmetry", f64, (B,)), ("sweeps", i32, (B,)), ("status", i32, (B,)), ("omega2", f64, (D,)), ("work", f64, (P,)), ("hessian", f64, (P,)),
            ("modes", f64, (P,))), pos.device)
        pos = pos.contiguous()
        out = (C.c_int32 * 3)()
        hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.load().nq_vib_init(_lib.ptr(self.buf), nbytes, hp(ptr32), hp(masses), hp(fixed_host), *self._dims, _lib.ptr(pos),
                                           int(pos.dtype == torch.float64), out, _lib.stream_ptr()))
        self.n_lds, self.max_m_lds, self.max_m = out[0], out[1], out[2]
        self.masses_host = masses

    def image_atoms(self, c0: int, c1: int) -> int:
        return int(self.plan["disp_off"][c1] - self.plan["disp_off"][c0])

    def displace(self, c0: int, c1: int, delta: float, image_pos: torch.Tensor):
        """float32 positions of the 2 (c1 - c0) images of chunk [c0, c1) -> ``image_pos`` [image_atoms(c0, c1), 3]; records the realised steps ``h[c0:c1]``."""
        if not (0 <= c0 < c1 <= self.D):
            raise ValueError(f"chunk [{c0}, {c1}) outside the {self.D} displacements")
        n = self.image_atoms(c0, c1)
        if image_pos.dtype != torch.float32 or tuple(image_pos.shape) != (n, 3) or image_pos.device != self.buf.device or not image_pos.is_contiguous():
            raise ValueError(f"image_pos must be a contiguous float32 [{n}, 3] tensor on {self.buf.device}")
        _lib.check(_lib.load().nq_vib_displace(_lib.ptr(self.buf), *self._dims, int(c0), int(c1), float(delta), _lib.ptr(image_pos), n, _lib.stream_ptr()))
        torch.autograd.graph.increment_version(image_pos)      # written through a raw pointer: a batch prepared for the previous images is refused

    def accumulate(self, c0: int, c1: int, forces: torch.Tensor):
        if not (0 <= c0 < c1 <= self.D):
            raise ValueError(f"chunk [{c0}, {c1}) outside the {self.D} displacements")
        n = self.image_atoms(c0, c1)
        forces = require_forces(forces, n, self.buf.device)
        _lib.check(_lib.load().nq_vib_accumulate(_lib.ptr(self.buf), *self._dims, int(c0), int(c1), _lib.ptr(forces), int(forces.dtype == torch.float64), n,
                                                 _lib.stream_ptr()))

    def finish(self):
        _lib.check(_lib.load().nq_vib_finish(_lib.ptr(self.buf), *self._dims, _lib.stream_ptr()))

    def eigh(self, scale_modes: bool = True):
        """Eigen-decomposition of every molecule's matrix in ``work`` (overwritten) -> ``omega2``, ``modes``, ``sweeps``, ``status``."""
        _lib.check(_lib.load().nq_vib_eigh(_lib.ptr(self.buf), *self._dims, self.n_lds, self.max_m_lds, self.max_m, int(scale_modes), _lib.stream_ptr()))

    def header(self) -> dict:
        """The header words (one small device->host copy, synchronises the stream)."""
        h = self._read_header()
        if h[5] == -2:
            raise RuntimeError("an nq_vib call came with other dimensions than nq_vib_init prepared the state for")
        if h[5] == -3:
            raise RuntimeError("an nq_vib chunk came with an image tensor of another size than the plan")
        return dict(N=h[0], B=h[1], D=h[2], P=h[3] + (h[4] << 32), status=h[5], n_lds=h[6])


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
class BatchedVibrations:
    """Normal modes of every molecule of a batch, driven by a ``PyGBatchwiseCalculator`` (any of the engines, or a callable ``Batch -> (energy, forces)``).

    ``run(batch)``: for each chunk of at most ``images_per_call`` images one displace launch, one model call on the images and one accumulate launch; then the
    finish launch and the eigensolver.  Between the first and the last model call this class copies nothing to the host and never synchronises: the images'
    ``z`` / ``batch`` / ``ptr`` tensors are built on the device from a plan computed once on the host.  ``images_per_call``: 2048 by default -- measured with
    PaiNN-OC on 2048 molecules (profiles/vib_step.json): 512 / 1024 / 2048 / 4096 images per call take 5.09 / 4.46 / 4.14 / 3.98 s at 22 / 22 / 40 / 76 GB
    peak memory (the engine's workspace grows with the call); 2048 is within 5 % of the fastest at half its memory.
    Results stay on the device (float64): ``hessian`` (packed, molecule b at ``hess_ptr[b]``, m_b x m_b), ``omega2`` and ``modes`` (row k of a molecule's
    block = mode k, ascending omega2, scaled by m^-1/2), ``asymmetry`` [B] (max |G - G^T|, the noise of the finite differences), ``sweeps`` and ``status`` [B].
    Host properties: ``energies`` (complex128 [D], Hartree, imaginary for omega2 < 0), ``frequencies`` (cm^-1), ``zero_point_energy`` (float64 [B], Hartree);
    ``dof_ptr`` splits them per molecule.  Departures from ase (module docstring): the realised float32 step divides the difference; fixed atoms are not displaced."""

    def __init__(self, calculator, delta: float = 0.01, fixed_atoms_mask=None, masses=None, images_per_call: int = 2048, nfree: int = 2):
        if nfree != 2:
            raise NotImplementedError(f"nfree={nfree}: only the two-point central difference (nfree=2) is built")
        if not (delta > 0.0):
            raise ValueError(f"delta={delta} must be positive")
        if images_per_call < 2:
            raise ValueError("images_per_call must hold at least one +- pair")
        units = getattr(calculator, "property_units", None)
        if units is not None and any(v != 1.0 for v in units.values()):
            raise NotImplementedError("only Hartree / Angstrom are built")
        self.calculator, self.delta, self.fixed_atoms_mask, self.masses, self.images_per_call = calculator, float(delta), fixed_atoms_mask, masses, int(images_per_call)
        self.state = None

    def prepare(self, batch) -> VibState:
        """The state, the chunk list and the device-side plan of the image batches (the only host-side planning of a run)."""
        st = self.state = VibState(batch_ptr_host(batch), batch.pos, masses_for(batch.z, self.masses), self.fixed_atoms_mask)
        pl, dev = st.plan, batch.pos.device
        self.todo = chunks(pl, self.images_per_call)
        cap = max([st.image_atoms(c0, c1) for c0, c1 in self.todo] or [0])
        self._image_pos = torch.empty(cap, 3, dtype=torch.float32, device=dev)
        self._n_dev = torch.from_numpy(pl["n"]).to(dev)
        self._start_dev = torch.from_numpy(pl["ptr"][:-1].copy()).to(dev)
        self._z = batch.z
        return st

    def image_batch(self, c0: int, c1: int) -> Batch:
        """The model's input for chunk [c0, c1): ``z`` / ``batch`` / ``ptr`` built on the device (no read of the device, no wait); ``pos`` is the slice of the
        image tensor that ``displace`` fills."""
        st, dev = self.state, self._image_pos.device
        natoms, nimg = st.image_atoms(c0, c1), 2 * (c1 - c0)
        mol = st.disp_mol[c0:c1].long().repeat_interleave(2, output_size=nimg)
        sizes = self._n_dev[mol]
        iptr = torch.zeros(nimg + 1, dtype=torch.int64, device=dev)
        iptr[1:] = torch.cumsum(sizes, 0)
        ibatch = torch.repeat_interleave(torch.arange(nimg, device=dev), sizes, output_size=natoms)
        iz = self._z[self._start_dev[mol][ibatch] + torch.arange(natoms, device=dev) - iptr[ibatch]]
        return Batch(self._image_pos[:natoms], iz, ibatch, None, None, iptr)

    def run(self, batch) -> VibState:
        st, calc = self.prepare(batch), self.calculator
        for c0, c1 in self.todo:      # nothing in this loop reads the device or waits for it
            images = self.image_batch(c0, c1)
            st.displace(c0, c1, self.delta, images.pos)
            calc.calculate(images)
            st.accumulate(c0, c1, calc.forces)
        st.finish()
        st.eigh(True)
        st.header()          # the first read of the device: raises if a launch was refused
        return st

    # device results
    hessian = property(lambda self: self.state.hessian)
    omega2 = property(lambda self: self.state.omega2)
    modes = property(lambda self: self.state.modes)
    asymmetry = property(lambda self: self.state.asymmetry)
    sweeps = property(lambda self: self.state.sweeps)
    status = property(lambda self: self.state.status)
    hess_ptr = property(lambda self: self.state.plan["hess_ptr"])
    dof_ptr = property(lambda self: self.state.plan["dof_ptr"])

    @property
    def energies(self) -> np.ndarray:
        return energies_from_omega2(self.state.omega2.cpu().numpy())

    @property
    def frequencies(self) -> np.ndarray:
        return frequencies_from_omega2(self.state.omega2.cpu().numpy())

    @property
    def zero_point_energy(self) -> np.ndarray:
        return zero_point_energy(self.energies, self.dof_ptr)


def energies_from_omega2(omega2) -> np.ndarray:
    """h nu in Hartree, complex128: imaginary where omega2 < 0."""
    return HARTREE_PER_SQRT_UNIT * np.sqrt(np.asarray(omega2, dtype=np.float64).astype(np.complex128))


def frequencies_from_omega2(omega2) -> np.ndarray:
    """cm^-1, complex128."""
    return CM1_PER_SQRT_UNIT * np.sqrt(np.asarray(omega2, dtype=np.float64).astype(np.complex128))


def zero_point_energy(energies, dof_ptr) -> np.ndarray:
    """float64 [B], Hartree: 1/2 sum Re h nu per molecule."""
    e = np.asarray(energies).real
    return np.array([0.5 * e[a:b].sum() for a, b in zip(dof_ptr[:-1], dof_ptr[1:])], dtype=np.float64)


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def write_summary(path: str, energies, dof_ptr):
    """One block per molecule in the layout of ase's ``Vibrations.summary``: ``#  meV  cm^-1`` rows, ``i`` marks an imaginary mode, then the zero-point energy."""
    energies = np.asarray(energies, dtype=np.complex128)
    zpe = zero_point_energy(energies, dof_ptr)
    to_cm = CM1_PER_SQRT_UNIT / HARTREE_PER_SQRT_UNIT
    with open(path, "w") as fh:
        for b, (a, e) in enumerate(zip(dof_ptr[:-1], dof_ptr[1:])):
            fh.write(f"# molecule {b}\n")
            fh.write("---------------------\n  #    meV     cm^-1\n---------------------\n")
            for k, en in enumerate(energies[a:e]):
                c, v = ("i", en.imag) if en.imag != 0 else (" ", en.real)
                fh.write("%3d %6.1f%s  %7.1f%s\n" % (k, 1000.0 * HARTREE_TO_EV * v, c, to_cm * v, c))
            fh.write("---------------------\n")
            fh.write("Zero-point energy: %.3f eV\n" % (HARTREE_TO_EV * zpe[b]))


def read_summary(path: str):
    """-> list per molecule of (energies complex128 [m] in meV, frequencies complex128 [m] in cm^-1, zero-point energy in eV)."""
    out, rows = [], None
    with open(path) as fh:
        for ln in fh:
            tok = ln.split()
            if ln.startswith("# molecule"):
                rows = []
            elif ln.startswith("Zero-point energy"):
                mev = np.array([r[0] for r in rows], dtype=np.complex128)
                cm = np.array([r[1] for r in rows], dtype=np.complex128)
                out.append((mev, cm, float(tok[2])))
            elif len(tok) == 3 and tok[0].isdigit():
                val = lambda t: complex(0.0, float(t[:-1])) if t.endswith("i") else complex(float(t), 0.0)
                rows.append((val(tok[1]), val(tok[2])))
    return out


def write_jmol(path: str, z, ptr, pos, frequencies, modes, dof_ptr, hess_ptr, free):
    """One frame per mode, as ase's ``Vibrations.write_jmol``: atom count, ``Mode #k, f = ... cm^-1.``, then symbol, position, displacement (zero for fixed atoms)."""
    frequencies = np.asarray(frequencies, dtype=np.complex128)
    with open(path, "w") as fh:
        for b in range(len(ptr) - 1):
            a, e = int(ptr[b]), int(ptr[b + 1])
            m = int(dof_ptr[b + 1] - dof_ptr[b])
            block = np.asarray(modes[int(hess_ptr[b]):int(hess_ptr[b + 1])]).reshape(m, m)
            idx = np.nonzero(free[a:e])[0]
            for k in range(m):
                f = frequencies[dof_ptr[b] + k]
                c, v = ("i", f.imag) if f.imag != 0 else (" ", f.real)
                fh.write("%6d\n" % (e - a))
                fh.write("Mode #%d, f = %.1f%s cm^-1.\n" % (k, v, c))
                disp = np.zeros((e - a, 3))
                disp[idx] = block[k].reshape(-1, 3)
                for i in range(e - a):
                    zi = int(z[a + i])
                    sym = SYMBOLS[zi] if 0 < zi < len(SYMBOLS) else str(zi)
                    fh.write("%2s %12.5f %12.5f %12.5f %12.5f %12.5f %12.5f\n" % (sym, pos[a + i, 0], pos[a + i, 1], pos[a + i, 2], disp[i, 0], disp[i, 1], disp[i, 2]))


def write_normal_modes(working_dir: str, vib: BatchedVibrations, z, ptr, pos, write_jmol_file: bool = True):
    """``normal_modes.npz`` (every result array plus ``ptr`` and ``z``), ``normal_modes.txt`` (summary) and, if asked, ``normal_modes.xyz`` (one frame per mode)."""
    st = vib.state
    arrays = dict(hessian=st.hessian.cpu().numpy(), hess_ptr=np.asarray(vib.hess_ptr), dof_ptr=np.asarray(vib.dof_ptr), omega2=st.omega2.cpu().numpy(),
                  modes=st.modes.cpu().numpy(), asymmetry=st.asymmetry.cpu().numpy(), sweeps=st.sweeps.cpu().numpy(), status=st.status.cpu().numpy())
    energies = energies_from_omega2(arrays["omega2"])
    freqs = frequencies_from_omega2(arrays["omega2"])
    np.savez(os.path.join(working_dir, "normal_modes.npz"), energies=energies, frequencies=freqs, zero_point_energy=zero_point_energy(energies, vib.dof_ptr),
             ptr=np.asarray(ptr), z=np.asarray(z), **arrays)
    write_summary(os.path.join(working_dir, "normal_modes.txt"), energies, vib.dof_ptr)
    if write_jmol_file:
        write_jmol(os.path.join(working_dir, "normal_modes.xyz"), z, ptr, pos, freqs, arrays["modes"], vib.dof_ptr, vib.hess_ptr, st.plan["free"])
    return arrays


__all__ = ["BatchedVibrations", "VibState", "MAX_DOF", "LDS_MAX_DOF", "HBAR_SI", "C_SI", "E_SI", "CM1_PER_SQRT_UNIT", "HARTREE_PER_SQRT_UNIT", "HARTREE_TO_EV",
           "plan", "chunks", "energies_from_omega2", "frequencies_from_omega2", "zero_point_energy", "write_summary", "read_summary", "write_jmol",
           "write_normal_modes"]
