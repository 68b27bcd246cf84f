"""The ``optimize`` job (config/gemnet-oc_optim.yaml, config/schnet_optim.yaml): batched L-BFGS geometry optimisation with the whole optimiser state on the GPU.

Mirrors of the three classes the job instantiates:
  nabladft_amd.optimization.ASEBatchwiseLBFGS       <-> nablaDFT.optimization.ASEBatchwiseLBFGS       (optimization/optimizers.py:293-605)
  nabladft_amd.optimization.PyGBatchwiseCalculator  <-> nablaDFT.optimization.PyGBatchwiseCalculator  (optimization/calculator.py:98-132)
  nabladft_amd.optimization.BatchwiseOptimizeTask   <-> nablaDFT.optimization.BatchwiseOptimizeTask   (optimization/task.py:9-73)

The reference keeps positions, history and forces in numpy on the host: a Python loop over molecules, a dense [B, N] mask, ``np.add.at`` scatters, a rebuilt
``ase.Atoms`` list and a device->host / host->device copy pair every step.  Here a step is ONE kernel launch (``nq_lbfgs_step``, csrc/lbfgs.hip): master
positions (float64), the (s, y, rho) ring, previous positions / forces, per-molecule converged flags and the iteration counter live in one device buffer, and
the kernel writes the float32 positions the model reads next.  The host only reads a 64-byte header every ``check_every`` steps.

Limits (each raises, nothing degrades silently): no line search (``use_line_search=True``: no nablaDFT config selects it), no ``restart`` / ``trajectory``
files, Hartree / Angstrom units only (the conversion table lives in schnetpack), molecules of at most 512 atoms, history depth at most 1024.

Arithmetic: everything the optimiser does is float64, forces are taken as float32 or float64.  With the PyG calculator the reference carries q / z of the
two-loop recursion in float32 (numpy keeps the dtype of the model output); float64 here is at least as accurate -- this is a statement about precision, not a
claim of bitwise parity with that path.
"""
import ctypes as C
import json
import os
import sqlite3
import struct
import sys
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._devstate import DeviceState, batch_ptr_host, fixed_to_uint8, require_forces, require_positions
from .data import _decode_ase_blob
from .trainer import Batch

_UNITS_ONE = {"hartree": 1.0, "ha": 1.0, "ang": 1.0, "angstrom": 1.0}
_HDR = ("iteration", "unconverged", "latch", "normalizations", "N", "B", "memory", "n_small")


# ---- device state -----------------------------------------------------------------------------------------------------------------------
class LBFGSState(DeviceState):
    """One caller-owned device buffer behind ``nq_lbfgs_init`` / ``nq_lbfgs_step`` plus typed views of its parts (include/nablaq.h, ABI 17)."""

    def __init__(self, ptr_host: Sequence[int], pos: torch.Tensor, memory: int):
        require_positions(pos, "optimization")
        ptr_host = np.ascontiguousarray(np.asarray(ptr_host, dtype=np.int32))
        self.B, self.N, self.memory = int(ptr_host.shape[0]) - 1, int(pos.shape[0]), int(memory)
        self.ptr_host = ptr_host
        N, B, m, i32, f64 = self.N, self.B, self.memory, torch.int32, torch.float64
        nbytes = self._allocate("lbfgs", (N, B, m), (
            ("header_dev", i32, (16,)), (None, i32, (B + 1,)), (None, i32, (B,)), ("converged_dev", i32, (B,)), ("rho", f64, (m, B)), ("r", f64, (N, 3)),
            ("r0", f64, (N, 3)), ("f0", f64, (N, 3)), ("S", f64, (m, N, 3)), ("Y", f64, (m, N, 3))), pos.device)
        self.pos32 = torch.empty(self.N, 3, dtype=torch.float32, device=pos.device)      # what the model reads; written by the step kernel
        pos = pos.contiguous()
        n_small = C.c_int32(0)
        _lib.check(_lib.load().nq_lbfgs_init(_lib.ptr(self.buf), nbytes, ptr_host.ctypes.data_as(C.c_void_p), *self._dims, _lib.ptr(pos),
                                             int(pos.dtype == torch.float64), _lib.ptr(self.pos32), C.byref(n_small), _lib.stream_ptr()))
        self.n_small = n_small.value

    def step(self, forces: torch.Tensor, fmax: float, maxstep: float, damping: float, alpha: float, fixed: Optional[torch.Tensor] = None,
             evaluate_only: bool = False):
        forces = require_forces(forces, self.N, self.buf.device)
        _lib.check(_lib.load().nq_lbfgs_step(_lib.ptr(self.buf), self.N, self.B, self.memory, self.n_small, _lib.ptr(forces), int(forces.dtype == torch.float64),
                                             _lib.ptr(fixed), _lib.ptr(self.pos32), float(fmax), float(maxstep), float(damping), float(alpha),
                                             int(evaluate_only), _lib.stream_ptr()))
        # the kernel wrote pos32 through a raw pointer: move its version counter, so that a prepared batch (net.prepare(data), _lib.geometry_key) built for
        # the previous geometry is refused instead of silently reused
        if not evaluate_only:
            torch.autograd.graph.increment_version(self.pos32)

    def header(self) -> dict:
        """The header words (one small device->host copy, synchronises the stream)."""
        h = self._read_header()
        if h[1] < 0:
            raise RuntimeError("nq_lbfgs_step was called with other dimensions than nq_lbfgs_init prepared the state for")
        return dict(zip(_HDR, h))


# ---- calculator -------------------------------------------------------------------------------------------------------------------------
class PyGBatchwiseCalculator:
    """optimization/calculator.py:98-132 for modules (or plain callables) that map a ``nabladft_amd.Batch`` to ``(energy, forces)`` device tensors: PaiNN,
    GemNet-OC, eSCN, EquiformerV2.  Results stay on the device (``energy``, ``forces``); ``results`` gives numpy copies on demand.  The model is called under
    ``torch.no_grad()`` (the engines return forces without an autograd graph).  Units: Hartree and Ang / Angstrom (factor 1, what
    config/calculator/pyg_calculator.yaml sets); anything else raises NotImplementedError -- the reference takes its table from schnetpack.units.
    ``data.prepared`` is never set on the batch handed to the model: the step kernel moves the atoms every call."""

    def __init__(self, model, device="cpu", energy_key: str = "energy", force_key: str = "forces", energy_unit: str = "eV", position_unit: str = "Ang",
                 dtype: torch.dtype = torch.float32):
        for what, unit in (("energy_unit", energy_unit), ("position_unit", position_unit)):
            if str(unit).lower() not in _UNITS_ONE:
                raise NotImplementedError(f"{what}={unit!r}: only Hartree / Ang(strom) are built (the reference converts with schnetpack.units.convert_units)")
        if dtype != torch.float32:
            raise NotImplementedError("the engines take float32 inputs (calculator.py:36 default)")
        self.device = torch.device(device) if isinstance(device, str) else device
        self.dtype, self.energy_key, self.force_key = dtype, energy_key, force_key
        self.property_units = {energy_key: 1.0, force_key: 1.0}
        self.model = model
        if isinstance(model, torch.nn.Module):
            model.to(self.device)
        self.energy = self.forces = None

    def calculate(self, batch: Batch) -> None:
        with torch.no_grad():
            out = self.model(batch)
        self.energy, self.forces = out[0].reshape(-1), out[1]

    @property
    def results(self):
        if self.forces is None:
            return None
        return {self.energy_key: self.energy.detach().cpu().numpy(), self.force_key: self.forces.detach().cpu().numpy()}


# ---- optimiser --------------------------------------------------------------------------------------------------------------------------
class ASEBatchwiseLBFGS:
    """optimization/optimizers.py:293-605 without the line search, same keyword surface and defaults (config/optimizer/batchwise_lbfgs.yaml instantiates it).

    ``run(batch, fmax=0.05, steps=None)`` follows BatchwiseDynamics.irun (optimizers.py:82-111): one model call on the start geometry, then step + model call
    until every atom of the batch is below fmax or ``steps`` steps were taken; returns the converged flag.  Afterwards: ``nsteps``, ``n_normalizations``,
    ``positions`` (float64 [N, 3], device), ``converged_mask`` (bool [B], device), ``calculator.energy / forces`` of the final geometry.
    ``check_every``: how often the host reads the unconverged count.  Once the whole batch is converged every molecule is masked and further steps do not
    move anything, and the kernel latches the first such iteration on the device: ``nsteps`` and the final positions do not depend on ``check_every``.
    ``steps=None`` keeps the reference's default bound (ase Dynamics: 100 000 000)."""

    defaults = {"maxstep": 0.2}

    def __init__(self, calculator, restart=None, logfile="-", trajectory=None, maxstep: Optional[float] = None, memory: int = 100, damping: float = 1.0,
                 alpha: float = 1.0, use_line_search: bool = False, master=None, log_every_step: bool = False, fixed_atoms_mask=None, verbose: bool = False,
                 check_every: int = 1):
        if use_line_search:
            raise NotImplementedError("use_line_search=True is not built (no nablaDFT config selects it)")
        if restart is not None or trajectory is not None:
            raise NotImplementedError("restart / trajectory files are not built")
        self.maxstep = self.defaults["maxstep"] if maxstep is None else maxstep
        if self.maxstep > 1.0:
            raise ValueError("You are using a much too large value for the maximum step size: %.1f Angstrom" % self.maxstep)
        if check_every < 1:
            raise ValueError("check_every must be >= 1")
        self.calculator, self.memory, self.damping, self.alpha = calculator, int(memory), damping, alpha
        self.H0 = 1.0 / alpha
        self.use_line_search, self.master, self.log_every_step, self.verbose = use_line_search, master, log_every_step, verbose
        self.fixed_atoms_mask, self.check_every = fixed_atoms_mask, int(check_every)
        self.logfile = logfile                      # "-": stdout; a path: opened for each record and closed again; a file object; None: silent
        self.max_steps = 100000000
        self.fmax = None
        self.initialize()

    def initialize(self):
        self.nsteps = 0
        self.n_normalizations = 0
        self.force_calls = self.function_calls = 0
        self.state = self.positions = self.converged_mask = None

    def _fixed(self, N, device):
        m = fixed_to_uint8(self.fixed_atoms_mask, N)                       # indices or a boolean mask, like f[fixed_atoms_mask] = 0 (calculator.py:86)
        return None if m is None else torch.from_numpy(m).to(device)

    def _log(self, forces):
        if self.logfile is None:
            return
        fmax = float(forces.double().pow(2).sum(1).max().sqrt())
        import time
        T = time.localtime()
        name = self.__class__.__name__
        msg = "%s  %4s %8s %12s\n" % (" " * len(name), "Step", "Time", "fmax") if self.nsteps == 0 else ""
        msg += "%s:  %3d %02d:%02d:%02d %12.4f\n" % (name, self.nsteps, T[3], T[4], T[5], fmax)
        if isinstance(self.logfile, str) and self.logfile != "-":
            with open(self.logfile, "a") as fh:
                fh.write(msg)
        else:
            out = sys.stdout if self.logfile == "-" else self.logfile
            out.write(msg)
            out.flush()

    def run(self, batch, fmax: float = 0.05, steps: Optional[int] = None) -> bool:
        self.initialize()
        self.fmax = fmax
        if steps:
            self.max_steps = steps
        dev = batch.pos.device
        st = self.state = LBFGSState(batch_ptr_host(batch), batch.pos, self.memory)
        fixed = self._fixed(st.N, dev)
        # the model's batch: same z / batch / ptr tensors, positions = the float32 tensor the step kernel rewrites (atoms_list_to_PYG does .float())
        work = Batch(st.pos32, batch.z, batch.batch, getattr(batch, "y", None), getattr(batch, "forces", None), batch.ptr if getattr(batch, "ptr", None) is not None else None)
        calc = self.calculator
        args = (self.fmax, self.maxstep, self.damping, self.alpha, fixed)
        calc.calculate(work)
        if self.logfile is not None:
            self._log(calc.forces)
        taken, latch = 0, -1
        while taken < self.max_steps:
            st.step(calc.forces, *args)
            taken += 1
            calc.calculate(work)
            if taken % self.check_every == 0 or taken == self.max_steps:
                latch = st.header()["latch"]
                if latch >= 0:
                    break
                if self.log_every_step and self.logfile is not None:
                    self.nsteps = taken
                    self._log(calc.forces)
        if latch < 0:      # steps exhausted (or max_steps == 0): the last forces decide (optimizers.py:108-111)
            st.step(calc.forces, *args, evaluate_only=True)
        h = st.header()
        # the step at which the latch fell saw an all-converged batch: the reference would not have taken it (`while not self.converged()`), and it moved nothing
        self.nsteps = h["latch"] if 0 <= h["latch"] < taken else taken
        self.n_normalizations = h["normalizations"]
        self.force_calls = self.function_calls = self.nsteps
        self.positions = st.r
        self.converged_mask = st.converged_dev.bool()
        if fixed is not None:
            calc.forces = calc.forces.masked_fill(fixed.bool()[:, None], 0.0)       # what get_forces(fixed_atoms_mask) leaves in results (calculator.py:84-87)
        if self.logfile is not None:
            self._log(calc.forces)
        return h["latch"] >= 0

    def converged(self) -> bool:
        return bool(self.converged_mask.all()) if self.converged_mask is not None else False


# ---- task -------------------------------------------------------------------------------------------------------------------------------
def _encode_ase_blob(obj: dict) -> bytes:
    """Inverse of ``data._decode_ase_blob`` (ase.db.core.object_to_bytes): <int64 json offset> <arrays, 8-byte aligned> <json>; numpy arrays go to the binary
    part as ``{"__ndarray__": [shape, dtype, offset]}``, everything else stays in the JSON document."""
    parts = [b"\0" * 8]
    size = 8

    def enc(o):
        nonlocal size
        if isinstance(o, dict):
            return {k: enc(v) for k, v in o.items()}
        if isinstance(o, np.ndarray):
            a = np.ascontiguousarray(o)
            if a.dtype.byteorder == ">":
                a = a.astype(a.dtype.newbyteorder("<"))
            offset = size
            raw = a.tobytes()
            pad = -len(raw) % 8
            parts.append(raw + b"\0" * pad)
            size += len(raw) + pad
            return {"__ndarray__": [list(a.shape), a.dtype.name, offset]}
        if isinstance(o, (np.floating, np.integer)):
            return o.item()
        return o

    doc = json.dumps(enc(obj), separators=(",", ":")).encode()
    parts[0] = struct.pack("<q", size)
    return b"".join(parts) + doc


class BatchwiseOptimizeTask:
    """optimization/task.py:9-73 without ase: reads the ASE-sqlite input with the standard library, optimises ``batch_size`` rows at a time and writes an output
    file with the input's schema (cloned from its ``sqlite_master``).  Every column of every row is copied verbatim except ``positions`` (the optimised
    geometry, float64) and ``data``, which gains ``model_energy`` (list of one float) and ``model_forces`` ([n, 3]) of the final geometry (task.py:56-69;
    the reference slices ``results["forces"][0:natoms]`` for every row because its ``force_idx`` never advances -- here each row gets its own atoms' forces).
    Pinned: the round trip through ``nabladft_amd.read_energy_database``.  Unpinned: that ``ase.db`` opens the output (ase is not a dependency and the tests do
    not have it); ase would also assign fresh ``unique_id`` / ``ctime`` values where this copies the input's."""

    def __init__(self, input_datapath: str, output_datapath: str, optimizer: ASEBatchwiseLBFGS, batch_size: int, fmax: float, steps: int) -> None:
        self.input_datapath, self.output_datapath = input_datapath, output_datapath
        self.optimizer, self.bs, self.fmax, self.steps = optimizer, batch_size, fmax, steps
        if not os.path.isfile(input_datapath):
            raise FileNotFoundError(input_datapath)

    def _open_output(self, src):
        if os.path.exists(self.output_datapath):
            raise FileExistsError(f"{self.output_datapath} exists; the task writes a new file")
        out = sqlite3.connect(self.output_datapath)
        for typ, name, sql in src.execute("select type, name, sql from sqlite_master order by rowid"):
            if sql is not None and not name.startswith("sqlite_"):
                out.execute(sql)
        for (name,) in src.execute("select name from sqlite_master where type = 'table' and name not like 'sqlite_%' and name != 'systems'").fetchall():
            rows = src.execute(f"select * from {name}").fetchall()                 # side tables (keys, information, ...) as they are
            if rows:
                out.executemany(f"insert into {name} values ({','.join('?' * len(rows[0]))})", rows)
        return out

    def optimize_batch(self, batch: Batch):
        self.optimizer.run(batch, fmax=self.fmax, steps=self.steps)
        return self.optimizer.positions

    def run(self):
        src = sqlite3.connect(f"file:{self.input_datapath}?mode=ro", uri=True)
        try:
            cols = [r[1] for r in src.execute("pragma table_info(systems)")]
            rows = src.execute("select * from systems order by id").fetchall()
            out = self._open_output(src)
        finally:
            src.close()
        i_num, i_pos, i_data = cols.index("numbers"), cols.index("positions"), cols.index("data")
        device = self.optimizer.calculator.device
        insert = f"insert into systems ({','.join(cols)}) values ({','.join('?' * len(cols))})"
        try:
            for lo in range(0, len(rows), self.bs):
                chunk = rows[lo:lo + self.bs]
                z = [np.frombuffer(r[i_num], dtype=np.int32) for r in chunk]
                pos = [np.frombuffer(r[i_pos], dtype=np.float64).reshape(-1, 3) for r in chunk]
                sizes = np.array([len(a) for a in z])
                ptr = np.concatenate([[0], np.cumsum(sizes)])
                batch = Batch(torch.from_numpy(np.concatenate(pos)).to(device), torch.from_numpy(np.concatenate(z).astype(np.int64)).to(device),
                              torch.from_numpy(np.repeat(np.arange(len(chunk)), sizes)).to(device), None, None, torch.from_numpy(ptr).to(device))
                final = self.optimize_batch(batch).cpu().numpy()
                res = self.optimizer.calculator.results
                energy, forces = res[self.optimizer.calculator.energy_key], res[self.optimizer.calculator.force_key]
                for k, r in enumerate(chunk):
                    a, b = int(ptr[k]), int(ptr[k + 1])
                    data = dict(_decode_ase_blob(r[i_data]))
                    data["model_energy"] = [float(energy[k])]
                    data["model_forces"] = np.ascontiguousarray(forces[a:b])
                    new = list(r)
                    new[i_pos] = np.ascontiguousarray(final[a:b], dtype=np.float64).tobytes()
                    new[i_data] = _encode_ase_blob(data)
                    out.execute(insert, new)
                out.commit()
        finally:
            out.close()


def __getattr__(name):
    # nablaDFT.optimization also exports PYGAseInterface (pyg_ase_interface.py:119-335); it lives in md.py, which imports this module
    if name in ("PYGAseInterface", "BatchedMD"):
        from . import md
        return getattr(md, name)
    if name == "BatchedVibrations":
        from . import vibrations
        return vibrations.BatchedVibrations
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["ASEBatchwiseLBFGS", "PyGBatchwiseCalculator", "BatchwiseOptimizeTask", "LBFGSState", "PYGAseInterface", "BatchedMD", "BatchedVibrations"]
