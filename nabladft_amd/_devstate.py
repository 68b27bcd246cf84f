"""What the device-resident batched jobs share on the Python side (optimization.py, md.py, vibrations.py, orbitals.py): one caller-owned device buffer cut
into 16-byte-aligned parts by ``nq_<job>_state_layout`` (csrc/devstate.h), typed views of those parts, and the argument checks of the jobs' entry points."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib


class DeviceState:
    """Base of ``LBFGSState`` / ``MDState`` / ``VibState`` / ``OrbitalState``: ``buf`` (uint8, the whole state), ``_dims`` (what every ``nq_<job>_*`` call
    repeats) and one attribute per named part."""

    def _allocate(self, prefix: str, dims, parts, device) -> int:
        """``parts``: the job's ordered ``(name, dtype, shape)`` table, in the order of the part enum of its .hip file; a part named None gets no attribute.
        -> the size of ``buf`` in bytes."""
        lib = _lib.load()
        self._dims = tuple(dims)
        nbytes = getattr(lib, f"nq_{prefix}_state_bytes")(*self._dims)
        if nbytes == 0:
            raise _lib.NablaqError(_lib.NQ_ERR_ARG, lib.nq_last_error().decode(errors="replace"))
        off = (C.c_size_t * len(parts))()
        _lib.check(getattr(lib, f"nq_{prefix}_state_layout")(*self._dims, off))
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        for o, (name, dtype, shape) in zip(off, parts):
            if name is not None:
                size = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
                setattr(self, name, self.buf[o:o + size].view(dtype).view(shape))
        return nbytes

    def _read_header(self) -> list:
        """The header words (one small device->host copy, synchronises the stream)."""
        return self.header_dev.cpu().tolist()


def require_positions(pos: torch.Tensor, module_name: str):
    if not pos.is_cuda:
        raise RuntimeError(f"nabladft_amd.{module_name} runs on MI355X only (no CPU fallback): move the batch to cuda")
    if pos.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"positions must be float32 or float64, not {pos.dtype}")


def require_forces(forces: torch.Tensor, n: int, device) -> torch.Tensor:
    if forces.dtype not in (torch.float32, torch.float64) or tuple(forces.shape) != (n, 3) or forces.device != device:
        raise ValueError(f"forces must be a float32 / float64 [{n}, 3] tensor on {device}")
    return forces.contiguous()


def fixed_to_uint8(fixed, N: int):
    """uint8 [N] on the host, 1 = fixed, from indices or a boolean mask (array or tensor); None stays None."""
    if fixed is None:
        return None
    mask = np.zeros(N, dtype=np.uint8)
    mask[np.asarray(fixed.cpu() if isinstance(fixed, torch.Tensor) else fixed)] = 1
    return mask


def batch_ptr_host(batch) -> np.ndarray:
    """``ptr`` [B+1] of a batch on the host: its ``ptr`` if it has one, else counted from ``batch.batch``."""
    if getattr(batch, "ptr", None) is not None:
        return batch.ptr.cpu().numpy()
    return np.concatenate([[0], np.cumsum(np.bincount(batch.batch.cpu().numpy()))])
