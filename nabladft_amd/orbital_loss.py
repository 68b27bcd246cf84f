"""Training on the spectrum: differentiable orbital energies of a predicted Hamiltonian, a loss on them, and the QHNet task that adds it to the matrix loss
(csrc/orbdens.hip, ``nq_orb_wgram`` of include/nablaq.h, on top of nabladft_amd/orbitals.py).

Fills the same empty slots as the solver: ``phisnet/nn/neural_network.py:969-993`` returns ``orbital_energies`` as zeros, so the reference has nothing a loss on
them could be compared with.  Parity status: **no reference code to pin against** -- the gradients are tested against ``torch.linalg`` autograd of the
Cholesky -> reduce -> ``eigvalsh`` route and against the closed form on a permuted copy of the problem (tests/orbital_grad_ref.py).

For ``H C = S C diag(eps)`` with ``C^T S C = I`` the eigenvalues move by ``d eps_k = c_k^T (dH - eps_k dS) c_k``, so for a loss ``L(eps)`` with
``g = dL/d eps``

    dL/dH = sum_k g_k c_k c_k^T            dL/dS = -sum_k g_k eps_k c_k c_k^T

No difference of eigenvalues is divided by: degenerate orbitals cannot blow the gradient up.  Both come out of ONE launch of the weighted Gram kernel on the
coefficient rows the solver left on the device (float64 matrix instructions, exactly symmetric, bitwise reproducible).

**Convention.**  The gradient handed back is that symmetric matrix: the gradient with respect to a *symmetric* input, which is also what
``torch.linalg.eigh`` returns.  Only the lower triangles of ``H`` and ``S`` are read by the solver, yet the gradient is spread over both triangles; the
assemblers (``BlockAssembler`` / ``IrrepsAssembler`` with ``symmetrize=True``) build ``H`` as ``X + X^T``, so the gradients of the network's parameters are the
true ones.

**Coefficients stay detached.**  No gradient flows through the eigenvectors: there is no loss on coefficients, densities or populations here
(``BatchedOrbitals.density`` / ``populations`` are post-processing).

Limits (each raises, nothing degrades silently): what ``BatchedOrbitals`` has -- 1..1024 orbitals per molecule, closed shells, MI355X only, no CPU path.
"""
from typing import Optional

import numpy as np
import torch
from torch import nn

from .lightning import QHNetLightning
from .orbitals import BatchedOrbitals, _orb_ptr_of, _require_gpu, check_occupied, mulliken_charges, occupied_counts  # noqa: F401


class _OrbitalEnergies(torch.autograd.Function):
    """Forward: ``BatchedOrbitals.solve``.  Backward: one ``nq_orb_wgram`` launch for ``gH`` (and ``gS`` when ``S`` asks for it)."""

    @staticmethod
    def forward(ctx, orb, H, S):
        orb.solve(H, S)
        ctx.orb = orb
        ctx.h = (H.shape, H.dtype)
        ctx.s = None if S is None else (S.shape, S.dtype)
        return orb.energies.clone()

    @staticmethod
    def backward(ctx, g):
        orb = ctx.orb
        g = g.to(torch.float64).reshape(-1).contiguous()
        want_s = ctx.s is not None and ctx.needs_input_grad[2]
        if not ctx.needs_input_grad[1] and not want_s:
            return None, None, None
        if want_s:
            gH, gS = orb.weighted_gram(g, -(orb.energies * g))
            gS = gS.to(ctx.s[1]).view(ctx.s[0])
        else:
            gH, gS = orb.weighted_gram(g), None
        return None, gH.to(ctx.h[1]).view(ctx.h[0]), gS


def orbital_energies(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, return_solution: bool = False):
    """Orbital energies of every molecule of a batch, differentiable with respect to ``H_packed`` and ``S_packed`` -> ``eps`` float64 [M] on the device,
    ascending inside each molecule (``return_solution=True``: ``(eps, BatchedOrbitals)``).

    ``H_packed`` / ``S_packed``: float32 or float64 packed matrices (``S_packed = None``: the identity); ``plan_or_orb_ptr``: a plan or ``orb_ptr`` [B+1] as
    for ``BatchedOrbitals``.  The gradients are the symmetric matrices ``sum_k g_k c_k c_k^T`` and ``-sum_k g_k eps_k c_k c_k^T`` (the convention of
    ``torch.linalg.eigh``, see the module text), cast to the inputs' dtypes; ``S`` gets one only if it requires it.  No solver status is read back and ``check()``
    is not called (a plan costs one small device -> host copy of its ``mol_orb_ptr``, an ``orb_ptr`` already on the host costs none, and preparing the solver
    state synchronises the stream once, as in ``BatchedOrbitals``): a molecule the solver fails on (an overlap that is not positive definite) yields NaN
    energies and a NaN gradient block for that molecule only.  ``return_solution=True`` hands back the solution to call ``check()`` on.  Its coefficients are detached: no gradient flows through eigenvectors."""
    _require_gpu(H_packed)
    if S_packed is not None:
        _require_gpu(S_packed)
    orb = BatchedOrbitals(plan_or_orb_ptr, H_packed.device)
    eps = _OrbitalEnergies.apply(orb, H_packed, S_packed)
    return (eps, orb) if return_solution else eps


class OrbitalEnergyLoss(nn.Module):
    """``kind`` "mae" | "mse" of the orbital energies over ``which`` = "occupied" (k < n_occ) | "all" | "frontier" (HOMO and LUMO; the HOMO alone where every
    orbital is occupied): the mean over the selected orbitals of each molecule, then the mean over the molecules.  ``("mae", "occupied")`` is the
    ``eps_mae_occ`` of ``OrbitalErrors``.  ``charge`` (one number or one per molecule) is what ``occupied(z, ptr, orb_ptr)`` counts electrons with."""

    packed = True          # QHNetOrbitalLightning, like QHNetLightning, hands packed quantities to losses that declare this

    def __init__(self, kind: str = "mae", which: str = "occupied", charge=0):
        super().__init__()
        if kind not in ("mae", "mse"):
            raise ValueError(f"kind must be 'mae' or 'mse', not {kind!r}")
        if which not in ("occupied", "all", "frontier"):
            raise ValueError(f"which must be 'occupied', 'all' or 'frontier', not {which!r}")
        self.kind, self.which, self.charge = kind, which, charge

    def occupied(self, z, ptr, orb_ptr=None) -> torch.Tensor:
        """``occupied_counts(z, ptr, self.charge, orb_ptr)``: int32 [B] on the host."""
        return occupied_counts(z, ptr, self.charge, orb_ptr)

    def forward(self, eps_pred: torch.Tensor, eps_target: torch.Tensor, n_occ, orb_ptr) -> torch.Tensor:
        _require_gpu(eps_pred)
        op = _orb_ptr_of(orb_ptr)
        no = check_occupied(n_occ, op)
        m = np.diff(op)
        B, M = m.shape[0], int(op[-1])
        if eps_pred.numel() != M or eps_target.numel() != M:
            raise ValueError(f"the energies have {eps_pred.numel()} / {eps_target.numel()} entries, orb_ptr counts {M}")
        k = np.arange(M) - np.repeat(op[:-1], m)
        nk = np.repeat(no.astype(np.int64), m)
        if self.which == "occupied":
            sel = k < nk
        elif self.which == "all":
            sel = np.ones(M, dtype=bool)
        else:
            sel = (k == nk - 1) | (k == nk)                      # k == n_occ does not exist where n_occ = m: the HOMO alone
        count = np.add.reduceat(sel.astype(np.float64), op[:-1])
        dev = eps_pred.device
        weight = torch.from_numpy(sel / np.repeat(count, m) / B).to(dev)        # float64 [M]: mean over the selection, then over the molecules
        d = eps_pred.reshape(-1).to(torch.float64) - eps_target.reshape(-1).to(torch.float64).detach()
        return torch.sum(weight * (d.abs() if self.kind == "mae" else d * d))


class QHNetOrbitalLightning(QHNetLightning):
    """``QHNetLightning`` with a term on the orbital energies: ``_evaluate`` adds ``"orbital_energies"`` to predictions and targets -- ``orbital_energies`` of
    the packed prediction under ``batch.overlap`` (a list of per-molecule matrices like ``batch.hamiltonian``; absent or None: the identity) and a detached
    solve of the packed target -- and ``losses`` / ``loss_coefs`` take that key beside ``"hamiltonian"`` (an ``OrbitalEnergyLoss``, whose ``charge`` counts the
    occupied orbitals).  Each step with the orbital term reads the batch's ``z`` / ``ptr`` and the plan's orbital pointer back to the host (two small copies).  Constructor, ``state_dict``, EMA hooks, validation, test and predict are the parent's; every loss must be a packed one.  With the
    coefficient at 0 (or without the key) nothing is solved and the step is ``QHNetLightning``'s."""

    KEY = "orbital_energies"

    def _orbital_term(self):
        return self.KEY in self.hparams.losses and self.hparams.loss_coefs.get(self.KEY, 0) != 0

    def _evaluate(self, batch):
        if not self._packed():
            raise ValueError("QHNetOrbitalLightning needs packed losses (HamiltonianLoss, OrbitalEnergyLoss): the dense path has no orbital term")
        preds, targets, loss_args = super()._evaluate(batch)
        if self._orbital_term():
            plan, asm = self.net.last_plan, self.net._asm
            overlap = getattr(batch, "overlap", None)
            S = None if overlap is None else asm.pack_targets(plan, overlap)
            op = _orb_ptr_of(plan)
            preds[self.KEY] = orbital_energies(preds["hamiltonian"], S, op)
            targets[self.KEY] = BatchedOrbitals(op, preds["hamiltonian"].device).solve(targets["hamiltonian"], S).energies
            loss_fn = self.hparams.losses[self.KEY]
            charge = getattr(loss_fn, "charge", 0)
            preds[self.KEY + "_args"] = (occupied_counts(batch.z, batch.ptr, charge, op), op)       # what the loss needs beside the energies: (n_occ, orb_ptr)
        return preds, targets, loss_args

    def _calculate_loss(self, y_pred, y_true, *loss_args):
        total = 0
        for name, fn in self.hparams.losses.items():
            if name == self.KEY:
                if self._orbital_term():
                    total = total + self.hparams.loss_coefs[name] * fn(y_pred[name], y_true[name], *y_pred[name + "_args"])
            else:
                total = total + self.hparams.loss_coefs[name] * fn(y_pred[name], y_true[name], *loss_args)
        return total

    def _calculate_metrics(self, y_pred, y_true, mask=None):
        # the metric sees the matrices only.  The parent's rescaling by the dense ``mask`` has no place here: ``_evaluate`` refuses the dense path, so ``mask`` is None
        if self.hparams.metric is None:
            return {}
        return self.hparams.metric({"hamiltonian": y_pred["hamiltonian"]}, {"hamiltonian": y_true["hamiltonian"]})


__all__ = ["orbital_energies", "OrbitalEnergyLoss", "QHNetOrbitalLightning", "mulliken_charges"]
