"""Training on the spectrum and on the occupied subspace: differentiable orbital energies, density matrices and Mulliken populations of a predicted
Hamiltonian, losses on them, and the QHNet tasks that add them to the matrix loss (csrc/orbdens.hip, csrc/orbresp.hip, ``nq_orb_wgram`` / ``nq_orb_resp_*`` /
``nq_orb_syr2k`` / ``nq_orb_population_backward`` of include/nablaq.h, on top of nabladft_amd/orbitals.py).

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

**Eigenvectors.**  No gradient flows through the eigenvectors of ``orbital_energies``: its coefficients stay detached, and ``BatchedOrbitals.density`` /
``populations`` are post-processing.  The occupied subspace is differentiated by ``orbital_solution`` / ``density_matrix`` below: the closed-shell density
``D = 2 C_o C_o^T`` depends on the eigenvectors only through the occupied subspace, and with ``Gs = (G + G^T) / 2`` for ``G = dL/dD``

    T = Gs C_o        W = C^T T        Z_ai = 4 W_ai / (eps_i - eps_a)   (a virtual, i occupied)
    R_H = C_v Z       R_S = -C_v (Z o eps_i) - 2 C_o W_o
    dL/dH = (R_H C_o^T + C_o R_H^T) / 2        dL/dS = (R_S C_o^T + C_o R_S^T) / 2

(csrc/orbresp.hip: four float64 matrix-instruction launches on the coefficient rows the solver left on the device, bitwise reproducible, exactly symmetric).
Only occupied-virtual differences are divided by: equal levels inside the occupied or inside the virtual orbitals are harmless, where the backward of
``torch.linalg.eigh`` divides by every difference and returns garbage.  With every orbital occupied ``dL/dH`` is exactly zero and ``dL/dS`` is that of
``D = 2 S^-1``.  **No gap regularisation, no clamping:** a vanishing HOMO-LUMO gap gives inf / NaN in that molecule's gradient block only;
``BatchedOrbitals.frontier`` gives the gap to watch.  Tested against ``torch.linalg`` autograd of Cholesky -> reduce -> ``eigh`` -> ``D`` and against the
closed form on a permuted copy (tests/orbital_density_ref.py).

**Smearing.**  ``smeared_solution`` / ``smeared_density_matrix`` replace the closed shell by Fermi-Dirac occupations ``F_k = 2 / (1 + exp((eps_k - mu) / kT))``
with ``mu`` fixed by the electron count (any count in (0, 2m): odd ones too).  ``D = sum_k F_k c_k c_k^T`` is then a smooth function of ``H`` and ``S`` also
where levels coincide or cross, and its response is ``C (K o W) C^T`` over ALL orbital pairs with the divided differences
``K_ij = (F_i - F_j) / (eps_i - eps_j)``, ``K_kk = F'_k``, which csrc/orbsmear.hip evaluates as
``-(1 / (2 kT)) sinhc((x_i - x_j) / 2) / (cosh(x_i / 2) cosh(x_j / 2))``: without dividing by a difference of orbital energies anywhere in the chain.  What IS
divided by: ``kT`` (which must be positive), ``(x_i - x_j) / 2`` inside sinhc (its limit 1 is taken at equal levels), the ``1 + e^-|x|`` factors of the Fermi
function, and the sum of the weights ``F'_k / sum F'`` that carry the gradient of ``mu`` (a softmax, never zero).  A vanishing or crossed HOMO-LUMO gap gives
finite gradients; with a gap much larger than ``kT`` the chain becomes that of ``orbital_solution``, which is unchanged, as is its behaviour at a vanishing
gap.  Tested against ``torch.linalg`` autograd, the closed form on a permuted copy and finite differences (tests/orbital_smearing_ref.py).

**Without a solve.**  ``purified_density_matrix`` gives the same closed-shell ``D`` and the same gradients from symmetric matrix products alone
(csrc/orbpurify.hip, ``BatchedPurification``): ``Z = L^-1`` of ``S = L L^T``, ``X`` the projector on the ``n_occ`` lowest levels of ``Z H Z^T`` by second-order
spectral-projection purification (SP2), ``D = 2 Z^T X Z``.  The response of a spectral projector is a self-adjoint map on symmetric matrices, so its
vector-Jacobian product is the density-matrix-perturbation recursion run with the upstream gradient as the perturbation, alongside the same SP2 iterates:
``X1_0 = -Gt / (e_max - e_min)``, ``X1 <- P + P^T`` or ``2 X1 - (P + P^T)`` with ``P = X X1`` by the branch the forward logged; then ``dL/dH = Z^T g Z`` and
``dL/dS = -Z^T (M + M^T + X Gt X) Z`` with ``M = g X Ht``.  No eigenpairs, no stored iterates, nothing divided.  It needs an open gap (a level shared by the
occupied and the virtual side does not converge: status 4, NaN in that molecule's blocks) and has no energies other than HOMO and LUMO (below) and no smearing: ``orbital_solution`` /
``smeared_solution`` stay the route for those.  ``QHNetPurifiedDensityLightning`` is ``QHNetDensityLightning`` on it.  Tested against the same yardsticks as
``orbital_solution`` and against ``orbital_solution`` itself (tests/orbital_purify_ref.py).

**HOMO, LUMO and the gap without a solve.**  The purification leaves the orthogonalised ``Ht``, the projector ``X`` and the Gershgorin bounds on the device;
``eps_HOMO = e_min + lambda_max(X (Ht - e_min I) X)`` and ``eps_LUMO = e_max - lambda_max((I - X)(e_max I - Ht)(I - X))`` are extreme eigenvalues of positive
semidefinite operators, which ``purified_frontier`` finds by a fully reorthogonalised Lanczos recurrence (csrc/orbfrontier.hip: one workgroup per molecule and
side, tens to about two hundred matrix-vector steps, no ``m^3`` work).  With ``c = Z^T v`` the gradients are ``d eps / dH = c c^T`` and
``d eps / dS = -eps c c^T``, the convention of ``orbital_energies``: no eigenvector response.  ``FrontierLoss`` is the loss on them (``("mae", "both")`` equals
``OrbitalEnergyLoss("mae", "frontier")``), ``QHNetPurifiedFrontierLightning`` the task with the key ``"frontier"``; a purified density term of the same step
shares the purification (``solution=``).  These two are the only VIRTUAL-side information the purification route has; ``purified_occupied_energies`` (below) gives every occupied level.  Tested against ``np.linalg.eigh``,
``torch.linalg`` autograd and ``BatchedOrbitals.frontier`` (tests/orbital_frontier_ref.py).

**All occupied levels without a full solve.**  An exact orthogonal projector of rank ``n_occ`` has a pivoted Cholesky factor ``X = Q^T Q`` whose rows are
orthonormal (``X^2 = X`` forces ``Q Q^T = I``; every Schur complement is again a projector, so every pivot is at least ``1/m``): the occupied levels are the standard
eigenvalues of the ``n_occ x n_occ`` matrix ``Q Ht Q^T`` and ``C = V Q Z`` their coefficients (csrc/orbocc.hip; the reduced blocks go through the batched solver).
``purified_occupied_energies`` returns them with NaN in the virtual slots; the gradients are ``c_k c_k^T`` and ``-eps_k c_k c_k^T`` again, one ``nq_orb_wgram`` launch.
``OccupiedEnergyLoss`` is ``OrbitalEnergyLoss(kind, "occupied")`` for such energies, ``QHNetPurifiedOrbitalLightning`` takes the key ``"occupied_energies"`` and shares
the purification with the density, charge and frontier terms, ``PurifiedOrbitalErrors`` reports ``eps_mae_occ`` / ``similarity`` of a test loop.  Closed shells, an open
gap, occupied levels only.  Tested against ``np.linalg.eigh``, ``scipy.linalg.eigh``, ``torch.linalg`` autograd and the solver route (tests/orbital_occupied_ref.py).

**Bond orders.**  ``bond_orders`` gives the Mayer bond-order table and the atomic valences of a closed-shell density under ``S``: with ``P = D S``,
``B_AB = sum_{mu in A, nu in B} P_mu,nu P_nu,mu`` and ``V_A = sum_{B != A} B_AB`` (``S = None``: the Wiberg index of an orthogonal basis).  The reverse forms
``E = dL/dP`` elementwise (``E_mu,nu = (Gamma_AB + Gamma_BA) P_nu,mu``, ``Gamma_AB = gB_AB + (A != B) gV_A``) and then ``dL/dD = sym(E S)``, ``dL/dS = sym(D E)`` as
float64 matrix-instruction products (csrc/orbbond.hip), exactly symmetric and bitwise reproducible.  For an idempotent density, ``(DS)^2 = 2 DS``, the rows sum
to twice the Mulliken populations: ``sum_B B_AB = 2 pop_A``.  ``BondOrderLoss`` and ``QHNetBondOrderLightning`` put the table beside the other targets.  Closed
shells only (no spin-density term), at most 32 orbitals per atom.  Tested against a numpy restatement and ``torch`` autograd (tests/orbital_bond_ref.py).

**Löwdin analysis.**  With ``S = U diag(s) U^T``, ``a = sqrt(s)``, ``A = S^(1/2) = U diag(a) U^T`` and ``A^- = S^(-1/2)``: ``lowdin_basis`` makes both from ONE
standard solve of ``S`` and one ``nq_orb_wgram`` launch; ``lowdin_density`` gives ``D^L = A D A``, ``lowdin_hamiltonian`` gives ``H^L = A^- H A^-`` (the matrix
SchNOrb-style models train on; its eigenvalues are the generalised ``eps``), ``lowdin_populations`` the populations ``q_A = sum_{mu in A} D^L_mu,mu`` (their sum
is ``Tr(D S)``), ``lowdin_bond_orders`` the Wiberg indices ``W_AB = sum_{mu in A, nu in B} (D^L_mu,nu)^2`` and the valences; for an idempotent closed-shell
density ``sum_B W_AB = 2 q_A``.  The congruence ``M^L = sym(X Y)``, ``Y = M X``, has the reverse ``dL/dM = sym(X (G X))``, ``dL/dX = Y G + G Y^T``; the matrix
functions have the Daleckii-Krein reverse ``dL/dS = U [K o (U^T sym(g) U)] U^T`` with ``K_ij = 1 / (a_i + a_j)`` for ``A`` and ``-1 / (a_i a_j (a_i + a_j))`` for
``A^-``, the diagonal included: NO difference of levels of ``S`` is divided, so equal levels (``S = I``, identical atoms far apart) give finite gradients where
the backward of ``torch.linalg.eigh`` returns non-finite values (csrc/orblowdin.hip, float64 matrix instructions, exactly symmetric, bitwise reproducible).
``LowdinChargeLoss`` and ``QHNetLowdinLightning`` put the charges and the table beside the other targets.  ``S`` belongs to the conformer, not to the model: a
``LowdinBasis`` can be cached across epochs.  Limits: closed shells only, ``S`` positive definite (info 1 and NaN otherwise), 1..1024 orbitals per molecule,
at most 32 orbitals per atom for the bond table, no ``S^(1/2)`` without a decomposition.  Tested against a numpy restatement, ``scipy.linalg.sqrtm`` and
``torch`` autograd (tests/orbital_lowdin_ref.py).

**SCF residual.**  ``scf_residual`` gives ``R^L = [H^L, D^L]`` of a Hamiltonian and a density in the Löwdin basis, the DIIS error vector
``S^(-1/2) (H D S - S D H) S^(-1/2)``.  It vanishes exactly when ``D`` is a stationary density of ``H``; with ``D`` the target's idempotent closed-shell density and
``H`` the prediction, ``sum_ij (R^L_ij)^2 = 8 sum_{i occ, a virt} h_ia^2`` with ``h_ia`` the occupied-virtual block of the predicted ``H^L`` in the TARGET's
orbitals: the block that rotates the occupied subspace.  Proof: ``D^L = 2 Q`` with ``Q`` the projector on the occupied space, ``[H^L, Q] = (1 - Q) H^L Q -
Q H^L (1 - Q)``, two blocks of equal norm ``sum h_ia^2`` that do not overlap, times ``2^2``.  No eigenpairs of the prediction, no ``1 / (eps_i - eps_a)``, no
iteration: the residual is linear in ``H``, finite at closed and crossed gaps, and its reverse is the same kernel (csrc/orbcomm.hip): for ``C = X Y - Y X`` and
``G_a`` the antisymmetric part of ``dL/dC``, ``dL/dX = [G_a, Y]`` and ``dL/dY = [X, G_a]``, both symmetric.  ``S`` and the target density belong to the
conformer: ``scf_target`` builds an ``ScfTarget`` (one target solve and one ``LowdinBasis.of``, or with ``scf_target_iterative`` Newton-Schulz square roots and an
SP2 purification of the Löwdin Hamiltonian: no solve at all) that can be cached across epochs (``scf_target_blocks`` gives the fields to store), after which a step
(``scf_residual_to_target``) is two congruence products and one commutator.  ``ScfResidualLoss`` and ``QHNetCommutatorLightning`` put the term beside the other
targets; ``ScfResidualErrors`` reports its root mean square and maximum.  What it is NOT: it carries no gap weighting, it is not ``D_pred - D_target``, and it
says nothing about the order of the levels inside the occupied space.  Tested against a numpy restatement and ``torch`` autograd
(tests/orbital_commutator_ref.py).

Limits (each raises, nothing degrades silently): what ``BatchedOrbitals`` has -- 1..1024 orbitals per molecule, closed shells or Fermi occupations (no spin
polarisation), MI355X only, no CPU path.
"""
from collections import namedtuple
from typing import Optional

import numpy as np
import torch
from torch import nn

from .lightning import QHNetLightning
from .orbitals import (BatchedMatrixRoot, BatchedOrbitals, BatchedPurification, FrontierLevels, LowdinBasis, Orthogonalizer, _orb_ptr_of, _require_gpu, bond_layout, check_occupied, dense_bond_orders,  # noqa: F401
                       ScfResidualErrors, electron_counts, mulliken_charges, occupied_counts, OccupiedOrbitals, PurifiedOrbitalErrors)


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


class _OrbitalSolution(torch.autograd.Function):
    """Forward: ONE ``BatchedOrbitals.solve`` and the density of its occupied orbitals.  Backward: ``nq_orb_wgram`` for the energies' upstream gradient plus the
    response chain for the density's; a half without an upstream gradient is skipped, and so is the ``S`` half when ``S`` asks for nothing."""

    @staticmethod
    def forward(ctx, orb, H, S, n_occ):
        orb.solve(H, S)
        ctx.set_materialize_grads(False)
        ctx.orb, ctx.n_occ = orb, n_occ
        ctx.h = (H.shape, H.dtype)
        ctx.s = None if S is None else (S.shape, S.dtype)
        return orb.energies.clone(), orb.density(n_occ)

    @staticmethod
    def backward(ctx, g_eps, g_D):
        orb = ctx.orb
        want_h = ctx.needs_input_grad[1]
        want_s = ctx.s is not None and ctx.needs_input_grad[2]
        if (g_eps is None and g_D is None) or not (want_h or want_s):
            return None, None, None, None
        gH = gS = None
        if g_eps is not None:
            g = g_eps.to(torch.float64).reshape(-1).contiguous()
            if want_s:
                gH, gS = orb.weighted_gram(g, -(orb.energies * g))
            else:
                gH = orb.weighted_gram(g)
        if g_D is not None:
            rH, rS = orb.density_response(g_D.to(torch.float64).reshape(-1).contiguous(), ctx.n_occ, want_s)
            gH = rH if gH is None else gH + rH
            if want_s:
                gS = rS if gS is None else gS + rS
        return (None, gH.to(ctx.h[1]).view(ctx.h[0]) if want_h else None, gS.to(ctx.s[1]).view(ctx.s[0]) if want_s else None, None)


def orbital_solution(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, n_occ, return_solution: bool = False):
    """Orbital energies AND the closed-shell density matrix of every molecule from ONE solve -> ``(eps float64 [M], D float64 [P])`` on the device
    (``return_solution=True``: ``(eps, D, BatchedOrbitals)``), both differentiable with respect to ``H_packed`` and ``S_packed``.

    Arguments as for ``orbital_energies``; ``n_occ`` [B]: doubly occupied orbitals per molecule (``occupied_counts``), checked on the host.
    ``D = 2 sum_{k < n_occ} c_k c_k^T`` is packed like the input and exactly symmetric.  The backward adds the ``nq_orb_wgram`` term of ``eps`` to the response
    chain of ``D`` (module text; the upstream gradient of ``D`` need not be symmetric), skips whichever output has no upstream gradient, skips the ``S`` half
    when ``S`` is None or requires no gradient, and casts the gradients to the inputs' dtypes.  The symmetric-matrix convention of ``orbital_energies``
    holds.  **No gap regularisation and no clamping**: the response divides by ``eps_i - eps_a`` over occupied i and virtual a, so a vanishing HOMO-LUMO gap
    gives inf / NaN in that molecule's gradient block only (``BatchedOrbitals.frontier`` returns the gap); degenerate levels inside the occupied or inside the
    virtual orbitals are harmless.  A molecule the solver fails on yields NaN energies, density and gradient blocks, for that molecule only."""
    _require_gpu(H_packed)
    if S_packed is not None:
        _require_gpu(S_packed)
    orb = BatchedOrbitals(plan_or_orb_ptr, H_packed.device)
    no = torch.from_numpy(check_occupied(n_occ, orb.orb_ptr))
    eps, D = _OrbitalSolution.apply(orb, H_packed, S_packed, no)
    return (eps, D, orb) if return_solution else (eps, D)


def density_matrix(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, n_occ, return_solution: bool = False):
    """``orbital_solution`` without the energies -> ``D`` float64 [P] (``return_solution=True``: ``(D, BatchedOrbitals)``); the backward is the response chain
    alone."""
    out = orbital_solution(H_packed, S_packed, plan_or_orb_ptr, n_occ, return_solution)
    return out[1:] if return_solution else out[1]


class _Populations(torch.autograd.Function):
    """Forward: ``nq_orb_population``.  Backward: ``nq_orb_population_backward`` (one elementwise launch)."""

    @staticmethod
    def forward(ctx, orb, plan, D, S, H):
        ctx.set_materialize_grads(False)
        pop, nelec, eband = orb.populations(D, plan, S, H)
        ctx.orb, ctx.plan = orb, plan
        ctx.save_for_backward(D, S, H)
        ctx.s = None if S is None else (S.shape, S.dtype)
        ctx.h = None if H is None else (H.shape, H.dtype)
        if eband is None:
            eband = nelec.new_zeros(nelec.shape)             # a placeholder the caller drops: a Function returns tensors
            ctx.mark_non_differentiable(eband)
        return pop, nelec, eband

    @staticmethod
    def backward(ctx, g_pop, g_nelec, g_eband):
        D, S, H = ctx.saved_tensors
        want_s = ctx.s is not None and ctx.needs_input_grad[3]
        want_h = ctx.h is not None and ctx.needs_input_grad[4]
        if g_pop is None and g_nelec is None and g_eband is None:
            return None, None, None, None, None
        f64 = lambda g: None if g is None else g.to(torch.float64).reshape(-1).contiguous()
        gD, gS, gH = ctx.orb.populations_backward(ctx.plan, f64(g_pop), f64(g_nelec), f64(g_eband) if ctx.h is not None else None, D, S, H, want_s, want_h)
        return (None, None, gD.view(D.shape) if ctx.needs_input_grad[2] else None, gS.to(ctx.s[1]).view(ctx.s[0]) if want_s else None,
                gH.to(ctx.h[1]).view(ctx.h[0]) if want_h else None)


def populations(D: torch.Tensor, plan, S_packed: Optional[torch.Tensor] = None, H_packed: Optional[torch.Tensor] = None, orbitals: Optional[BatchedOrbitals] = None):
    """Differentiable Mulliken analysis of a packed float64 density -> ``(atom_pop [N], nelec [B], eband [B] or None without H_packed)`` as
    ``BatchedOrbitals.populations``, with gradients for ``D`` and, where they require one, ``S_packed`` and ``H_packed``.  The gradients are those with respect
    to SYMMETRIC matrices, spread over both triangles (the convention of this module): ``dL/dD_ij = ((g_A(i) + g_A(j)) / 2 + g_nelec) S_ij + g_eband H_ij``.
    ``orbitals``: the solution of the same batch, whose state the kernels read the layout from (None: one is prepared, which synchronises the stream once)."""
    _require_gpu(D)
    orb = BatchedOrbitals(plan, D.device) if orbitals is None else orbitals
    pop, nelec, eband = _Populations.apply(orb, plan, D, S_packed, H_packed)
    return pop, nelec, (None if H_packed is None else eband)


def _molecule_mean_weights(counts: np.ndarray, device) -> torch.Tensor:
    """float64 [sum counts]: 1 / (count of the entry's molecule) / B -- the mean over a molecule's entries, then over the molecules."""
    return torch.from_numpy(np.repeat(1.0 / (counts.astype(np.float64) * counts.shape[0]), counts)).to(device)


class _PackedMeanLoss(nn.Module):
    packed = True

    def __init__(self, kind: str = "mae", charge=0):
        super().__init__()
        if kind not in ("mae", "mse"):
            raise ValueError(f"kind must be 'mae' or 'mse', not {kind!r}")
        self.kind, self.charge = kind, charge

    def _mean(self, pred, target, counts):
        _require_gpu(pred)
        n = int(counts.sum())
        if pred.numel() != n or target.numel() != n:
            raise ValueError(f"prediction and target have {pred.numel()} / {target.numel()} entries, the pointer counts {n}")
        d = pred.reshape(-1).to(torch.float64) - target.reshape(-1).to(torch.float64).detach()
        return torch.sum(_molecule_mean_weights(counts, pred.device) * (d.abs() if self.kind == "mae" else d * d))


class DensityMatrixLoss(_PackedMeanLoss):
    """``kind`` "mae" | "mse" of packed density matrices: the mean over the ``m^2`` entries of each molecule, then the mean over the molecules.  ``charge`` is what
    ``QHNetDensityLightning`` counts the occupied orbitals with."""

    def forward(self, D_pred: torch.Tensor, D_target: torch.Tensor, orb_ptr) -> torch.Tensor:
        m = np.diff(_orb_ptr_of(orb_ptr))
        return self._mean(D_pred, D_target, m * m)


class MullikenChargeLoss(_PackedMeanLoss):
    """``kind`` "mae" | "mse" of Mulliken charges (or populations) per atom: the mean over the atoms of each molecule, then the mean over the molecules.
    ``mol_ptr`` [B+1]: the atoms of every molecule (the batch's ``ptr``)."""

    def forward(self, q_pred: torch.Tensor, q_target: torch.Tensor, mol_ptr) -> torch.Tensor:
        return self._mean(q_pred, q_target, np.diff(_orb_ptr_of(mol_ptr)))


class QHNetDensityLightning(QHNetOrbitalLightning):
    """``QHNetOrbitalLightning`` with terms on the occupied subspace: ``losses`` / ``loss_coefs`` take ``"density_matrix"`` (a ``DensityMatrixLoss``) and
    ``"mulliken_charges"`` (a ``MullikenChargeLoss``) beside ``"hamiltonian"`` and ``"orbital_energies"``.  A step solves the packed prediction ONCE
    (``orbital_solution``; ``orbital_energies`` when no density is asked for) and the packed target once, detached, however many of the three keys are active;
    densities, populations under ``batch.overlap`` and charges ``Z - pop`` come from those two solutions.  The occupied orbitals are counted with the ``charge``
    of the active losses, which must agree.  With all three coefficients at 0 (or without the keys) nothing is solved and the step is ``QHNetLightning``'s."""

    KEYS = ("orbital_energies", "density_matrix", "mulliken_charges")

    def _active(self):
        return [k for k in self.KEYS if k in self.hparams.losses and self.hparams.loss_coefs.get(k, 0) != 0]

    def _evaluate(self, batch):
        if not self._packed():
            raise ValueError("QHNetDensityLightning needs packed losses (HamiltonianLoss, OrbitalEnergyLoss, DensityMatrixLoss, MullikenChargeLoss)")
        preds, targets, loss_args = QHNetLightning._evaluate(self, batch)
        active = self._active()
        if not active:
            return preds, targets, loss_args
        charges = [getattr(self.hparams.losses[k], "charge", 0) for k in active]
        if any(not np.array_equal(np.asarray(c), np.asarray(charges[0])) for c in charges[1:]):
            raise ValueError("the orbital losses count the occupied orbitals with different charges")
        plan, asm = self.net.last_plan, self.net._asm
        overlap = getattr(batch, "overlap", None)
        S = None if overlap is None else asm.pack_targets(plan, overlap)
        op = _orb_ptr_of(plan)
        n_occ = occupied_counts(batch.z, batch.ptr, charges[0], op)
        Hp, Ht = preds["hamiltonian"], targets["hamiltonian"]
        sol_t = BatchedOrbitals(op, Hp.device).solve(Ht, S)
        if active == ["orbital_energies"]:
            eps, sol_p = orbital_energies(Hp, S, op, return_solution=True)
        else:
            eps, D, sol_p = orbital_solution(Hp, S, op, n_occ, return_solution=True)
            D_t = sol_t.density(n_occ)
        for k in active:
            if k == "orbital_energies":
                preds[k], targets[k], preds[k + "_args"] = eps, sol_t.energies, (n_occ, op)
            elif k == "density_matrix":
                preds[k], targets[k], preds[k + "_args"] = D, D_t, (op,)
            else:
                preds[k] = mulliken_charges(batch.z, populations(D, plan, S, None, sol_p)[0])
                targets[k] = mulliken_charges(batch.z, sol_t.populations(D_t, plan, S)[0])
                preds[k + "_args"] = (batch.ptr,)
        return preds, targets, loss_args

    def _calculate_loss(self, y_pred, y_true, *loss_args):
        active, total = self._active(), 0
        for name, fn in self.hparams.losses.items():
            if name in self.KEYS:
                if name in active:
                    total = total + self.hparams.loss_coefs[name] * fn(y_pred[name], y_true[name], *y_pred[name + "_args"])
            else:
                total = total + self.hparams.loss_coefs[name] * fn(y_pred[name], y_true[name], *loss_args)
        return total


class _BondOrders(torch.autograd.Function):
    """Forward: ``nq_orb_bond_product`` and ``nq_orb_bond_reduce``.  Backward: ``nq_orb_bond_backward`` (``E`` elementwise, then ``sym(E S)`` and, where ``S``
    asks for it, ``sym(D E)`` in one launch); nothing is launched without an upstream gradient."""

    @staticmethod
    def forward(ctx, orb, plan, D, S):
        ctx.set_materialize_grads(False)
        bond, valence, Pm = orb.bond_orders(D, plan, S)
        ctx.orb, ctx.plan = orb, plan
        ctx.save_for_backward(D, S, Pm)
        ctx.s = None if S is None else (S.shape, S.dtype)
        return bond, valence

    @staticmethod
    def backward(ctx, g_bond, g_valence):
        D, S, Pm = ctx.saved_tensors
        want_d = ctx.needs_input_grad[2]
        want_s = ctx.s is not None and ctx.needs_input_grad[3]
        if (g_bond is None and g_valence is None) or not (want_d or want_s):
            return None, None, None, None
        f64 = lambda g: None if g is None else g.to(torch.float64).reshape(-1).contiguous()
        gD, gS = ctx.orb.bond_orders_backward(ctx.plan, f64(g_bond), f64(g_valence), Pm, D if want_s else None, S, want_d, want_s)
        return None, None, gD.view(D.shape) if want_d else None, gS.to(ctx.s[1]).view(ctx.s[0]) if want_s else None


def bond_orders(D: torch.Tensor, plan, S_packed: Optional[torch.Tensor] = None, orbitals: Optional[BatchedOrbitals] = None):
    """Differentiable Mayer bond orders and atomic valences of a packed float64 closed-shell density (carrying the factor 2) -> ``(bond [Q], valence [N])``,
    float64 on the device: with ``P = D S``, ``B_AB = sum_{mu in A, nu in B} P_mu,nu P_nu,mu`` over the ``n^2`` ordered atom pairs of every molecule, ``B_AA``
    included (``bond_layout`` / ``dense_bond_orders`` give a molecule's ``[n, n]`` table, exactly symmetric), and ``V_A = sum_{B != A} B_AB``.  ``S_packed = None``:
    the Wiberg index of an orthogonal basis.  Gradients for ``D`` and, where it requires one, ``S_packed`` (a float32 ``S`` gets a float32 gradient), with respect
    to SYMMETRIC matrices, spread over both triangles (the convention of this module): ``dL/dD = sym(E S)``, ``dL/dS = sym(D E)`` with
    ``E_mu,nu = (Gamma_AB + Gamma_BA) P_nu,mu`` and ``Gamma_AB = g_bond_AB + (A != B) g_valence_A``.  On the ``D`` of ``orbital_solution`` / ``smeared_solution``
    / ``purified_density_matrix`` the gradients flow on to ``H`` and ``S`` through their response chains.  ``orbitals``: the solution (or purification) of the
    same batch, whose state the kernels read the layout from (None: one is prepared, which synchronises the stream once).  Limits: closed shells, at most 32
    orbitals per atom (NaN in that atom's row and column), 1..1024 orbitals per molecule.  The Löwdin counterpart (the Wiberg index of the symmetrically
    orthogonalised density) is ``lowdin_bond_orders``."""
    _require_gpu(D)
    orb = BatchedOrbitals(plan, D.device) if orbitals is None else orbitals
    return _BondOrders.apply(orb, plan, D, S_packed)


class BondOrderLoss(_PackedMeanLoss):
    """``kind`` "mae" | "mse" of bond-order tables: the mean over the ``n^2`` entries of each molecule, then the mean over the molecules.  ``mol_ptr`` [B+1]: the
    atoms of every molecule (the batch's ``ptr``).  ``charge`` is what ``QHNetBondOrderLightning`` counts the occupied orbitals with."""

    def forward(self, b_pred: torch.Tensor, b_target: torch.Tensor, mol_ptr) -> torch.Tensor:
        n = np.diff(_orb_ptr_of(mol_ptr))
        return self._mean(b_pred, b_target, n * n)


class QHNetBondOrderLightning(QHNetDensityLightning):
    """``QHNetDensityLightning`` with a term on the Mayer bond orders: ``losses`` / ``loss_coefs`` take ``"bond_orders"`` (a ``BondOrderLoss``) beside the parent's
    keys.  The bond orders of the prediction (``bond_orders`` of the density of ``orbital_solution``, under ``batch.overlap``) and of the detached target come
    from the SAME single solve of each that serves the parent's keys.  With the coefficient at 0 (or without the key) the step is the parent's."""

    BOND = "bond_orders"
    KEYS = QHNetDensityLightning.KEYS + (BOND,)

    def _solved_sides(self, batch, active, who: str, packed_names: str, need_overlap: bool = False):
        """What every step with a density term does once, shared with the subclasses: the parent's packed matrices, the charges check, ONE
        ``orbital_solution`` of the prediction and ONE detached solve of the target -> ``(preds, targets, loss_args, c)`` with
        ``c = (plan, S, op, n_occ, eps, D, sol_p, sol_t, D_t)``."""
        if not self._packed():
            raise ValueError(f"{who} needs packed losses ({packed_names})")
        preds, targets, loss_args = QHNetLightning._evaluate(self, batch)
        charges = [getattr(self.hparams.losses[k], "charge", 0) for k in active]
        if any(not np.array_equal(np.asarray(c), np.asarray(charges[0])) for c in charges[1:]):
            raise ValueError("the orbital losses count the occupied orbitals with different charges")
        plan, asm = self.net.last_plan, self.net._asm
        overlap = getattr(batch, "overlap", None)
        if overlap is None and need_overlap:
            raise ValueError(f"{who}: the Löwdin terms need batch.overlap (without an overlap they are the parent's Mulliken and Mayer terms)")
        S = None if overlap is None else asm.pack_targets(plan, overlap)
        op = _orb_ptr_of(plan)
        n_occ = occupied_counts(batch.z, batch.ptr, charges[0], op)
        Hp, Ht = preds["hamiltonian"], targets["hamiltonian"]
        sol_t = BatchedOrbitals(op, Hp.device).solve(Ht, S)
        eps, D, sol_p = orbital_solution(Hp, S, op, n_occ, return_solution=True)
        D_t = sol_t.density(n_occ)
        return preds, targets, loss_args, (plan, S, op, n_occ, eps, D, sol_p, sol_t, D_t)

    def _fill(self, k, preds, targets, batch, c):
        """The entries of one of this class's keys from the two solutions."""
        plan, S, op, n_occ, eps, D, sol_p, sol_t, D_t = c
        if k == "orbital_energies":
            preds[k], targets[k], preds[k + "_args"] = eps, sol_t.energies, (n_occ, op)
        elif k == "density_matrix":
            preds[k], targets[k], preds[k + "_args"] = D, D_t, (op,)
        elif k == "mulliken_charges":
            preds[k] = mulliken_charges(batch.z, populations(D, plan, S, None, sol_p)[0])
            targets[k] = mulliken_charges(batch.z, sol_t.populations(D_t, plan, S)[0])
            preds[k + "_args"] = (batch.ptr,)
        else:
            preds[k], targets[k], preds[k + "_args"] = bond_orders(D, plan, S, sol_p)[0], sol_t.bond_orders(D_t, plan, S)[0], (batch.ptr,)

    def _evaluate(self, batch):
        active = self._active()
        if self.BOND not in active:
            return super()._evaluate(batch)
        preds, targets, loss_args, c = self._solved_sides(batch, active, "QHNetBondOrderLightning",
                                                          "HamiltonianLoss, OrbitalEnergyLoss, DensityMatrixLoss, MullikenChargeLoss, BondOrderLoss")
        for k in active:
            self._fill(k, preds, targets, batch, c)
        return preds, targets, loss_args

class _LowdinBasis(torch.autograd.Function):
    """Forward: ONE standard solve of ``S``, ``nq_orb_low_weights`` and ONE ``nq_orb_wgram`` launch.  Backward: per output WITH an upstream gradient the chain
    ``nq_orb_resp_project`` -> ``nq_orb_low_mo`` -> ``nq_orb_smear_back`` -> ``nq_orb_syr2k`` over all orbital pairs; nothing is launched for an output without."""

    @staticmethod
    def forward(ctx, orb, S):
        orb.solve(S)
        ctx.set_materialize_grads(False)
        half, inv_half, cond, info = orb.overlap_functions()
        ctx.orb = orb
        ctx.s = (S.shape, S.dtype)
        ctx.mark_non_differentiable(cond, info)
        return half, inv_half, cond, info

    @staticmethod
    def backward(ctx, g_half, g_inv, g_cond, g_info):
        if (g_half is None and g_inv is None) or not ctx.needs_input_grad[1]:
            return None, None
        gS = None
        for kind, g in ((0, g_half), (1, g_inv)):
            if g is not None:
                r = ctx.orb.matfun_response(g.to(torch.float64).reshape(-1).contiguous(), kind)
                gS = r if gS is None else gS + r
        return None, gS.to(ctx.s[1]).view(ctx.s[0])


def lowdin_basis(S_packed: torch.Tensor, plan_or_orb_ptr) -> LowdinBasis:
    """The symmetric orthogonalisation of every molecule of a batch -> ``LowdinBasis`` whose ``half`` = ``S^(1/2)`` and ``inv_half`` = ``S^(-1/2)`` (packed
    float64 [P], exactly symmetric) carry gradients back to ``S_packed`` (a float32 ``S`` gets a float32 gradient, a symmetric matrix in the convention of
    ``orbital_energies``).  One standard solve of ``S`` (latency-bound: the dominant cost), ``nq_orb_low_weights`` and one ``nq_orb_wgram`` launch; the backward
    is the Daleckii-Krein form of the module text, which divides no difference of levels, and launches nothing for an output without an upstream gradient.
    ``plan_or_orb_ptr`` as for ``BatchedOrbitals``.  One basis serves prediction and target of a step; ``S`` belongs to the conformer, so it can be cached
    across epochs (``LowdinBasis.of`` builds one without gradients).  ``S`` must be positive definite: otherwise ``info = 1`` and NaN in that molecule's
    blocks, which ``check()`` reports.  The gradient of ``S`` needs the decomposition; without one, and without that gradient, ``LowdinBasis.of(...,
    method="newton_schulz")`` gives the two functions from matrix products alone."""
    _require_gpu(S_packed)
    orb = BatchedOrbitals(plan_or_orb_ptr, S_packed.device)
    return LowdinBasis(orb, *_LowdinBasis.apply(orb, S_packed))


class _Congruence(torch.autograd.Function):
    """Forward: ``Y = M X`` (``nq_orb_low_product``) and ``M^L = sym(X Y)`` (``nq_orb_low_symprod``).  Backward for ``G = dL/dM^L``, made symmetric first on the device (``nq_orb_low_symmetrize``):
    ``dL/dM = sym(X (G X))`` (two launches) and ``dL/dX = 2 sym(Y G)`` (one); a half nobody asks for is skipped, nothing is launched without ``G``."""

    @staticmethod
    def forward(ctx, orb, M, X):
        ctx.set_materialize_grads(False)
        ML, Y = orb.sym_congruence(X, M)
        ctx.orb = orb
        ctx.m = (M.shape, M.dtype)
        ctx.save_for_backward(X, Y)
        return ML

    @staticmethod
    def backward(ctx, G):
        X, Y = ctx.saved_tensors
        want_m, want_x = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if G is None or not (want_m or want_x):
            return None, None, None
        # the products read the lower triangle of a symmetric G: one nq_orb_low_symmetrize launch first, whatever the upstream hands over
        gM, gX = ctx.orb.sym_congruence_backward(G.to(torch.float64).reshape(-1).contiguous(), X, Y, want_m, want_x, symmetric=False)
        return None, gM.to(ctx.m[1]).view(ctx.m[0]) if want_m else None, gX.view(X.shape) if want_x else None


def _congruence(M, which, basis, name):
    _require_gpu(M)
    if not isinstance(basis, LowdinBasis):
        raise TypeError(f"{name}: basis must be a LowdinBasis (lowdin_basis(S_packed, plan)), not {type(basis).__name__}")
    P = basis.orbitals.state.P
    if M.numel() != P:
        raise ValueError(f"{name}: the matrix has {M.numel()} entries, the basis packs {P}")
    return _Congruence.apply(basis.orbitals, M, getattr(basis, which))


def lowdin_density(D: torch.Tensor, basis: LowdinBasis) -> torch.Tensor:
    """The Löwdin density ``D^L = S^(1/2) D S^(1/2)`` of a packed symmetric density (float32 or float64; its lower triangle is read) -> packed float64 [P],
    exactly symmetric, with gradients for ``D`` and, through ``basis.half``, for the ``S`` of ``lowdin_basis``."""
    return _congruence(D, "half", basis, "lowdin_density")


def lowdin_hamiltonian(H: torch.Tensor, basis: LowdinBasis) -> torch.Tensor:
    """The Löwdin-orthogonalised Hamiltonian ``H^L = S^(-1/2) H S^(-1/2)`` (float32 or float64 ``H``; its lower triangle is read) -> packed float64 [P], exactly
    symmetric; its eigenvalues are the generalised orbital energies.  Gradients for ``H`` (cast to its dtype) and, through ``basis.inv_half``, for ``S``."""
    return _congruence(H, "inv_half", basis, "lowdin_hamiltonian")


def lowdin_populations(D: torch.Tensor, plan, basis: LowdinBasis):
    """Löwdin populations of a packed closed-shell density -> ``(atom_pop [N], nelec [B], None)``: ``populations(lowdin_density(D, basis), plan, None)``, that is
    ``q_A = sum_{mu in A} D^L_mu,mu`` and ``nelec = Tr(D^L) = Tr(D S)``; differentiable with respect to ``D`` and ``S``."""
    return populations(lowdin_density(D, basis), plan, None, None, basis.orbitals)


def lowdin_charges(z, atom_pop: torch.Tensor) -> torch.Tensor:
    """Löwdin charges ``Z_A - q_A`` from ``lowdin_populations`` (the arithmetic of ``mulliken_charges``)."""
    return mulliken_charges(z, atom_pop)


def lowdin_bond_orders(D: torch.Tensor, plan, basis: LowdinBasis):
    """Wiberg indices in the Löwdin basis and the valences -> ``(bond [Q], valence [N])``: ``bond_orders(lowdin_density(D, basis), plan, None)``, that is
    ``W_AB = sum_{mu in A, nu in B} (D^L_mu,nu)^2``; for an idempotent closed-shell density ``sum_B W_AB = 2 q_A``.  Differentiable with respect to ``D`` and
    ``S``.  Limits: closed shells only, at most 32 orbitals per atom (NaN in that atom's row and column), ``S`` positive definite, 1..1024 orbitals."""
    return bond_orders(lowdin_density(D, basis), plan, None, basis.orbitals)


class LowdinChargeLoss(_PackedMeanLoss):
    """``kind`` "mae" | "mse" of Löwdin charges (or populations) per atom: the mean over the atoms of each molecule, then the mean over the molecules.
    ``mol_ptr`` [B+1]: the atoms of every molecule (the batch's ``ptr``).  ``charge`` is what ``QHNetLowdinLightning`` counts the occupied orbitals with."""

    def forward(self, q_pred: torch.Tensor, q_target: torch.Tensor, mol_ptr) -> torch.Tensor:
        return self._mean(q_pred, q_target, np.diff(_orb_ptr_of(mol_ptr)))


class QHNetLowdinLightning(QHNetBondOrderLightning):
    """``QHNetBondOrderLightning`` with terms in the Löwdin basis: ``losses`` / ``loss_coefs`` take ``"lowdin_charges"`` (a ``LowdinChargeLoss``) and
    ``"lowdin_bond_orders"`` (a ``BondOrderLoss``) beside the parent's keys.  A step makes ONE ``lowdin_basis`` of ``batch.overlap`` (required), shared by the
    prediction and the detached target; the densities come from the SAME single solve of each that serves the parent's keys.  With both coefficients at 0 (or
    without the keys) the step is the parent's."""

    LOWDIN = ("lowdin_charges", "lowdin_bond_orders")
    KEYS = QHNetBondOrderLightning.KEYS + LOWDIN

    def _evaluate(self, batch):
        active = self._active()
        if not any(k in active for k in self.LOWDIN):
            return super()._evaluate(batch)
        preds, targets, loss_args, c = self._solved_sides(batch, active, "QHNetLowdinLightning",
                                                          "HamiltonianLoss, OrbitalEnergyLoss, DensityMatrixLoss, MullikenChargeLoss, BondOrderLoss, LowdinChargeLoss",
                                                          need_overlap=True)
        plan, S, op, n_occ, eps, D, sol_p, sol_t, D_t = c
        basis = lowdin_basis(S, op)                                # one decomposition of S per step, for both sides
        for k in active:
            if k == "lowdin_charges":
                preds[k] = lowdin_charges(batch.z, lowdin_populations(D, plan, basis)[0])
                targets[k] = lowdin_charges(batch.z, lowdin_populations(D_t, plan, basis)[0]).detach()
                preds[k + "_args"] = (batch.ptr,)
            elif k == "lowdin_bond_orders":
                preds[k], targets[k], preds[k + "_args"] = lowdin_bond_orders(D, plan, basis)[0], lowdin_bond_orders(D_t, plan, basis)[0].detach(), (batch.ptr,)
            else:
                self._fill(k, preds, targets, batch, c)
        return preds, targets, loss_args


class _Commutator(torch.autograd.Function):
    """Forward: ONE ``nq_orb_comm_product`` launch.  Backward for ``G = dL/dC``: ``G_a = (G - G^T) / 2`` (``nq_orb_comm_antisymmetrize``), then
    ``dL/dX = [G_a, Y]`` and ``dL/dY = [X, G_a]``, the same kernel with an antisymmetric first operand; a half nobody asks for is skipped, nothing is launched
    without ``G``."""

    @staticmethod
    def forward(ctx, orb, X, Y):
        ctx.set_materialize_grads(False)
        ctx.orb = orb
        ctx.save_for_backward(X, Y)
        return orb.commutator(X, Y).view(X.shape)

    @staticmethod
    def backward(ctx, G):
        X, Y = ctx.saved_tensors
        want_x, want_y = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if G is None or not (want_x or want_y):
            return None, None, None
        orb = ctx.orb
        Ga = orb.antisymmetrize(G.to(torch.float64).reshape(-1).contiguous())
        gX = orb.commutator(Ga, Y, True, 1.0).view(X.shape) if want_x else None
        gY = orb.commutator(Ga, X, True, -1.0).view(Y.shape) if want_y else None
        return None, gX, gY


def commutator(X: torch.Tensor, Y: torch.Tensor, orbitals) -> torch.Tensor:
    """``C = X Y - Y X`` per molecule for packed float64 [P] SYMMETRIC ``X`` and ``Y`` (their lower triangles are read) -> packed float64 [P], exactly
    antisymmetric with a ``+0.0`` diagonal, differentiable with respect to both.  ``orbitals``: a ``BatchedOrbitals`` or ``BatchedPurification`` of the batch;
    only its layout is read, nothing has to be solved.  The gradients are symmetric matrices (the convention of ``orbital_energies``):
    ``dL/dX = [G_a, Y]``, ``dL/dY = [X, G_a]`` with ``G_a`` the antisymmetric part of the upstream gradient, whose symmetric part cannot reach a
    commutator of symmetric matrices.  One launch forward, one plus one per gradient backward (csrc/orbcomm.hip), bitwise reproducible."""
    if not isinstance(orbitals, (BatchedOrbitals, BatchedPurification)):
        raise TypeError(f"commutator: orbitals must be a BatchedOrbitals or a BatchedPurification of the batch, not {type(orbitals).__name__}")
    _require_gpu(X)
    _require_gpu(Y)
    P = orbitals.state.P
    for name, t in (("X", X), ("Y", Y)):
        if t.dtype != torch.float64:
            raise TypeError(f"commutator: {name} must be float64, not {t.dtype}")
        if t.numel() != P:
            raise ValueError(f"commutator: {name} has {t.numel()} entries, the batch packs {P}")
    return _Commutator.apply(orbitals, X, Y)


def scf_residual(H: torch.Tensor, D: torch.Tensor, basis: LowdinBasis) -> torch.Tensor:
    """The SCF residual (the DIIS error vector) of a Hamiltonian and a density in the Löwdin basis, ``R^L = [H^L, D^L]`` with ``H^L = S^(-1/2) H S^(-1/2)`` and
    ``D^L = S^(1/2) D S^(1/2)``, which is ``S^(-1/2) (H D S - S D H) S^(-1/2)``: ``commutator(lowdin_hamiltonian(H, basis), lowdin_density(D, basis),
    basis.orbitals)`` -> packed float64 [P], exactly antisymmetric.  ``H`` and ``D`` packed symmetric, float32 or float64 (their lower triangles are read);
    ``basis`` a ``LowdinBasis``.  Differentiable with respect to ``H`` and ``D``, and to ``S`` when the basis came from ``lowdin_basis``.

    ``R^L = 0`` holds exactly when ``D`` is a stationary density of ``H``.  For an idempotent closed-shell ``D`` (``D^L = 2 Q``, ``Q`` a projector) and any
    ``H``: ``sum_ij (R^L_ij)^2 = 8 sum_{i occ, a virt} h_ia^2`` with ``h_ia`` the occupied-virtual block of ``H^L`` in the orbitals of ``D``: the block that
    rotates the occupied subspace.  Nothing is solved, iterated or divided for ``H``: the residual is linear in ``H``, its gradient is one more commutator,
    and it stays finite where the HOMO and LUMO of ``H`` coincide or cross, where ``orbital_solution`` does not.

    Limits: ``S`` must be positive definite (``info = 1`` and NaN in that molecule's blocks otherwise); 1..1024 orbitals per molecule; the raw AO form
    ``H D S - S D H`` without a basis is out of scope.  The residual measures the occupied-virtual coupling WITHOUT gap weighting: it is not
    ``D_pred - D_target``, and it says nothing about the order of the levels inside the occupied space."""
    HL = _congruence(H, "inv_half", basis, "scf_residual")
    DL = _congruence(D, "half", basis, "scf_residual")
    return commutator(HL, DL, basis.orbitals)


def scf_residual_to_target(H: torch.Tensor, target) -> torch.Tensor:
    """``scf_residual`` of ``H`` against a cached ``ScfTarget``: ``commutator(lowdin_hamiltonian(H, target.basis), target.DL, target.basis.orbitals)``: the
    target's half is already in the Löwdin basis, so a step is two congruence products and one commutator; differentiable with respect to ``H``."""
    basis, DL = target
    return commutator(_congruence(H, "inv_half", basis, "scf_residual_to_target"), DL, basis.orbitals)


class ScfResidualLoss(_PackedMeanLoss):
    """``kind`` "mse" | "mae" of a packed SCF residual against zero: the mean over the ``m^2`` entries of each molecule, then the mean over the molecules.
    ``R_target``: None (zero: the stationary density) or a packed residual.  ``charge`` is what ``QHNetCommutatorLightning`` counts the occupied orbitals of
    the target with, ``target_method`` ("solve" | "iterative") whether it builds an uncached target by ``scf_target`` or ``scf_target_iterative``."""

    def __init__(self, kind: str = "mae", charge=0, target_method: str = "solve"):
        super().__init__(kind, charge)
        if target_method not in ("solve", "iterative"):
            raise ValueError(f"target_method must be 'solve' or 'iterative', not {target_method!r}")
        self.target_method = target_method

    def forward(self, R_pred: torch.Tensor, R_target: Optional[torch.Tensor], orb_ptr) -> torch.Tensor:
        m = np.diff(_orb_ptr_of(orb_ptr))
        return self._mean(R_pred, torch.zeros_like(R_pred) if R_target is None else R_target, m * m)


class ScfTarget(namedtuple("ScfTarget", "basis DL")):
    """What the residual term needs of a batch beside the prediction, detached, cacheable across epochs (both belong to the conformer): ``basis``, the
    ``LowdinBasis`` of its overlap, and ``DL``, the target's Löwdin density ``S^(1/2) D S^(1/2)`` packed float64 [P].  ``purification``: the
    ``BatchedPurification`` behind ``DL`` for ``scf_target_iterative``, else None.  ``check()`` reads the status words once (a host synchronisation)
    and raises ``RuntimeError`` naming the molecule whose overlap is not positive definite or whose target has no gap."""

    purification = None

    def check(self) -> "ScfTarget":
        if self.basis.info is not None or self.basis.root is not None:
            self.basis.check()
        if self.purification is not None:
            self.purification.check()
        return self


def scf_target(H_target: torch.Tensor, S: torch.Tensor, plan, n_occ) -> ScfTarget:
    """``ScfTarget`` of a batch from ONE solve of the target Hamiltonian under ``S`` (its closed-shell density of ``n_occ`` [B] doubly occupied orbitals) and ONE
    ``LowdinBasis.of(S, plan)``, both latency-bound; no gradient flows through.  ``plan``: a plan or ``orb_ptr`` as for ``BatchedOrbitals``.
    ``scf_target_iterative`` builds the same target without any solve."""
    _require_gpu(H_target)
    _require_gpu(S)
    op = _orb_ptr_of(plan)
    basis = LowdinBasis.of(S.detach(), op)
    D = BatchedOrbitals(op, H_target.device).solve(H_target.detach(), S.detach()).density(n_occ)
    return ScfTarget(basis, basis.orbitals.sym_congruence(basis.half, D)[0])


def scf_target_iterative(H_target: torch.Tensor, S: torch.Tensor, plan, n_occ, max_iter: int = 100) -> ScfTarget:
    """The ``ScfTarget`` of ``scf_target`` with NOTHING solved; no gradient flows through.  ``S^(1/2)`` and ``S^(-1/2)`` by Newton-Schulz
    (``LowdinBasis.of(..., method="newton_schulz", max_iter=max_iter)``), ``H^L = S^(-1/2) H S^(-1/2)`` by one congruence, the projector ``X`` on its ``n_occ``
    lowest levels by SP2 purification of that STANDARD problem (``BatchedPurification``, at most ``max_iter`` iterations), ``D^L = 2 X`` with no back-transform.
    A target without a gap (status 4) or an overlap that is not positive definite gives NaN in that molecule's blocks only and is named by
    ``ScfTarget.check()``."""
    _require_gpu(H_target)
    _require_gpu(S)
    op = _orb_ptr_of(plan)
    no = check_occupied(n_occ, op)
    basis = LowdinBasis.of(S.detach(), op, method="newton_schulz", max_iter=max_iter)
    HL = basis.orbitals.sym_congruence(basis.inv_half, H_target.detach())[0]
    pur = BatchedPurification(op, H_target.device).purify(HL, no, max_iter)
    target = ScfTarget(basis, pur.density())
    target.purification = pur
    return target


def scf_target_blocks(target) -> dict:
    """The three fields ``QHNetCommutatorLightning`` reads from a batch (its ``CACHED``), from an ``ScfTarget``: ``{"lowdin_inv_half", "lowdin_half",
    "target_density_lowdin"}``, each a list of per-molecule float64 ``[m, m]`` CPU tensors, for a data pipeline to store with the conformer.  One device -> host
    copy per field."""
    basis, DL = target
    pp, m = basis.orbitals.pack_ptr, np.diff(basis.orbitals.orb_ptr)
    out = {}
    for name, t in (("lowdin_inv_half", basis.inv_half), ("lowdin_half", basis.half), ("target_density_lowdin", DL)):
        flat = t.detach().to(torch.float64).reshape(-1).cpu()
        out[name] = [flat[int(pp[b]):int(pp[b + 1])].reshape(int(m[b]), int(m[b])).clone() for b in range(m.shape[0])]
    return out


def _pack_f64(blocks, P: int, device, name: str) -> torch.Tensor:
    flat = np.concatenate([np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64).reshape(-1) for b in blocks])
    if flat.size != P:
        raise ValueError(f"batch.{name} holds {flat.size} elements, the batch packs {P}")
    return torch.from_numpy(flat).to(device)


class QHNetCommutatorLightning(QHNetLowdinLightning):
    """``QHNetLowdinLightning`` with a term on the SCF residual: ``losses`` / ``loss_coefs`` take ``"scf_residual"`` (an ``ScfResidualLoss``) beside the parent's
    keys: ``scf_residual`` of the packed prediction against the target's Löwdin density, against zero.  When that key is the only active orbital key the step
    solves NOTHING for the prediction.  If the batch carries ``batch.lowdin_inv_half``, ``batch.lowdin_half`` and ``batch.target_density_lowdin`` (lists of
    per-molecule float64 matrices like ``batch.hamiltonian``: what ``scf_target`` computes, cached with the conformer), they are packed and used, and the step
    launches no solve at all; otherwise it computes ``scf_target`` from ``batch.hamiltonian`` and ``batch.overlap`` (required): one target solve and one
    decomposition of ``S``, both detached, or, with ``ScfResidualLoss(target_method="iterative")``, matrix products alone.  Beside other active keys the parent's step runs unchanged and the residual term is added to it.  With the
    coefficient at 0 (or without the key) the step is the parent's."""

    SCF = "scf_residual"
    KEYS = QHNetLowdinLightning.KEYS + (SCF,)
    CACHED = ("lowdin_inv_half", "lowdin_half", "target_density_lowdin")
    _scf_hidden = False

    def _active(self):
        active = super()._active()
        return [k for k in active if k != self.SCF] if self._scf_hidden else active

    def _evaluate(self, batch):
        if self.SCF not in self._active():
            return super()._evaluate(batch)
        if not self._packed():
            raise ValueError("QHNetCommutatorLightning needs packed losses (HamiltonianLoss, ScfResidualLoss and the parent's)")
        self._scf_hidden = True                                    # the parent's step sees its own keys only (none: QHNetLightning's step, nothing solved)
        try:
            preds, targets, loss_args = super()._evaluate(batch)
        finally:
            self._scf_hidden = False
        plan, asm = self.net.last_plan, self.net._asm
        op = _orb_ptr_of(plan)
        Hp = preds["hamiltonian"]
        cached = [getattr(batch, n, None) for n in self.CACHED]
        if all(c is not None for c in cached):
            P = Hp.numel()
            inv_half, half, DL = (_pack_f64(c, P, Hp.device, n) for c, n in zip(cached, self.CACHED))
            target = ScfTarget(LowdinBasis(BatchedOrbitals(op, Hp.device), half, inv_half, None, None), DL)
        else:
            overlap = getattr(batch, "overlap", None)
            if overlap is None:
                raise ValueError("QHNetCommutatorLightning: the residual term needs batch.overlap, or the cached batch.lowdin_inv_half / lowdin_half / "
                                 "target_density_lowdin")
            loss = self.hparams.losses[self.SCF]
            build = scf_target_iterative if getattr(loss, "target_method", "solve") == "iterative" else scf_target
            target = build(targets["hamiltonian"], asm.pack_targets(plan, overlap), op, occupied_counts(batch.z, batch.ptr, getattr(loss, "charge", 0), op))
        k = self.SCF
        preds[k], targets[k], preds[k + "_args"] = scf_residual_to_target(Hp, target), None, (op,)
        return preds, targets, loss_args


SmearedSolution = namedtuple("SmearedSolution", "eps D occ mu entropy")
SmearedSolution.__doc__ = """What ``smeared_solution`` returns, float64 on the device: ``eps`` [M], ``D`` [P], ``occ`` = F [M], ``mu`` [B], ``entropy`` [B] (units of k_B)."""


class _SmearedSolution(torch.autograd.Function):
    """Forward: ONE ``BatchedOrbitals.solve``, ``fermi`` and the density of its occupations.  Backward: the chain of ``BatchedOrbitals.smeared_response`` for
    whatever upstream gradients there are -- ``nq_orb_wgram`` alone where only ``eps`` has one; the two launches that serve ``D`` are skipped without one for
    ``D``; nothing is launched without any, and the ``S`` half is skipped when ``S`` asks for nothing."""

    @staticmethod
    def forward(ctx, orb, H, S, n_elec, kT):
        orb.solve(H, S)
        ctx.set_materialize_grads(False)
        fr = orb.fermi(n_elec, kT)
        ctx.orb, ctx.fermi = orb, fr
        ctx.h = (H.shape, H.dtype)
        ctx.s = None if S is None else (S.shape, S.dtype)
        return orb.energies.clone(), orb.smeared_density(fr.occ), fr.occ.clone(), fr.mu.clone(), fr.entropy.clone()

    @staticmethod
    def backward(ctx, g_eps, g_D, g_occ, g_mu, g_ent):
        orb = ctx.orb
        want_h = ctx.needs_input_grad[1]
        want_s = ctx.s is not None and ctx.needs_input_grad[2]
        gs = [g_eps, g_D, g_occ, g_mu, g_ent]
        if all(g is None for g in gs) or not (want_h or want_s):
            return None, None, None, None, None
        g_eps, g_D, g_occ, g_mu, g_ent = [None if g is None else g.to(torch.float64).reshape(-1).contiguous() for g in gs]
        if g_D is None and g_occ is None and g_mu is None and g_ent is None:           # the energies alone: the eigenvalue term, one launch
            gH, gS = orb.weighted_gram(g_eps, -(orb.energies * g_eps)) if want_s else (orb.weighted_gram(g_eps), None)
        else:
            gH, gS = orb.smeared_response(g_D, ctx.fermi, g_eps, g_occ, g_mu, g_ent, overlap=want_s)
        return (None, gH.to(ctx.h[1]).view(ctx.h[0]) if want_h else None, gS.to(ctx.s[1]).view(ctx.s[0]) if want_s else None, None, None)


def smeared_solution(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, n_elec, kT, return_solution: bool = False):
    """Orbital energies, the Fermi-smeared density matrix, the occupations, the chemical potential and the electronic entropy of every molecule from ONE
    solve -> ``SmearedSolution(eps [M], D [P], occ [M], mu [B], entropy [B])``, float64 on the device (``return_solution=True``:
    ``(SmearedSolution, BatchedOrbitals)``); every member is differentiable with respect to ``H_packed`` and ``S_packed``.

    Arguments as for ``orbital_energies``; ``n_elec``: electrons per molecule (``electron_counts``; any number in (0, 2m), odd counts too), ``kT`` > 0: the
    smearing temperature in the energy unit of ``H``; each one number or one per molecule.  ``occ_k = 2 / (1 + exp((eps_k - mu) / kT))`` with ``mu`` fixed by
    ``sum occ = n_elec``, ``D = sum_k occ_k c_k c_k^T`` (packed like the input, exactly symmetric), ``entropy = -2 sum (f ln f + (1 - f) ln(1 - f))`` with
    ``f = occ / 2``; the band energy is ``populations(D, plan, S, H)[2]``.  The backward is ``C (K o W) C^T`` over all orbital pairs with the divided
    differences of the occupations, evaluated without dividing by a difference of orbital energies (module text): coincident and crossed levels, a vanishing
    HOMO-LUMO gap included, give finite gradients.  A member without an upstream gradient costs nothing, the ``S`` half is skipped when ``S`` is None or requires
    no gradient, and the gradients are cast to the inputs' dtypes in the symmetric-matrix convention of ``orbital_energies``.  Per-level losses on ``eps_k`` or
    ``occ_k`` are not differentiable where levels cross (the labels swap); losses on ``D``, ``mu``, ``entropy`` and symmetric functions of the levels are.  A
    molecule the solver fails on, or with ``n_elec`` outside (0, 2m) or ``kT`` not positive, yields NaN in its own blocks only
    (``BatchedOrbitals.check()`` reports both)."""
    _require_gpu(H_packed)
    if S_packed is not None:
        _require_gpu(S_packed)
    orb = BatchedOrbitals(plan_or_orb_ptr, H_packed.device)
    ne, kt = orb._per_molecule(n_elec, "n_elec"), orb._per_molecule(kT, "kT")
    out = SmearedSolution(*_SmearedSolution.apply(orb, H_packed, S_packed, ne, kt))
    return (out, orb) if return_solution else out


def smeared_density_matrix(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, n_elec, kT, return_solution: bool = False):
    """``smeared_solution`` without the rest -> ``D`` float64 [P] (``return_solution=True``: ``(D, BatchedOrbitals)``).  Like it, the backward is evaluated
    without dividing by a difference of orbital energies."""
    out = smeared_solution(H_packed, S_packed, plan_or_orb_ptr, n_elec, kT, return_solution)
    return (out[0].D, out[1]) if return_solution else out.D


class QHNetSmearedDensityLightning(QHNetDensityLightning):
    """``QHNetDensityLightning`` with Fermi-smeared occupations at the temperature ``kT`` (attribute; class default 0.01 Hartree, settable on the instance):
    the same keys, losses and constructor.  Prediction AND detached target are evaluated at the same ``kT`` (``smeared_solution`` / ``BatchedOrbitals.fermi``),
    so a perfect prediction has zero loss; electrons are counted with ``electron_counts`` and the ``charge`` of the active losses, odd counts included.  The
    gradients stay finite where the predicted HOMO and LUMO come close or cross, which is what lets training start from scratch; prefer the parent for
    fine-tuning a prediction whose gap is safely open.  ``OrbitalEnergyLoss`` selects "occupied" / "frontier" with ``ceil(n_elec / 2)`` levels.  With all three
    coefficients at 0 (or without the keys) nothing is solved and the step is ``QHNetLightning``'s."""

    kT = 0.01

    def _evaluate(self, batch):
        if not self._packed():
            raise ValueError("QHNetSmearedDensityLightning needs packed losses (HamiltonianLoss, OrbitalEnergyLoss, DensityMatrixLoss, MullikenChargeLoss)")
        preds, targets, loss_args = QHNetLightning._evaluate(self, batch)
        active = self._active()
        if not active:
            return preds, targets, loss_args
        charges = [getattr(self.hparams.losses[k], "charge", 0) for k in active]
        if any(not np.array_equal(np.asarray(c), np.asarray(charges[0])) for c in charges[1:]):
            raise ValueError("the orbital losses count the electrons with different charges")
        plan, asm = self.net.last_plan, self.net._asm
        overlap = getattr(batch, "overlap", None)
        S = None if overlap is None else asm.pack_targets(plan, overlap)
        op = _orb_ptr_of(plan)
        n_elec = electron_counts(batch.z, batch.ptr, charges[0], op)
        n_occ = torch.minimum(torch.ceil(n_elec / 2.0), torch.from_numpy(np.diff(op).astype(np.float64))).to(torch.int32)
        Hp, Ht = preds["hamiltonian"], targets["hamiltonian"]
        sol_t = BatchedOrbitals(op, Hp.device).solve(Ht, S)
        D_t = sol_t.smeared_density(sol_t.fermi(n_elec, self.kT).occ)
        sm, sol_p = smeared_solution(Hp, S, op, n_elec, self.kT, return_solution=True)
        for k in active:
            if k == "orbital_energies":
                preds[k], targets[k], preds[k + "_args"] = sm.eps, sol_t.energies, (n_occ, op)
            elif k == "density_matrix":
                preds[k], targets[k], preds[k + "_args"] = sm.D, D_t, (op,)
            else:
                preds[k] = mulliken_charges(batch.z, populations(sm.D, plan, S, None, sol_p)[0])
                targets[k] = mulliken_charges(batch.z, sol_t.populations(D_t, plan, S)[0])
                preds[k + "_args"] = (batch.ptr,)
        return preds, targets, loss_args


class _PurifiedDensity(torch.autograd.Function):
    """Forward: ``BatchedPurification.purify`` and ``density``.  Backward: ``BatchedPurification.response``; nothing is launched without an upstream gradient,
    and the ``S`` half is skipped when ``S`` asks for nothing."""

    @staticmethod
    def forward(ctx, pur, H, S, n_occ, orth, max_iter):
        pur.purify(H, n_occ, max_iter, orth)
        ctx.set_materialize_grads(False)
        ctx.pur = pur
        ctx.h = (H.shape, H.dtype)
        ctx.s = None if S is None else (S.shape, S.dtype)
        return pur.density()

    @staticmethod
    def backward(ctx, g_D):
        want_h = ctx.needs_input_grad[1]
        want_s = ctx.s is not None and ctx.needs_input_grad[2]
        if g_D is None or not (want_h or want_s):
            return None, None, None, None, None, None
        gH, gS = ctx.pur.response(g_D.to(torch.float64).reshape(-1).contiguous(), want_s)
        return (None, gH.to(ctx.h[1]).view(ctx.h[0]) if want_h else None, gS.to(ctx.s[1]).view(ctx.s[0]) if want_s else None, None, None, None)


def purified_density_matrix(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, n_occ, orthogonalizer: Optional[Orthogonalizer] = None,
                            max_iter: int = 100, return_solution: bool = False):
    """The closed-shell density matrix of every molecule WITHOUT a solve -> ``D`` float64 [P] on the device (``return_solution=True``:
    ``(D, BatchedPurification)``), differentiable with respect to ``H_packed`` and ``S_packed``: the ``D`` of ``density_matrix`` to rounding, from symmetric
    float64 matrix products alone (module text, "Without a solve").

    Arguments as for ``density_matrix``.  ``orthogonalizer``: what ``BatchedPurification.orthogonalize(S_packed)`` returned for this batch (it must be the
    one of ``S_packed``: the gradient of ``S_packed`` is evaluated through it); None: one is made here, one latency-bound launch.  Prediction and target of a
    step share ``S`` and so the orthogonalizer.  ``S_packed = None``: the standard problem, no orthogonalizer.  ``max_iter``: the iteration cap (11..49
    iterations were needed at gaps of 1e-3..0.3 of a 20-unit spectrum).  The backward runs the recursion of the module text along the logged branches; the
    upstream gradient need not be symmetric; nothing is launched without one, the ``S`` half is skipped when ``S`` is None or requires no gradient, and the
    gradients are cast to the inputs' dtypes in the symmetric-matrix convention of ``orbital_energies``.  **Needs an open gap**: a molecule whose
    purification does not converge in ``max_iter`` iterations (status 4) or whose overlap is not positive definite (status 1) yields NaN in its own blocks
    only; ``BatchedPurification.check()`` reports both.  No energies other than HOMO and LUMO (``purified_frontier(..., solution=solution)``) and no smearing.
    ``populations(D, plan, S, H, orbitals=solution)`` works on the result."""
    _require_gpu(H_packed)
    if S_packed is not None:
        _require_gpu(S_packed)
    elif orthogonalizer is not None:
        raise ValueError("purified_density_matrix: an orthogonalizer without S_packed")
    pur = BatchedPurification(plan_or_orb_ptr, H_packed.device)
    if S_packed is not None and orthogonalizer is None:
        orthogonalizer = pur.orthogonalize(S_packed)
    D = _PurifiedDensity.apply(pur, H_packed, S_packed, n_occ, orthogonalizer, max_iter)
    return (D, pur) if return_solution else D


class QHNetPurifiedDensityLightning(QHNetDensityLightning):
    """``QHNetDensityLightning`` without a solve: ``"density_matrix"`` and ``"mulliken_charges"`` come from ``purified_density_matrix`` of the packed prediction
    and a detached ``BatchedPurification`` of the packed target, both through ONE orthogonalizer of ``batch.overlap`` per step.  Purification has no orbital
    energies other than HOMO and LUMO (``QHNetPurifiedFrontierLightning``): an active ``"orbital_energies"`` key raises ``ValueError`` (use the parent).  ``max_iter`` (attribute; class default 100) caps the iterations.
    Prefer it where the gaps are safely open; a molecule without a gap gets NaN, which the parent's solver does not need.  With both coefficients at 0 (or
    without the keys) nothing is purified and the step is ``QHNetLightning``'s."""

    max_iter = 100

    def _evaluate(self, batch):
        if not self._packed():
            raise ValueError("QHNetPurifiedDensityLightning needs packed losses (HamiltonianLoss, DensityMatrixLoss, MullikenChargeLoss)")
        active = self._active()
        if "orbital_energies" in active:
            raise ValueError("QHNetPurifiedDensityLightning: purification has no orbital energies; use QHNetDensityLightning for an \"orbital_energies\" term")
        preds, targets, loss_args = QHNetLightning._evaluate(self, batch)
        if not active:
            return preds, targets, loss_args
        charges = [getattr(self.hparams.losses[k], "charge", 0) for k in active]
        if any(not np.array_equal(np.asarray(c), np.asarray(charges[0])) for c in charges[1:]):
            raise ValueError("the orbital losses count the occupied orbitals with different charges")
        plan, asm = self.net.last_plan, self.net._asm
        overlap = getattr(batch, "overlap", None)
        S = None if overlap is None else asm.pack_targets(plan, overlap)
        op = _orb_ptr_of(plan)
        n_occ = occupied_counts(batch.z, batch.ptr, charges[0], op)
        Hp, Ht = preds["hamiltonian"], targets["hamiltonian"]
        pur_t = BatchedPurification(op, Hp.device)
        orth = None if S is None else pur_t.orthogonalize(S)
        D_t = pur_t.purify(Ht, n_occ, self.max_iter, orth).density()
        D, pur_p = purified_density_matrix(Hp, S, op, n_occ, orth, self.max_iter, return_solution=True)
        for k in active:
            if k == "density_matrix":
                preds[k], targets[k], preds[k + "_args"] = D, D_t, (op,)
            else:
                preds[k] = mulliken_charges(batch.z, populations(D, plan, S, None, pur_p)[0])
                targets[k] = mulliken_charges(batch.z, pur_t.populations(D_t, plan, S)[0])
                preds[k + "_args"] = (batch.ptr,)
        return preds, targets, loss_args



class _PurifiedFrontier(torch.autograd.Function):
    """Forward: ``BatchedPurification.purify`` (unless the solution came purified) and ``frontier``.  Backward: one ``nq_orb_front_gram`` launch; nothing is
    launched without an upstream gradient, and the ``S`` half is skipped when ``S`` asks for nothing."""

    @staticmethod
    def forward(ctx, pur, H, S, n_occ, orth, max_iter, k_max, tol, fresh):
        if fresh:
            pur.purify(H, n_occ, max_iter, orth)
        levels = pur.frontier(k_max, tol)
        ctx.set_materialize_grads(False)
        ctx.pur, ctx.levels = pur, levels
        ctx.h = (H.shape, H.dtype)
        ctx.s = None if S is None else (S.shape, S.dtype)
        pur.levels = levels
        return levels.homo.clone(), levels.lumo.clone()

    @staticmethod
    def backward(ctx, g_homo, g_lumo):
        none = (None,) * 9
        want_h = ctx.needs_input_grad[1]
        want_s = ctx.s is not None and ctx.needs_input_grad[2]
        if (g_homo is None and g_lumo is None) or not (want_h or want_s):
            return none
        g = [None if t is None else t.to(torch.float64).reshape(-1).contiguous() for t in (g_homo, g_lumo)]
        gH, gS = ctx.pur.frontier_gradients(ctx.levels, g[0], g[1], want_s)
        return (None, gH.to(ctx.h[1]).view(ctx.h[0]) if want_h else None, gS.to(ctx.s[1]).view(ctx.s[0]) if want_s else None) + none[3:]


def purified_frontier(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, n_occ, orthogonalizer: Optional[Orthogonalizer] = None,
                      max_iter: int = 100, k_max: int = 256, tol: float = 2.0 ** -44, solution: Optional[BatchedPurification] = None,
                      return_solution: bool = False):
    """HOMO and LUMO of every molecule WITHOUT a solve -> ``(homo, lumo)`` float64 [B] on the device (``return_solution=True``: ``(homo, lumo,
    BatchedPurification)``; its ``levels`` attribute holds the ``FrontierLevels``), differentiable with respect to ``H_packed`` and ``S_packed``: SP2
    purification, then a projected Lanczos recurrence on ``X``, ``Ht`` and the bounds (``BatchedPurification.frontier``).

    Arguments as for ``purified_density_matrix``; ``k_max`` caps the Lanczos steps per side (26..190 were needed at 130..539 orbitals), ``tol`` is the
    residual bound in units of the Gershgorin width (the gradients are accurate to ``tol / sep``, ``sep`` the distance to the neighbouring level).
    ``solution``: the ``BatchedPurification`` that ``purified_density_matrix(..., return_solution=True)`` already ran on the SAME ``H_packed`` (and ``S_packed``)
    -- the prediction is then purified once per step; ``orthogonalizer`` and ``max_iter`` are its own.  The gradients need no eigenvector response:
    ``d eps / dH = c c^T``, ``d eps / dS = -eps c c^T`` (the convention of ``orbital_energies``), cast to the inputs' dtypes; nothing is launched without an
    upstream gradient and the ``S`` half is skipped when ``S`` is None or requires no gradient.  A level that does not exist (the LUMO where ``n_occ = m``, the
    HOMO where ``n_occ = 0``) is NaN and takes no gradient; a side that does not converge in ``k_max`` steps is NaN and gives NaN gradient blocks for its
    molecule only (``solution.frontier_check(solution.levels)`` reports it).  Needs an open gap, like the purification it follows."""
    _require_gpu(H_packed)
    if S_packed is not None:
        _require_gpu(S_packed)
    elif orthogonalizer is not None:
        raise ValueError("purified_frontier: an orthogonalizer without S_packed")
    fresh = solution is None
    if fresh:
        pur = BatchedPurification(plan_or_orb_ptr, H_packed.device)
        if S_packed is not None and orthogonalizer is None:
            orthogonalizer = pur.orthogonalize(S_packed)
    else:
        pur = solution
        pur._purified()
        if not np.array_equal(pur.orb_ptr, _orb_ptr_of(plan_or_orb_ptr)):
            raise ValueError("purified_frontier: the solution belongs to another batch")
        if (pur._orth is None) != (S_packed is None):
            raise ValueError("purified_frontier: the solution was purified with an overlap and S_packed is None, or the reverse")
    homo, lumo = _PurifiedFrontier.apply(pur, H_packed, S_packed, n_occ, orthogonalizer, max_iter, k_max, tol, fresh)
    return (homo, lumo, pur) if return_solution else (homo, lumo)


class FrontierLoss(nn.Module):
    """``kind`` "mae" | "mse" of the frontier levels, ``which`` = "gap" (LUMO - HOMO) | "homo" | "lumo" | "both": the mean over the existing selected levels of each
    molecule, then the mean over the molecules (a molecule where none of them exists -- the LUMO or the gap where every orbital is occupied -- adds 0).
    ``("mae", "both")`` equals ``OrbitalEnergyLoss("mae", "frontier")`` on the same levels.  Prediction and target: float64 [2, B], row 0 HOMO, row 1 LUMO (what
    ``torch.stack(purified_frontier(...))`` gives; NaN where a level does not exist).  ``charge`` is what the task counts the occupied orbitals with."""

    packed = True

    def __init__(self, kind: str = "mae", which: str = "gap", charge=0):
        super().__init__()
        if kind not in ("mae", "mse"):
            raise ValueError(f"kind must be 'mae' or 'mse', not {kind!r}")
        if which not in ("gap", "homo", "lumo", "both"):
            raise ValueError(f"which must be 'gap', 'homo', 'lumo' or 'both', not {which!r}")
        self.kind, self.which, self.charge = kind, which, charge

    def occupied(self, z, ptr, orb_ptr=None) -> torch.Tensor:
        return occupied_counts(z, ptr, self.charge, orb_ptr)

    def forward(self, pred: torch.Tensor, target: torch.Tensor, n_occ, orb_ptr) -> torch.Tensor:
        _require_gpu(pred)
        op = _orb_ptr_of(orb_ptr)
        no = check_occupied(n_occ, op)
        m = np.diff(op)
        B = m.shape[0]
        if tuple(pred.shape) != (2, B) or tuple(target.shape) != (2, B):
            raise ValueError(f"the levels have shapes {tuple(pred.shape)} / {tuple(target.shape)}, orb_ptr counts [2, {B}]")
        has_lumo = no < m
        d = pred.to(torch.float64) - target.to(torch.float64).detach()
        if self.which == "gap":
            rows, w = (d[1] - d[0]).unsqueeze(0), has_lumo[None, :] / B
        elif self.which == "homo":
            rows, w = d[0:1], np.full((1, B), 1.0 / B)
        elif self.which == "lumo":
            rows, w = d[1:2], has_lumo[None, :] / B
        else:
            rows, w = d, np.stack([np.ones(B), has_lumo.astype(np.float64)]) / (1.0 + has_lumo) / B
        weight = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(pred.device)
        rows = torch.where(weight > 0, rows, torch.zeros_like(rows))          # a level that does not exist is NaN: it neither counts nor takes a gradient
        return torch.sum(weight * (rows.abs() if self.kind == "mae" else rows * rows))


class QHNetPurifiedFrontierLightning(QHNetPurifiedDensityLightning):
    """``QHNetPurifiedDensityLightning`` with a term on HOMO, LUMO or the gap, still without a solve: ``losses`` / ``loss_coefs`` take ``"frontier"`` (a
    ``FrontierLoss``).  The prediction goes through ``purified_frontier``, which shares the purification of an active ``"density_matrix"`` /
    ``"mulliken_charges"`` term (one ``nq_orb_pur_run`` for the prediction per step); the target through a detached ``BatchedPurification(...).frontier()``;
    ONE orthogonalizer of ``batch.overlap`` per step serves all of it.  ``k_max`` / ``tol`` (attributes; class defaults 256 and 2^-44) are the Lanczos limits.
    With the ``"frontier"`` coefficient at 0 (or without the key) the step is the parent's, and the parent's refusal of ``"orbital_energies"`` stays."""

    KEYS = QHNetPurifiedDensityLightning.KEYS + ("frontier",)
    k_max = 256
    tol = 2.0 ** -44

    def _evaluate(self, batch):
        active = self._active()
        if "frontier" not in active:
            return super()._evaluate(batch)
        if not self._packed():
            raise ValueError("QHNetPurifiedFrontierLightning needs packed losses (HamiltonianLoss, FrontierLoss, DensityMatrixLoss, MullikenChargeLoss)")
        if "orbital_energies" in active:
            raise ValueError("QHNetPurifiedFrontierLightning: purification has no orbital energies other than HOMO and LUMO; use QHNetDensityLightning for an "
                             "\"orbital_energies\" term")
        preds, targets, loss_args = QHNetLightning._evaluate(self, batch)
        charges = [getattr(self.hparams.losses[k], "charge", 0) for k in active]
        if any(not np.array_equal(np.asarray(c), np.asarray(charges[0])) for c in charges[1:]):
            raise ValueError("the orbital losses count the occupied orbitals with different charges")
        plan, asm = self.net.last_plan, self.net._asm
        overlap = getattr(batch, "overlap", None)
        S = None if overlap is None else asm.pack_targets(plan, overlap)
        op = _orb_ptr_of(plan)
        n_occ = occupied_counts(batch.z, batch.ptr, charges[0], op)
        Hp, Ht = preds["hamiltonian"], targets["hamiltonian"]
        pur_t = BatchedPurification(op, Hp.device)
        orth = None if S is None else pur_t.orthogonalize(S)
        pur_t.purify(Ht, n_occ, self.max_iter, orth)
        lv_t = pur_t.frontier(self.k_max, self.tol)
        need_density = any(k != "frontier" for k in active)
        pur_p = None
        if need_density:
            D_t = pur_t.density()
            D, pur_p = purified_density_matrix(Hp, S, op, n_occ, orth, self.max_iter, return_solution=True)
        homo, lumo = purified_frontier(Hp, S, op, n_occ, orth, self.max_iter, self.k_max, self.tol, solution=pur_p)
        for k in active:
            if k == "frontier":
                preds[k], targets[k], preds[k + "_args"] = torch.stack((homo, lumo)), torch.stack((lv_t.homo, lv_t.lumo)), (n_occ, op)
            elif k == "density_matrix":
                preds[k], targets[k], preds[k + "_args"] = D, D_t, (op,)
            else:
                preds[k] = mulliken_charges(batch.z, populations(D, plan, S, None, pur_p)[0])
                targets[k] = mulliken_charges(batch.z, pur_t.populations(D_t, plan, S)[0])
                preds[k + "_args"] = (batch.ptr,)
        return preds, targets, loss_args


class _PurifiedOccupied(torch.autograd.Function):
    """Forward: ``BatchedPurification.purify`` (unless the solution came purified) and ``occupied``.  Backward: ONE ``nq_orb_wgram`` launch on the occupied state
    with ``w = g`` and ``w = -eps g`` over ``k < n_occ``; nothing is launched without an upstream gradient, and the ``S`` half is skipped when ``S`` asks for
    nothing."""

    @staticmethod
    def forward(ctx, pur, H, S, n_occ, orth, max_iter, fresh):
        if fresh:
            pur.purify(H, n_occ, max_iter, orth)
        occ = pur.occupied()
        ctx.set_materialize_grads(False)
        ctx.occ = occ
        ctx.h = (H.shape, H.dtype)
        ctx.s = None if S is None else (S.shape, S.dtype)
        pur.occupied_orbitals = occ
        return occ.energies.clone()

    @staticmethod
    def backward(ctx, g):
        none = (None,) * 7
        want_h = ctx.needs_input_grad[1]
        want_s = ctx.s is not None and ctx.needs_input_grad[2]
        if g is None or not (want_h or want_s):
            return none
        occ = ctx.occ
        g = g.to(torch.float64).reshape(-1).contiguous()
        if want_s:
            gH, gS = occ.weighted_gram(g, -(occ.energies * g))
            gS = gS.to(ctx.s[1]).view(ctx.s[0])
        else:
            gH, gS = occ.weighted_gram(g), None
        return (None, gH.to(ctx.h[1]).view(ctx.h[0]) if want_h else None, gS) + none[3:]


def purified_occupied_energies(H_packed: torch.Tensor, S_packed: Optional[torch.Tensor], plan_or_orb_ptr, n_occ, orthogonalizer: Optional[Orthogonalizer] = None,
                               max_iter: int = 100, solution: Optional[BatchedPurification] = None, return_solution: bool = False):
    """ALL occupied orbital energies of every molecule WITHOUT a full solve -> ``eps`` float64 [M] on the device, ascending in the slots ``k < n_occ`` of each
    molecule and NaN in the others (``return_solution=True``: ``(eps, BatchedPurification)``; its ``occupied_orbitals`` attribute holds the
    ``OccupiedOrbitals``), differentiable with respect to ``H_packed`` and ``S_packed``: SP2 purification, a pivoted Cholesky factor of the projector and the
    ``n_occ x n_occ`` Rayleigh-Ritz problem (``BatchedPurification.occupied``).

    Arguments as for ``purified_frontier``.  ``solution``: the ``BatchedPurification`` that ``purified_density_matrix(..., return_solution=True)`` already ran on the
    SAME ``H_packed`` (and ``S_packed``) -- the prediction is then purified once per step.  The gradients need no eigenvector response: ``d eps_k / dH = c_k c_k^T``,
    ``d eps_k / dS = -eps_k c_k c_k^T`` (the convention of ``orbital_energies``), one ``nq_orb_wgram`` launch over ``k < n_occ``, cast to the inputs' dtypes;
    nothing is launched without an upstream gradient and the ``S`` half is skipped when ``S`` is None or requires no gradient.  The NaN slots take no gradient
    (mask them with ``torch.where`` before reducing, as ``OccupiedEnergyLoss`` does).  A molecule whose purification failed (status 1 / 4) or whose projector is
    not one (status 5) is NaN in all its slots and gives NaN gradient blocks for that molecule only (``solution.occupied_orbitals.check()`` reports it).  Needs
    an open gap, like the purification it follows; closed shells, occupied levels only."""
    _require_gpu(H_packed)
    if S_packed is not None:
        _require_gpu(S_packed)
    elif orthogonalizer is not None:
        raise ValueError("purified_occupied_energies: an orthogonalizer without S_packed")
    fresh = solution is None
    if fresh:
        pur = BatchedPurification(plan_or_orb_ptr, H_packed.device)
        if S_packed is not None and orthogonalizer is None:
            orthogonalizer = pur.orthogonalize(S_packed)
    else:
        pur = solution
        pur._purified()
        if not np.array_equal(pur.orb_ptr, _orb_ptr_of(plan_or_orb_ptr)):
            raise ValueError("purified_occupied_energies: the solution belongs to another batch")
        if (pur._orth is None) != (S_packed is None):
            raise ValueError("purified_occupied_energies: the solution was purified with an overlap and S_packed is None, or the reverse")
    eps = _PurifiedOccupied.apply(pur, H_packed, S_packed, n_occ, orthogonalizer, max_iter, fresh)
    return (eps, pur) if return_solution else eps


class OccupiedEnergyLoss(nn.Module):
    """``kind`` "mae" | "mse" of the occupied orbital energies: the mean over the ``n_occ`` occupied levels of each molecule, then the mean over the molecules --
    ``OrbitalEnergyLoss(kind, "occupied")`` for energies whose virtual slots are NaN (what ``purified_occupied_energies`` / ``OccupiedOrbitals.energies`` give): the
    slots ``k >= n_occ`` are masked with ``torch.where``, so they neither count nor take a gradient.  ``("mae")`` is the ``eps_mae_occ`` of ``OrbitalErrors`` /
    ``PurifiedOrbitalErrors``.  ``charge`` is what the task counts the occupied orbitals with."""

    packed = True

    def __init__(self, kind: str = "mae", charge=0):
        super().__init__()
        if kind not in ("mae", "mse"):
            raise ValueError(f"kind must be 'mae' or 'mse', not {kind!r}")
        self.kind, self.charge = kind, charge

    def occupied(self, z, ptr, orb_ptr=None) -> torch.Tensor:
        return occupied_counts(z, ptr, self.charge, orb_ptr)

    def forward(self, eps_pred: torch.Tensor, eps_target: torch.Tensor, n_occ, orb_ptr) -> torch.Tensor:
        op = _orb_ptr_of(orb_ptr)
        no = check_occupied(n_occ, op)
        m = np.diff(op)
        B, M = m.shape[0], int(op[-1])
        if eps_pred.numel() != M or eps_target.numel() != M:
            raise ValueError(f"the energies have {eps_pred.numel()} / {eps_target.numel()} entries, orb_ptr counts {M}")
        k = np.arange(M) - np.repeat(op[:-1], m)
        sel = k < np.repeat(no.astype(np.int64), m)
        weight = torch.from_numpy(sel / np.repeat(no.astype(np.float64), m) / B).to(eps_pred.device)        # float64 [M]: mean over the occupied, then the molecules
        d = eps_pred.reshape(-1).to(torch.float64) - eps_target.reshape(-1).to(torch.float64).detach()
        d = torch.where(weight > 0, d, torch.zeros_like(d))          # a virtual slot is NaN: it neither counts nor takes a gradient
        return torch.sum(weight * (d.abs() if self.kind == "mae" else d * d))


class QHNetPurifiedOrbitalLightning(QHNetPurifiedFrontierLightning):
    """``QHNetPurifiedFrontierLightning`` with a term on ALL occupied orbital energies, still without a full solve: ``losses`` / ``loss_coefs`` take
    ``"occupied_energies"`` (an ``OccupiedEnergyLoss``).  Per step ONE orthogonalizer of ``batch.overlap`` and ONE purification of the prediction
    (``nq_orb_pur_run``), shared with any active ``"density_matrix"`` / ``"mulliken_charges"`` / ``"frontier"`` term; the prediction's levels come from
    ``purified_occupied_energies``, the target's from a detached ``purify().occupied()``; the only ``nq_orb_solve`` launches are those of the ``n_occ x n_occ``
    blocks.  The parent's refusal of ``"orbital_energies"`` stays (no virtual levels).  With the ``"occupied_energies"`` coefficient at 0 (or without the key) the
    step is the parent's."""

    KEYS = QHNetPurifiedFrontierLightning.KEYS + ("occupied_energies",)

    def _evaluate(self, batch):
        active = self._active()
        if "occupied_energies" not in active:
            return super()._evaluate(batch)
        if not self._packed():
            raise ValueError("QHNetPurifiedOrbitalLightning needs packed losses (HamiltonianLoss, OccupiedEnergyLoss, FrontierLoss, DensityMatrixLoss, MullikenChargeLoss)")
        if "orbital_energies" in active:
            raise ValueError("QHNetPurifiedOrbitalLightning: purification has the occupied orbital energies only (\"occupied_energies\"); use QHNetDensityLightning "
                             "for an \"orbital_energies\" term")
        preds, targets, loss_args = QHNetLightning._evaluate(self, batch)
        charges = [getattr(self.hparams.losses[k], "charge", 0) for k in active]
        if any(not np.array_equal(np.asarray(c), np.asarray(charges[0])) for c in charges[1:]):
            raise ValueError("the orbital losses count the occupied orbitals with different charges")
        plan, asm = self.net.last_plan, self.net._asm
        overlap = getattr(batch, "overlap", None)
        S = None if overlap is None else asm.pack_targets(plan, overlap)
        op = _orb_ptr_of(plan)
        n_occ = occupied_counts(batch.z, batch.ptr, charges[0], op)
        Hp, Ht = preds["hamiltonian"], targets["hamiltonian"]
        pur_t = BatchedPurification(op, Hp.device)
        orth = None if S is None else pur_t.orthogonalize(S)
        pur_t.purify(Ht, n_occ, self.max_iter, orth)
        eps_t = pur_t.occupied().energies
        pur_p = None
        if any(k in ("density_matrix", "mulliken_charges") for k in active):
            D_t = pur_t.density()
            D, pur_p = purified_density_matrix(Hp, S, op, n_occ, orth, self.max_iter, return_solution=True)
        eps, pur_p = purified_occupied_energies(Hp, S, op, n_occ, orth, self.max_iter, solution=pur_p, return_solution=True)
        for k in active:
            if k == "occupied_energies":
                preds[k], targets[k], preds[k + "_args"] = eps, eps_t, (n_occ, op)
            elif k == "frontier":
                lv_t = pur_t.frontier(self.k_max, self.tol)
                homo, lumo = purified_frontier(Hp, S, op, n_occ, orth, self.max_iter, self.k_max, self.tol, solution=pur_p)
                preds[k], targets[k], preds[k + "_args"] = torch.stack((homo, lumo)), torch.stack((lv_t.homo, lv_t.lumo)), (n_occ, op)
            elif k == "density_matrix":
                preds[k], targets[k], preds[k + "_args"] = D, D_t, (op,)
            else:
                preds[k] = mulliken_charges(batch.z, populations(D, plan, S, None, pur_p)[0])
                targets[k] = mulliken_charges(batch.z, pur_t.populations(D_t, plan, S)[0])
                preds[k + "_args"] = (batch.ptr,)
        return preds, targets, loss_args


__all__ = ["orbital_energies", "OrbitalEnergyLoss", "QHNetOrbitalLightning", "mulliken_charges", "orbital_solution", "density_matrix", "populations",
           "DensityMatrixLoss", "MullikenChargeLoss", "QHNetDensityLightning", "electron_counts", "SmearedSolution", "smeared_solution", "smeared_density_matrix",
           "QHNetSmearedDensityLightning", "purified_density_matrix", "QHNetPurifiedDensityLightning", "bond_orders", "BondOrderLoss", "QHNetBondOrderLightning",
           "bond_layout", "dense_bond_orders", "LowdinBasis", "lowdin_basis", "lowdin_density", "lowdin_hamiltonian", "lowdin_populations", "lowdin_charges",
           "lowdin_bond_orders", "LowdinChargeLoss", "QHNetLowdinLightning", "commutator", "scf_residual", "scf_residual_to_target", "ScfResidualLoss", "ScfTarget",
           "scf_target", "scf_target_iterative", "scf_target_blocks", "BatchedMatrixRoot", "QHNetCommutatorLightning", "ScfResidualErrors", "purified_frontier", "FrontierLoss",
           "QHNetPurifiedFrontierLightning", "FrontierLevels", "purified_occupied_energies", "OccupiedEnergyLoss", "QHNetPurifiedOrbitalLightning",
           "OccupiedOrbitals", "PurifiedOrbitalErrors"]
