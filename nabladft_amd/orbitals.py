"""Batched orbital energies on the GPU: the generalized symmetric eigenproblem ``H C = S C diag(eps)`` of every molecule of a batch in one launch
(csrc/orbitals.hip, csrc/orbdens.hip, ``nq_orb_*`` of include/nablaq.h).

Fills what the reference leaves empty: ``phisnet/nn/neural_network.py:969-993`` returns ``orbital_energies`` and ``orbital_coefficients`` as zeros.  Parity
status: **no reference code to pin against** -- the kernels are tested against a float64 numpy restatement of the textbook route (tests/orbitals_ref.py:
``np.linalg.cholesky``, two triangular solves, ``np.linalg.eigh``, back substitution).

Algorithm (float64 throughout, one 512-thread workgroup per molecule, no atomics, no host round trip): Cholesky ``S = L L^T``; ``A = L^-1 H L^-T``
symmetrised; Householder tridiagonalisation; implicit-shift QL with the vectors accumulated row-wise; ``C = L^-T Y``.  Only the lower triangles of ``H`` and
``S`` are read.  ``S = None`` is the standard problem.  Results: ``eps`` ascending inside each molecule; ``coeff`` packed like the input, ROW k of a
molecule's block = orbital k (``C^T S C = I``; the largest-magnitude component of every orbital, the first on ties, is positive).  ``per_molecule()`` hands
the user orbitals as COLUMNS, the convention of ``scipy.linalg.eigh``.

No gradient flows through the solver: the inputs of ``BatchedOrbitals`` are detached.  A loss on orbital energies needs the gradient of the eigenvalues, a loss
on densities or populations the response of the occupied subspace: both are ``nabladft_amd.orbital_loss`` (``orbital_energies``, ``orbital_solution``,
``density_matrix``, ``populations``, the losses and the QHNet tasks), built on this class and on the launches ``resp_*`` / ``syr2k`` / ``density_response`` /
``populations_backward`` below (csrc/orbresp.hip).

After a solve, ``density(n_occ)`` gives the closed-shell density matrix ``D = 2 sum_occ c_k c_k^T`` (and the energy-weighted one) and ``populations(D, plan, S)``
the Mulliken populations per atom, the electron count ``Tr(D S)`` and the band energy ``Tr(D H)`` (csrc/orbdens.hip), all on the device.

**Bond orders.**  ``bond_orders(D, plan, S)`` gives the Mayer bond-order table ``B_AB = sum_{mu in A, nu in B} (DS)_mu,nu (DS)_nu,mu`` of every molecule (the Wiberg
index without ``S``) and the atomic valences ``V_A = sum_{B != A} B_AB``, ``bond_orders_backward`` their reverse (csrc/orbbond.hip;
``nabladft_amd.orbital_loss.bond_orders`` is the differentiable call).  Closed shells only, at most ``MAX_ATOM_ORBITALS`` = 32 orbitals per atom; the Löwdin counterpart is below.

**Löwdin analysis.**  After a standard solve of ``S`` itself, ``overlap_functions()`` gives ``S^(1/2)`` and ``S^(-1/2)`` (``LowdinBasis`` holds them and the
decomposition; one per batch serves prediction and target, and since ``S`` belongs to the conformer it can be cached across epochs), ``sym_congruence(X, M)``
the Löwdin density ``S^(1/2) D S^(1/2)`` or the orthogonalised Hamiltonian ``S^(-1/2) H S^(-1/2)``, ``sym_congruence_backward`` / ``matfun_response`` their
reverse down to ``S``, evaluated without dividing by a difference of levels of ``S`` (csrc/orblowdin.hip; ``nabladft_amd.orbital_loss.lowdin_basis`` /
``lowdin_density`` / ``lowdin_populations`` / ``lowdin_bond_orders`` / ``lowdin_hamiltonian`` are the differentiable calls).  ``S`` must be positive definite
(``info = 1`` and NaN otherwise).  ``BatchedMatrixRoot`` / ``LowdinBasis.of(..., method="newton_schulz")`` give the two functions WITHOUT a decomposition, by the coupled
Newton-Schulz iteration on the matrix cores (csrc/orbsqrt.hip): no levels, no ``cond``, no gradient of ``S``; meant for ``kappa_2(S) <= 1e8``.

**SCF residual.**  ``commutator(X, Y, x_anti, alpha)`` gives ``alpha (X Y - Y X)`` of packed symmetric matrices (``x_anti``: an antisymmetric ``X``, the form of
its own reverse), ``antisymmetrize(G)`` the antisymmetric part of an upstream gradient, ``commutator_norms(R)`` the sum of squares and the largest magnitude (the
DIIS error) per molecule (csrc/orbcomm.hip); they read the layout of the state alone, nothing has to be solved.  ``nabladft_amd.orbital_loss.commutator`` /
``scf_residual`` are the differentiable calls, ``ScfResidualErrors`` accumulates the figures of a test loop.

**Smearing.**  ``fermi(n_elec, kT)`` gives Fermi-Dirac occupations ``F_k = 2 / (1 + exp((eps_k - mu) / kT))`` with the chemical potential fixed by the electron
count (``electron_counts``: odd counts and fractions are fine), ``smeared_density(occ)`` the density ``sum_k F_k c_k c_k^T`` and ``smeared_response`` its
gradient chain over all orbital pairs, evaluated without dividing by a difference of orbital energies (csrc/orbsmear.hip;
``nabladft_amd.orbital_loss.smeared_solution`` is the differentiable call).

**Without a solve.**  ``BatchedPurification`` gives the closed-shell density ``D = 2 Z^T X Z`` and its gradients from symmetric matrix products alone
(csrc/orbpurify.hip): ``Z = L^-1`` of ``S = L L^T`` (``orthogonalize``; one serves prediction and target), ``X`` the projector on the ``n_occ`` lowest levels of
``Z H Z^T`` by second-order spectral-projection purification, the gradient by the density-matrix-perturbation recursion along the same iterates
(``nabladft_amd.orbital_loss.purified_density_matrix`` is the differentiable call).  Closed shells only, needs an open gap, no smearing, no orbital energies
other than HOMO and LUMO: ``frontier()`` gives those two from ``X``, ``Ht`` and the bounds by a projected Lanczos recurrence (csrc/orbfrontier.hip; one
workgroup per molecule and side, no ``m^3`` work), ``frontier_gradients`` their gradients ``c c^T`` and ``-eps c c^T``
(``nabladft_amd.orbital_loss.purified_frontier`` is the differentiable call).  ``occupied()`` gives ALL occupied levels and coefficients, still without a
full solve (csrc/orbocc.hip): an exact projector of rank ``n_occ`` has a pivoted Cholesky factor ``X = Q^T Q`` with orthonormal rows, so Rayleigh-Ritz on the
``n_occ x n_occ`` matrix ``Q Ht Q^T`` gives them (``OccupiedOrbitals``; ``nabladft_amd.orbital_loss.purified_occupied_energies`` is the differentiable call,
``PurifiedOrbitalErrors`` accumulates the figures of a test loop).  Closed shells, an open gap, occupied levels only, 1..1024 orbitals; no virtual level
other than the LUMO of ``frontier()``.

Limits (each raises, nothing degrades silently): 1..``MAX_ORBITALS`` = 1024 orbitals per molecule; closed shells only in ``occupied_counts`` / ``density``
(``occupied_counts`` refuses an odd electron count; the smeared calls take any count in (0, 2m)); MI355X only, no CPU path.
"""
import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._devstate import DeviceState

MAX_ORBITALS = 1024
MAX_ATOM_ORBITALS = 32        # per atom in the bond-order kernels (NQ_BD_MAX_ATOM_ORB of csrc/orbbond.hip)
MAX_QL_SWEEPS = 60            # per eigenvalue (NQ_ORB_MAX_ITER of csrc/orbitals.hip)
FIGURES = ("eps_mae_occ", "eps_mae_all", "psi_sim_occ", "homo_abs_err", "lumo_abs_err", "gap_abs_err", "psi_sim_min_occ")


def _host_ptr(p) -> np.ndarray:
    if isinstance(p, torch.Tensor):
        p = p.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(p, dtype=np.int64).reshape(-1))


def _orb_ptr_of(plan_or_orb_ptr) -> np.ndarray:
    """``orb_ptr`` [B+1] on the host from a ``BlockAssembler`` / ``IrrepsAssembler`` plan (its ``mol_orb_ptr``; one small device->host copy) or from the array."""
    src = getattr(plan_or_orb_ptr, "mol_orb_ptr", plan_or_orb_ptr)
    return _host_ptr(src)


def occupied_counts(z, ptr, charge=0, orb_ptr=None) -> torch.Tensor:
    """Doubly occupied orbitals per molecule, int32 [B] on the host: ``(sum Z - charge) / 2``.  ``charge``: one number or one per molecule.  Raises
    ``ValueError`` (on the host, before any device work) for an odd electron count or a count below 1, and, given the batch's ``orb_ptr`` (or a plan), for
    ``n_occ > m``; ``BatchedOrbitals.frontier`` and ``OrbitalErrors.update`` check that upper end again against the orbitals they solved."""
    zz, pp = _host_ptr(z), _host_ptr(ptr)
    B = pp.shape[0] - 1
    ch = np.broadcast_to(np.asarray(charge, dtype=np.int64), (B,))
    ne = np.add.reduceat(zz, pp[:-1])[:B] - ch if B > 0 else np.zeros(0, dtype=np.int64)
    if np.any(np.diff(pp) < 1):
        raise ValueError("occupied_counts: a molecule without atoms")
    if np.any(ne % 2 != 0):
        b = int(np.nonzero(ne % 2)[0][0])
        raise ValueError(f"occupied_counts: molecule {b} has {int(ne[b])} electrons: open shells are not built")
    if np.any(ne < 2):
        b = int(np.nonzero(ne < 2)[0][0])
        raise ValueError(f"occupied_counts: molecule {b} has {int(ne[b])} electrons: n_occ must be in 1..m")
    no = (ne // 2).astype(np.int32)
    if orb_ptr is not None:
        check_occupied(no, _orb_ptr_of(orb_ptr))
    return torch.from_numpy(no)


def electron_counts(z, ptr, charge=0, orb_ptr=None) -> torch.Tensor:
    """Electrons per molecule, float64 [B] on the host: ``sum Z - charge`` (``charge``: one number or one per molecule; fractions allowed).  Odd counts are
    fine: this is what ``BatchedOrbitals.fermi`` / ``smeared_solution`` count with.  Raises ``ValueError`` (on the host, before any device work) for a count
    <= 0 and, given the batch's ``orb_ptr`` (or a plan), for a count >= 2 m: Fermi occupations need ``0 < n_elec < 2 m``."""
    zz, pp = _host_ptr(z), _host_ptr(ptr)
    B = pp.shape[0] - 1
    if B < 1 or np.any(np.diff(pp) < 1):
        raise ValueError("electron_counts: a molecule without atoms")
    ne = np.add.reduceat(zz, pp[:-1])[:B].astype(np.float64) - np.broadcast_to(np.asarray(charge, dtype=np.float64), (B,))
    if np.any(~(ne > 0)):
        b = int(np.nonzero(~(ne > 0))[0][0])
        raise ValueError(f"electron_counts: molecule {b} has {ne[b]:g} electrons: n_elec must be in (0, 2m)")
    if orb_ptr is not None:
        m = np.diff(_orb_ptr_of(orb_ptr))
        if m.shape != ne.shape:
            raise ValueError(f"orb_ptr counts {m.shape[0]} molecules, ptr {B}")
        bad = np.nonzero(ne >= 2.0 * m)[0]
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"electron_counts: molecule {b} has {ne[b]:g} electrons for m={int(m[b])} orbitals: n_elec must be in (0, 2m)")
    return torch.from_numpy(np.ascontiguousarray(ne))


FermiResult = namedtuple("FermiResult", "mu occ docc entropy info n_elec kT")
FermiResult.__doc__ = """What ``BatchedOrbitals.fermi`` returns, all on the device: ``mu`` [B], ``occ`` = F [M], ``docc`` = dF/d eps at fixed mu [M] (<= 0), ``entropy`` [B]
(units of k_B), ``info`` int32 [B] (0 ok, 1: NaN outputs), and the ``n_elec`` / ``kT`` float64 [B] the call was made with."""


def check_occupied(n_occ, orb_ptr) -> np.ndarray:
    """``n_occ`` [B] against the orbital counts of ``orb_ptr``: ``ValueError`` on the host unless ``1 <= n_occ <= m`` for every molecule.  -> int32 array."""
    no = _host_ptr(n_occ).astype(np.int32)
    m = np.diff(_host_ptr(orb_ptr))
    if no.shape != m.shape:
        raise ValueError(f"n_occ has {no.shape[0]} entries for {m.shape[0]} molecules")
    bad = np.nonzero((no < 1) | (no > m))[0]
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"molecule {b}: n_occ={int(no[b])} outside 1..m={int(m[b])}")
    return no


def bond_layout(mol_ptr) -> np.ndarray:
    """``bond_ptr`` int64 [B+1] on the host from the atoms' ``mol_ptr`` [B+1]: molecule b owns the ``n_b^2`` ordered atom pairs ``(A, B)``, ``A = B`` included,
    row-major at ``bond_ptr[b]``; ``Q = bond_ptr[B]`` (the ragged layout of the Graphormer3D ``pair_ptr``)."""
    mp = _host_ptr(mol_ptr)
    if mp.shape[0] < 2 or np.any(np.diff(mp) < 1):
        raise ValueError("bond_layout: mol_ptr needs at least one molecule and one atom in each")
    n = np.diff(mp)
    return np.concatenate([[0], np.cumsum(n * n)]).astype(np.int64)


def dense_bond_orders(bond, mol_ptr, b: int):
    """Molecule ``b``'s ``[n_b, n_b]`` table as a view of the flat ``bond`` [Q] (a tensor or an array; ``mol_ptr`` [B+1]: the atoms of every molecule)."""
    mp = _host_ptr(mol_ptr)
    bp = bond_layout(mp)
    if not 0 <= b < mp.shape[0] - 1:
        raise IndexError(f"molecule {b} of {mp.shape[0] - 1}")
    if bond.shape[0] != int(bp[-1]) or len(bond.shape) != 1:
        raise ValueError(f"bond has {tuple(bond.shape)} entries, mol_ptr counts {int(bp[-1])}")
    n = int(mp[b + 1] - mp[b])
    return bond[int(bp[b]):int(bp[b + 1])].reshape(n, n)


def _failure_text(b: int, status: int, info: int, m: int) -> str:
    """What a non-zero ``status[b]`` means (include/nablaq.h)."""
    if status == 1:
        return f"molecule {b}: the overlap matrix is not positive definite (Cholesky pivot {info} of {m} is <= 0 or not finite)"
    if status == 2:
        return f"molecule {b}: the QL iteration did not converge in {MAX_QL_SWEEPS} sweeps on one eigenvalue"
    if status == 4:
        return f"molecule {b}: the purification did not converge in {info} iterations (no gap between the occupied and the virtual levels?)"
    return f"molecule {b}: the state buffer no longer holds the batch nq_orb_init prepared (status {status}): it was overwritten"


def _require_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("MI355X only: nabladft_amd.orbitals has no CPU path, move the matrices to cuda")


def _packed(t: torch.Tensor, P: int, name: str) -> torch.Tensor:
    _require_gpu(t)
    t = t.detach()
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64, not {t.dtype}")
    if t.numel() != P:
        raise ValueError(f"{name} has {t.numel()} entries, the plan packs {P}")
    return t.reshape(-1).contiguous()


def _typed(t: Optional[torch.Tensor]):
    """The argument pair of a float32-or-float64 matrix that may be absent: ``(pointer, is_float64)``."""
    return _lib.ptr(t), int(t is not None and t.dtype == torch.float64)


def _ptrs(tensors):
    return [_lib.ptr(t) for t in tensors]


class OrbitalState(DeviceState):
    """One caller-owned device buffer behind ``nq_orb_*`` plus typed views of its parts: ``eps`` f64 [M], ``coeff`` f64 [P] (row k of a block = orbital k),
    ``status`` / ``info`` / ``iters`` int32 [B] (include/nablaq.h)."""

    def __init__(self, orb_ptr, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("MI355X only: nabladft_amd.orbitals has no CPU path")
        op =_orb_ptr_of(orb_ptr)
        if op.shape[0] < 2:
            raise ValueError("orb_ptr needs at least one molecule")
        m = np.diff(op)
        if int(m.max()) > MAX_ORBITALS:
            b = int(m.argmax())
            raise _lib.NablaqError(_lib.NQ_ERR_MOL_TOO_LARGE, f"molecule {b} has {int(m[b])} orbitals, the limit is {MAX_ORBITALS}")
        if int(m.min()) < 1:
            raise ValueError(f"molecule {int(m.argmin())} has {int(m.min())} orbitals")
        self.orb_ptr_host = op
        self.pack_ptr_host = np.concatenate([[0], np.cumsum(m * m)]).astype(np.int64)
        self.m = m
        self.B, self.M, self.P = int(m.shape[0]), int(op[-1]), int(self.pack_ptr_host[-1])
        B, M, P, i32, f64 = self.B, self.M, self.P, torch.int32, torch.float64
        nbytes = self._allocate("orb", (B, M, P), (
            ("header_dev", i32, (16,)), ("orb_ptr", i32, (B + 1,)), ("pack_ptr", torch.int64, (B + 1,)), ("order", i32, (B,)), ("status", i32, (B,)),
            ("info", i32, (B,)), ("iters", i32, (B,)), ("eps", f64, (M,)), ("coeff", f64, (P,)), ("work", f64, (P,)), ("chol", f64, (P,))), device)
        op32 = np.ascontiguousarray(op.astype(np.int32))
        out = (C.c_int32 * 2)()
        with torch.cuda.device(device):
            _lib.check(_lib.load().nq_orb_init(_lib.ptr(self.buf), nbytes, op32.ctypes.data_as(C.c_void_p), *self._dims, out, _lib.stream_ptr()))
        self.max_m = int(out[0])

    def call(self, name: str, *args):
        """The one launch line of the family: ``name(buf, B, M, P, *args, stream)`` on the state's device and the current stream; raises on a refusal."""
        with torch.cuda.device(self.buf.device):
            _lib.check(getattr(_lib.load(), name)(_lib.ptr(self.buf), *self._dims, *args, _lib.stream_ptr()))

    def solve(self, H_packed: torch.Tensor, S_packed: Optional[torch.Tensor] = None):
        H = _packed(H_packed, self.P, "H_packed")
        S = None if S_packed is None else _packed(S_packed, self.P, "S_packed")
        if H.device != self.buf.device or (S is not None and S.device != self.buf.device):
            raise ValueError(f"the matrices must live on {self.buf.device}")
        self.call("nq_orb_solve", *_typed(H), *_typed(S))

    def header(self) -> dict:
        """The header words (one small device->host copy, synchronises the stream); raises if a call was refused on the device."""
        h = self._read_header()
        if h[4] == -2:
            raise RuntimeError("an nq_orb call came with other dimensions than nq_orb_init prepared the state for")
        if h[4] == -3:
            raise RuntimeError("a state that holds a purification was passed to a call that reads orbital coefficients, or the reverse")
        return dict(B=h[0], M=h[1], P=(h[2] & 0xffffffff) + (h[3] << 32), status=h[4], max_m=h[5])

    def first_failure(self):
        """What every ``check()`` starts with: the header (raises if a call was refused on the device) and the status words, one host synchronisation ->
        ``(b, status[b])`` of the first molecule with a non-zero status, or None."""
        self.header()
        status = self.status.cpu().numpy()
        bad = np.nonzero(status)[0]
        return (int(bad[0]), int(status[bad[0]])) if bad.size else None


class _LayoutLaunches:
    """The launches that read the layout of ``self.state`` alone (its ``orb_ptr`` / ``pack_ptr`` and status words), whatever its matrices hold: populations, bond
    orders, the Löwdin congruences and the commutators.  ``BatchedOrbitals`` and ``BatchedPurification`` derive from it."""

    def _f64(self, t: torch.Tensor, n: int, name: str) -> torch.Tensor:
        dev = self.state.buf.device
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.numel() != n or t.device != dev:
            raise ValueError(f"{name} must be float64 [{n}] on {dev}")
        return t.detach().reshape(-1).contiguous()

    def _scratch(self, n: int, make: bool = True):
        return torch.empty(n, dtype=torch.float64, device=self.state.buf.device) if make else None

    # ---- populations (csrc/orbdens.hip, csrc/orbresp.hip) and bond orders (csrc/orbbond.hip) ------------------------------------------------------------------
    def _bond_tables(self, plan):
        """The one validation of a plan against the batch -> ``(N, Q, mol_ptr int32, atom_orb_ptr int64, bond_ptr int64)``, the three tables on the device; one
        small device -> host copy of ``mol_ptr``, remembered per plan.  The populations use the first, third and fourth, the bond orders all five."""
        st, dev = self.state, self.state.buf.device
        cached = getattr(self, "_bond_cache", None)
        if cached is not None and cached[0] is plan:
            return cached[1]
        if int(plan.B) != st.B or int(plan.m_total) != st.M or int(plan.total) != st.P:
            raise ValueError("the plan belongs to another batch")
        N = int(plan.N)
        mp = _host_ptr(plan.mol_ptr)
        if mp.shape[0] != st.B + 1 or plan.orb_ptr.numel() != N + 1 or int(mp[0]) != 0 or int(mp[-1]) != N:
            raise ValueError("the plan belongs to another batch: its mol_ptr / orb_ptr do not have B + 1 / N + 1 entries")
        bp = bond_layout(mp)
        out = (N, int(bp[-1]), plan.mol_ptr.to(device=dev, dtype=torch.int32).contiguous(), plan.orb_ptr.to(device=dev, dtype=torch.int64).contiguous(),
               torch.from_numpy(bp).to(dev))
        self._bond_cache = (plan, out)
        return out

    def populations(self, D: torch.Tensor, plan, S_packed: Optional[torch.Tensor] = None, H_packed: Optional[torch.Tensor] = None):
        """Mulliken analysis of a packed density ``D`` -> ``(atom_pop [N], nelec [B], eband [B] or None without H_packed)``, float64 on the device:
        ``pop_mu = sum_nu D_mu,nu S_mu,nu`` summed over each atom's orbitals, ``nelec = Tr(D S)``, ``eband = Tr(D H)``.  ``plan``: the ``BlockAssembler`` /
        ``IrrepsAssembler`` plan of the batch (its ``mol_ptr`` and per-atom ``orb_ptr``).  ``S_packed = None``: the identity."""
        st, dev = self.state, self.state.buf.device
        Dp = _packed(D, st.P, "D")
        if Dp.dtype != torch.float64:
            raise TypeError("D must be float64 (what density() returns)")
        S = None if S_packed is None else _packed(S_packed, st.P, "S_packed")
        H = None if H_packed is None else _packed(H_packed, st.P, "H_packed")
        N, _, mol_ptr, atom_ptr, _ = self._bond_tables(plan)
        pop = torch.empty(N, dtype=torch.float64, device=dev)
        nelec = torch.empty(st.B, dtype=torch.float64, device=dev)
        eband = None if H is None else torch.empty(st.B, dtype=torch.float64, device=dev)
        st.call("nq_orb_population", _lib.ptr(Dp), *_typed(H), *_typed(S), N, _lib.ptr(mol_ptr), _lib.ptr(atom_ptr), _lib.ptr(pop), _lib.ptr(nelec),
                                     _lib.ptr(eband))
        return pop, nelec, eband

    def populations_backward(self, plan, g_pop, g_nelec, g_eband, D=None, S_packed=None, H_packed=None, want_s: bool = False, want_h: bool = False):
        """The reverse of ``populations`` (``nq_orb_population_backward``): upstream gradients (float64, each may be None) -> ``(gD, gS or None, gH or None)``,
        packed float64 [P], with respect to symmetric ``D``, ``S`` and ``H``."""
        st = self.state
        S = None if S_packed is None else _packed(S_packed, st.P, "S_packed")
        H = None if H_packed is None else _packed(H_packed, st.P, "H_packed")
        Dp = None if D is None else self._f64(D, st.P, "D")
        N, _, mol_ptr, atom_ptr, _ = self._bond_tables(plan)
        gs = [None if g is None else self._f64(g, n, name) for g, n, name in ((g_pop, N, "g_pop"), (g_nelec, st.B, "g_nelec"), (g_eband, st.B, "g_eband"))]
        outs = [self._scratch(st.P), self._scratch(st.P, want_s), self._scratch(st.P, want_h)]
        st.call("nq_orb_population_backward", *[_lib.ptr(g) for g in gs], _lib.ptr(Dp), *_typed(H), *_typed(S), N, _lib.ptr(mol_ptr), _lib.ptr(atom_ptr),
                                              *[_lib.ptr(o) for o in outs])
        return tuple(outs)

    def bond_product(self, D: torch.Tensor, S_packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``P = D S`` per molecule (``nq_orb_bond_product``), packed float64 [P], not symmetric; only the lower triangles of ``D`` and ``S`` are read.
        ``S_packed = None``: ``D`` made symmetric from its lower triangle."""
        st = self.state
        Dp = self._f64(D, st.P, "D")
        S = None if S_packed is None else _packed(S_packed, st.P, "S_packed")
        out = self._scratch(st.P)
        st.call("nq_orb_bond_product", _lib.ptr(Dp), *_typed(S), _lib.ptr(out))
        return out

    def bond_reduce(self, Pm: torch.Tensor, plan, valence: bool = True):
        """``B_AB = sum_{mu in A, nu in B} P_mu,nu P_nu,mu`` and (``valence``) ``V_A = sum_{B != A} B_AB`` (``nq_orb_bond_reduce``) -> ``(bond [Q], valence [N] or
        None)``, float64 on the device; ``bond`` is exactly symmetric inside each molecule's ``[n, n]`` block (``bond_layout``)."""
        st, dev = self.state, self.state.buf.device
        N, Q, mol_ptr, atom_ptr, bond_ptr = self._bond_tables(plan)
        bond = self._scratch(Q)
        val = torch.empty(N, dtype=torch.float64, device=dev) if valence else None
        st.call("nq_orb_bond_reduce", _lib.ptr(self._f64(Pm, st.P, "P")), N, Q, _lib.ptr(mol_ptr), _lib.ptr(atom_ptr), _lib.ptr(bond_ptr), _lib.ptr(bond),
                                      _lib.ptr(val))
        return bond, val

    def bond_orders(self, D: torch.Tensor, plan, S_packed: Optional[torch.Tensor] = None):
        """Mayer bond orders and valences of a packed closed-shell density ``D`` (float64 [P], carrying the factor 2: what ``density()`` returns) ->
        ``(bond [Q], valence [N], P [P])``, float64 on the device: ``P = D S``, ``B_AB = sum_{mu in A, nu in B} P_mu,nu P_nu,mu`` (``B_AA`` included; molecule b's
        table is ``dense_bond_orders(bond, plan.mol_ptr, b)``), ``V_A = sum_{B != A} B_AB``.  ``plan``: the ``BlockAssembler`` / ``IrrepsAssembler`` plan of the batch
        (its ``mol_ptr`` and per-atom ``orb_ptr``).  ``S_packed = None``: the Wiberg index of an orthogonal basis.  An atom with more than 32 orbitals gets NaN
        in its row and column, a molecule the solver failed on NaN in all its entries.  Two launches (three with the valences); nothing is read back."""
        Pm = self.bond_product(D, S_packed)
        bond, val = self.bond_reduce(Pm, plan)
        return bond, val, Pm

    def bond_orders_backward(self, plan, g_bond, g_valence, Pm: torch.Tensor, D=None, S_packed=None, want_d: bool = True, want_s: bool = False, return_e: bool = False):
        """The reverse of ``bond_orders`` (``nq_orb_bond_backward``): upstream gradients ``g_bond`` [Q] and ``g_valence`` [N] (float64, each may be None) and the
        ``P`` of the forward -> ``(gD or None, gS or None)``, packed float64 [P], exactly symmetric, with respect to symmetric ``D`` and ``S``:
        ``sym(E S)`` and ``sym(D E)`` with ``E_mu,nu = (Gamma_AB + Gamma_BA) P_nu,mu``, ``Gamma_AB = g_bond_AB + (A != B) g_valence_A``.  ``want_s`` needs ``D`` and
        ``S_packed``.  ``return_e``: ``E`` as a third member (for tests)."""
        st = self.state
        N, Q, mol_ptr, atom_ptr, bond_ptr = self._bond_tables(plan)
        if not (want_d or want_s):
            raise ValueError("bond_orders_backward: neither gradient is asked for")
        S = None if S_packed is None else _packed(S_packed, st.P, "S_packed")
        if want_s and (S is None or D is None):
            raise ValueError("bond_orders_backward: the gradient of S needs S_packed and D")
        Dp = self._f64(D, st.P, "D") if want_s else None
        gb = None if g_bond is None else self._f64(g_bond, Q, "g_bond")
        gv = None if g_valence is None else self._f64(g_valence, N, "g_valence")
        E, gD, gS = self._scratch(st.P), self._scratch(st.P, want_d), self._scratch(st.P, want_s)
        st.call("nq_orb_bond_backward", _lib.ptr(gb), _lib.ptr(gv), _lib.ptr(self._f64(Pm, st.P, "P")), _lib.ptr(Dp), *_typed(S), N, Q, _lib.ptr(mol_ptr),
                                        _lib.ptr(atom_ptr), _lib.ptr(bond_ptr), _lib.ptr(E), _lib.ptr(gD), _lib.ptr(gS))
        return (gD, gS, E) if return_e else (gD, gS)

    # ---- Löwdin congruences (csrc/orblowdin.hip) ---------------------------------------------------------------------------------------------------------------
    def low_product(self, Msym: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
        """``Y = M X`` per molecule (``nq_orb_low_product``), packed float64 [P], not symmetric: ``Msym`` float32 or float64 [P] and ``X`` float64 [P] are
        symmetric and only their lower triangles are read."""
        st = self.state
        Mp = _packed(Msym, st.P, "M")
        out = self._scratch(st.P)
        st.call("nq_orb_low_product", *_typed(Mp), _lib.ptr(self._f64(X, st.P, "X")), _lib.ptr(out))
        return out

    def low_symprod(self, E: torch.Tensor, X: torch.Tensor, side: int, alpha: float = 1.0) -> torch.Tensor:
        """``alpha sym(X E)`` (``side`` 0) or ``alpha sym(E X)`` (``side`` 1) per molecule (``nq_orb_low_symprod``), packed float64 [P], exactly symmetric: ``E``
        any matrix, ``X`` symmetric, its lower triangle read."""
        st = self.state
        if side not in (0, 1):
            raise ValueError(f"low_symprod: side must be 0 (sym(X E)) or 1 (sym(E X)), not {side!r}")
        out = self._scratch(st.P)
        st.call("nq_orb_low_symprod", _lib.ptr(self._f64(E, st.P, "E")), _lib.ptr(self._f64(X, st.P, "X")), int(side), float(alpha), _lib.ptr(out))
        return out

    def low_symmetrize(self, G: torch.Tensor) -> torch.Tensor:
        """``(G + G^T) / 2`` per molecule (``nq_orb_low_symmetrize``), packed float64 [P], exactly symmetric: one elementwise launch on the device."""
        st = self.state
        out = self._scratch(st.P)
        st.call("nq_orb_low_symmetrize", _lib.ptr(self._f64(G, st.P, "G")), _lib.ptr(out))
        return out

    def sym_congruence(self, X: torch.Tensor, Msym: torch.Tensor):
        """``M^L = X M X`` for symmetric ``X`` (``S^(1/2)`` or ``S^(-1/2)``) and symmetric ``M`` (``D`` or ``H``, float32 or float64) -> ``(M_L, Y)``: ``Y = M X``
        is kept for the reverse, ``M_L = sym(X Y)`` is exactly symmetric.  Two launches."""
        Y = self.low_product(Msym, X)
        return self.low_symprod(Y, X, 0), Y

    def sym_congruence_backward(self, G: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, want_m: bool = True, want_x: bool = True, symmetric: bool = True):
        """The reverse of ``sym_congruence`` for an upstream ``G = dL/dM^L`` -> ``(dL/dM or None, dL/dX or None)``: ``sym(X (G X))`` (two launches) and
        ``Y G + G Y^T = 2 sym(Y G)`` (one), packed float64 [P], exactly symmetric.  ``symmetric=True`` (the default): ``G`` is symmetric and its lower triangle
        is read; ``False``: any matrix, made symmetric first by one ``nq_orb_low_symmetrize`` launch."""
        if not (want_m or want_x):
            raise ValueError("sym_congruence_backward: neither gradient is asked for")
        if not symmetric:
            G = self.low_symmetrize(G)
        gM = self.low_symprod(self.low_product(G, X), X, 0) if want_m else None
        gX = self.low_symprod(Y, G, 1, 2.0) if want_x else None
        return gM, gX

    # ---- SCF residual (csrc/orbcomm.hip) -------------------------------------------------------------------------------------------------------------------------
    def commutator(self, X: torch.Tensor, Y: torch.Tensor, x_anti: bool = False, alpha: float = 1.0) -> torch.Tensor:
        """``alpha (X Y - Y X)`` per molecule (``nq_orb_comm_product``), packed float64 [P].  ``Y`` is symmetric, its lower triangle is read.  ``x_anti=False``:
        ``X`` symmetric (lower triangle read), the result exactly antisymmetric with a ``+0.0`` diagonal; ``x_anti=True``: ``X`` antisymmetric (strict lower
        triangle read, the mirrored element is the negated one, the stored diagonal is ignored), the result exactly symmetric.  Only the layout of the state
        is read: no solve is needed."""
        st = self.state
        out = self._scratch(st.P)
        st.call("nq_orb_comm_product", _lib.ptr(self._f64(X, st.P, "X")), int(bool(x_anti)), _lib.ptr(self._f64(Y, st.P, "Y")), float(alpha), _lib.ptr(out))
        return out

    def antisymmetrize(self, G: torch.Tensor) -> torch.Tensor:
        """``(G - G^T) / 2`` per molecule (``nq_orb_comm_antisymmetrize``), packed float64 [P], exactly antisymmetric with a ``+0.0`` diagonal."""
        st = self.state
        out = self._scratch(st.P)
        st.call("nq_orb_comm_antisymmetrize", _lib.ptr(self._f64(G, st.P, "G")), _lib.ptr(out))
        return out

    def commutator_norms(self, R: torch.Tensor):
        """``(sum_ij R_ij^2, max_ij |R_ij|)`` per molecule over the whole block (``nq_orb_comm_norms``), float64 [B] each on the device; the maximum of an SCF
        residual is the DIIS error.  A molecule with ``status != 0`` or a NaN entry gets NaN in both."""
        st = self.state
        sumsq, maxabs = self._scratch(st.B), self._scratch(st.B)
        st.call("nq_orb_comm_norms", _lib.ptr(self._f64(R, st.P, "R")), _lib.ptr(sumsq), _lib.ptr(maxabs))
        return sumsq, maxabs


class BatchedOrbitals(_LayoutLaunches):
    """Orbital energies and coefficients of every molecule of a batch.

    ``BatchedOrbitals(orb_ptr)``: ``orb_ptr`` [B+1] (host array or tensor), or a ``BlockAssembler`` / ``IrrepsAssembler`` plan (its ``mol_orb_ptr``).
    ``solve(H_packed, S_packed=None)`` launches the solver on the current stream and returns ``self``; nothing is read back.  ``energies`` [M] and
    ``coefficients`` [P] stay on the device (float64; row k of a molecule's block = orbital k).  ``per_molecule()`` -> (list of [m], list of [m, m] with the
    orbitals as columns).  ``frontier(n_occ)`` -> (homo, lumo, gap), float64 [B] on the device.  ``check()`` reads the status once (a host synchronisation)
    and raises ``RuntimeError`` naming the molecule and the pivot where S was not positive definite.  Inputs are detached: no gradient flows through
    (``nabladft_amd.orbital_loss.orbital_energies`` is the differentiable call).  ``density(n_occ)`` / ``populations(D, plan, S, H)`` / ``weighted_gram(w)``:
    density matrices, Mulliken populations and weighted Gram products of the solved coefficients, on the device.  ``fermi(n_elec, kT)`` /
    ``smeared_density(occ)`` / ``smeared_response(G, fermi_result, ...)``: Fermi-Dirac occupations, their density and its gradient chain; ``check()`` also
    reports the ``info`` of the last ``fermi``."""

    def __init__(self, orb_ptr, device="cuda"):
        self.state = OrbitalState(orb_ptr, device)

    def solve(self, H_packed: torch.Tensor, S_packed: Optional[torch.Tensor] = None) -> "BatchedOrbitals":
        self.state.solve(H_packed, S_packed)
        return self

    energies = property(lambda self: self.state.eps)
    coefficients = property(lambda self: self.state.coeff)
    status = property(lambda self: self.state.status)
    info = property(lambda self: self.state.info)
    iters = property(lambda self: self.state.iters)
    orb_ptr = property(lambda self: self.state.orb_ptr_host)
    pack_ptr = property(lambda self: self.state.pack_ptr_host)

    def per_molecule(self):
        st = self.state
        eps = [st.eps[int(a):int(b)] for a, b in zip(st.orb_ptr_host[:-1], st.orb_ptr_host[1:])]
        coeff = [st.coeff[int(a):int(b)].view(int(m), int(m)).t() for a, b, m in zip(st.pack_ptr_host[:-1], st.pack_ptr_host[1:], st.m)]
        return eps, coeff

    def dense_coefficients(self, dtype=torch.float64) -> torch.Tensor:
        """Block-diagonal [M, M] with the orbitals as COLUMNS of each molecule's block (the layout of PhiSNet's ``orbital_coefficients``); no host read."""
        st, dev = self.state, self.state.buf.device
        m = torch.from_numpy(st.m).to(dev)
        b = torch.repeat_interleave(torch.arange(st.B, device=dev), m * m, output_size=st.P)
        loc = torch.arange(st.P, device=dev) - st.pack_ptr[b]
        o = st.orb_ptr.long()[b]
        dense = torch.zeros(st.M, st.M, dtype=dtype, device=dev)
        dense[o + loc % m[b], o + loc // m[b]] = st.coeff.to(dtype)
        return dense

    def frontier(self, n_occ):
        st = self.state
        no = torch.from_numpy(check_occupied(n_occ, st.orb_ptr_host)).to(st.buf.device)
        out = torch.empty(3, st.B, dtype=torch.float64, device=st.buf.device)
        st.call("nq_orb_frontier", _lib.ptr(no), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]))
        return out[0], out[1], out[2]

    def compare(self, target: "BatchedOrbitals", n_occ, S_packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """This (predicted) solution against ``target`` under the common ``S`` -> float64 [7, B] on the device, rows in the order of ``FIGURES``."""
        st, tt = self.state, target.state
        if st._dims != tt._dims or not np.array_equal(st.orb_ptr_host, tt.orb_ptr_host):
            raise ValueError("the two solutions belong to different batches")
        no = torch.from_numpy(check_occupied(n_occ, st.orb_ptr_host)).to(st.buf.device)
        S = None if S_packed is None else _packed(S_packed, st.P, "S_packed")
        out = torch.empty(len(FIGURES), st.B, dtype=torch.float64, device=st.buf.device)
        with torch.cuda.device(st.buf.device):
            # two states in front of the dimensions: the one launch that is not OrbitalState.call
            _lib.check(_lib.load().nq_orb_compare(_lib.ptr(st.buf), _lib.ptr(tt.buf), *st._dims, *_typed(S), _lib.ptr(no), _lib.ptr(out), _lib.stream_ptr()))
        return out

    def weighted_gram(self, w0: torch.Tensor, w1: Optional[torch.Tensor] = None, k_lo=None, k_hi=None):
        """``X_b = sum_{k in [lo_b, hi_b)} w[k] c_k c_k^T`` of every molecule from the coefficients of the last solve, one launch (``nq_orb_wgram``): packed float64
        [P], exactly symmetric; with ``w1`` a pair from the same operand loads.  ``w*``: float64 [M] on the device; ``k_lo`` / ``k_hi``: int32 [B] on the device or
        None (0 and m).  A molecule the solver failed on gets NaN.  Nothing is read back."""
        st, dev = self.state, self.state.buf.device
        ws = []
        for name, w in (("w0", w0), ("w1", w1)):
            if w is None:
                ws.append(None)
                continue
            _require_gpu(w)
            if w.dtype != torch.float64 or w.numel() != st.M or w.device != dev:
                raise ValueError(f"{name} must be float64 [{st.M}] on {dev}")
            ws.append(w.detach().reshape(-1).contiguous())
        ks = []
        for name, k in (("k_lo", k_lo), ("k_hi", k_hi)):
            if k is not None and (not isinstance(k, torch.Tensor) or k.dtype != torch.int32 or k.numel() != st.B or k.device != dev):
                raise ValueError(f"{name} must be an int32 [{st.B}] tensor on {dev}")
            ks.append(None if k is None else k.contiguous())
        out0 = torch.empty(st.P, dtype=torch.float64, device=dev)
        out1 = None if ws[1] is None else torch.empty(st.P, dtype=torch.float64, device=dev)
        st.call("nq_orb_wgram", _lib.ptr(ws[0]), _lib.ptr(ws[1]), _lib.ptr(ks[0]), _lib.ptr(ks[1]), _lib.ptr(out0), _lib.ptr(out1))
        return out0 if out1 is None else (out0, out1)

    def density(self, n_occ, energy_weighted: bool = False):
        """The closed-shell density matrix ``D = 2 sum_{k < n_occ} c_k c_k^T`` of every molecule, packed float64 [P] like the input; with ``energy_weighted`` also
        ``W = 2 sum_{k < n_occ} eps_k c_k c_k^T`` -> ``(D, W)``.  ``n_occ``: [B], checked on the host against the orbital counts."""
        st = self.state
        no = torch.from_numpy(check_occupied(n_occ, st.orb_ptr_host)).to(st.buf.device)
        two = torch.full((st.M,), 2.0, dtype=torch.float64, device=st.buf.device)
        return self.weighted_gram(two, 2.0 * st.eps if energy_weighted else None, None, no)

    # ---- the density response (csrc/orbresp.hip): thin launches; nabladft_amd.orbital_loss chains them -------------------------------------------------------
    def occupied_layout(self, n_occ):
        """The occupied-packed layout of the response's scratch arrays -> ``(n_occ int32 [B], occ_ptr int64 [B+1], O)``, the first two on the device:
        molecule b owns ``n_occ_b m_b`` doubles at ``occ_ptr[b]``.  ``n_occ`` is checked on the host against the orbital counts."""
        st = self.state
        no = check_occupied(n_occ, st.orb_ptr_host)
        occ = np.concatenate([[0], np.cumsum(no.astype(np.int64) * st.m)]).astype(np.int64)
        return torch.from_numpy(no).to(st.buf.device), torch.from_numpy(occ).to(st.buf.device), int(occ[-1])

    def resp_project(self, G: torch.Tensor, layout) -> torch.Tensor:
        """``T = Gs C_o`` with ``Gs = (G + G^T) / 2`` (``nq_orb_resp_project``): ``G`` packed float64 [P], any matrix -> occupied-packed [m][n_occ], float64 [O]."""
        P = self.state.P
        Gs, T = self._scratch(P), self._scratch(layout[2])
        self.state.call("nq_orb_resp_project", *_ptrs(layout[:2]), layout[2], *_ptrs([self._f64(G, P, "G"), Gs, T]))
        return T

    def resp_mo(self, T: torch.Tensor, layout, overlap: bool = True):
        """``W = C^T T`` divided by the occupied-virtual differences (``nq_orb_resp_mo``) -> ``(A_H, A_S or None)``, occupied-packed [m][n_occ]."""
        O = layout[2]
        outs = self._scratch(O), self._scratch(O, overlap)
        self.state.call("nq_orb_resp_mo", *_ptrs(layout[:2]), O, *_ptrs((self._f64(T, O, "T"),) + outs))
        return outs

    def resp_back(self, A_H: torch.Tensor, A_S: Optional[torch.Tensor], layout):
        """``Rt_X = A_X^T C^T`` (``nq_orb_resp_back``) -> ``(Rt_H, Rt_S or None)``, occupied-packed [n_occ][m]; both from the same loads of the coefficients."""
        O = layout[2]
        ins = self._f64(A_H, O, "A_H"), None if A_S is None else self._f64(A_S, O, "A_S")
        outs = self._scratch(O), self._scratch(O, A_S is not None)
        self.state.call("nq_orb_resp_back", *_ptrs(layout[:2]), O, *_ptrs(ins + outs))
        return outs

    def syr2k(self, Rt0: torch.Tensor, Rt1: Optional[torch.Tensor], layout):
        """``X = 1/2 sum_{i < n_occ} (r_i c_i^T + c_i r_i^T)`` (``nq_orb_syr2k``) -> ``(X0, X1 or None)``, packed float64 [P], exactly symmetric."""
        O, P = layout[2], self.state.P
        ins = self._f64(Rt0, O, "Rt0"), None if Rt1 is None else self._f64(Rt1, O, "Rt1")
        outs = self._scratch(P), self._scratch(P, Rt1 is not None)
        self.state.call("nq_orb_syr2k", *_ptrs(layout[:2]), O, *_ptrs(ins + outs))
        return outs

    def density_response(self, G: torch.Tensor, n_occ_or_layout, overlap: bool = True):
        """``dL/dH`` and (``overlap``) ``dL/dS`` of a loss with ``dL/dD = G`` on the density ``density(n_occ)`` of the last solve: the four launches above ->
        ``(gH, gS or None)``, packed float64 [P], symmetric matrices in the convention of ``weighted_gram``.  Nothing is read back."""
        layout = n_occ_or_layout if isinstance(n_occ_or_layout, tuple) else self.occupied_layout(n_occ_or_layout)
        A_H, A_S = self.resp_mo(self.resp_project(G, layout), layout, overlap)
        return self.syr2k(*self.resp_back(A_H, A_S, layout), layout)

    # ---- Fermi-Dirac smearing (csrc/orbsmear.hip) ------------------------------------------------------------------------------------------------------------
    def _per_molecule(self, v, name: str) -> torch.Tensor:
        st, dev = self.state, self.state.buf.device
        if isinstance(v, torch.Tensor):
            t = v.detach().to(device=dev, dtype=torch.float64).reshape(-1)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))).to(dev)
        if t.numel() == 1:
            t = t.expand(st.B)
        if t.numel() != st.B:
            raise ValueError(f"{name} must be one number or one per molecule ({st.B}), not {t.numel()}")
        return t.contiguous()

    def fermi(self, n_elec, kT) -> FermiResult:
        """Fermi-Dirac occupations of the last solve (``nq_orb_fermi``): ``n_elec`` electrons per molecule (``electron_counts``; any number in (0, 2m)) and
        the temperature ``kT`` > 0 in the energy unit of H, each one number or one per molecule -> ``FermiResult``.  Nothing is read back: a molecule with
        ``n_elec`` outside (0, 2m), ``kT`` not a positive finite number (or >= 1e300) or a failed solve gets ``info = 1`` and NaN, which ``check()`` reports."""
        st, dev = self.state, self.state.buf.device
        ne, kt = self._per_molecule(n_elec, "n_elec"), self._per_molecule(kT, "kT")
        mu, ent = self._scratch(st.B), self._scratch(st.B)
        occ, docc = self._scratch(st.M), self._scratch(st.M)
        info = torch.empty(st.B, dtype=torch.int32, device=dev)
        st.call("nq_orb_fermi", _lib.ptr(ne), _lib.ptr(kt), _lib.ptr(mu), _lib.ptr(occ), _lib.ptr(docc), _lib.ptr(ent), _lib.ptr(info))
        self._fermi_info = info
        return FermiResult(mu, occ, docc, ent, info, ne, kt)

    def smeared_density(self, occ: torch.Tensor, energy_weighted: bool = False):
        """``D = sum_k F_k c_k c_k^T`` over ALL orbitals for the occupations ``occ`` [M] of ``fermi`` (one ``nq_orb_wgram`` launch), packed float64 [P], exactly
        symmetric; with ``energy_weighted`` also ``sum_k F_k eps_k c_k c_k^T`` -> ``(D, W)``."""
        F = self._f64(occ, self.state.M, "occ")
        return self.weighted_gram(F, F * self.state.eps if energy_weighted else None)

    def full_layout(self):
        """The layout that makes the closed-shell launches run over all orbitals: ``(n_occ = m, occ_ptr = pack_ptr, O = P)``."""
        st = self.state
        if getattr(self, "_full", None) is None:
            self._full = (torch.from_numpy(st.m.astype(np.int32)).to(st.buf.device), st.pack_ptr, st.P)
        return self._full

    def smear_mo(self, T: torch.Tensor, fermi_result: FermiResult, overlap: bool = True):
        """``W = C^T T`` times the divided differences of F (``nq_orb_smear_mo``) -> ``(A_H, A_S or None, wdiag)``: packed [m][m] without their diagonals, which
        ``smear_diag`` writes, and ``wdiag`` [M] = ``W_kk``."""
        st = self.state
        out = [self._scratch(st.P), self._scratch(st.P, overlap), self._scratch(st.M)]
        st.call("nq_orb_smear_mo", *_ptrs([fermi_result.mu, fermi_result.kT, self._f64(T, st.P, "T")] + out))
        return tuple(out)

    def smear_diag(self, A_H: torch.Tensor, A_S: Optional[torch.Tensor], wdiag: torch.Tensor, fermi_result: FermiResult, g_eps=None, g_occ=None, g_mu=None, g_ent=None):
        """The diagonals of ``A_H`` / ``A_S`` in place (``nq_orb_smear_diag``) from ``wdiag`` and the upstream gradients of ``eps`` [M], ``occ`` [M], ``mu`` [B] and
        ``entropy`` [B] (each may be None) -> ``(A_H, A_S)``."""
        st, fr = self.state, fermi_result
        gs = [None if g is None else self._f64(g, n, name) for g, n, name in ((g_eps, st.M, "g_eps"), (g_occ, st.M, "g_occ"), (g_mu, st.B, "g_mu"), (g_ent, st.B, "g_ent"))]
        st.call("nq_orb_smear_diag", *_ptrs([fr.mu, fr.kT, fr.occ, fr.docc, self._f64(wdiag, st.M, "wdiag")] + gs +
                                            [self._f64(A_H, st.P, "A_H"), None if A_S is None else self._f64(A_S, st.P, "A_S")]))
        return A_H, A_S

    def smear_back(self, A_H: torch.Tensor, A_S: Optional[torch.Tensor]):
        """``Rt_X = A_X^T C^T`` over all orbitals (``nq_orb_smear_back``) -> ``(Rt_H, Rt_S or None)``, packed [m][m]; both from the same loads of the coefficients."""
        P = self.state.P
        out = [self._scratch(P), self._scratch(P, A_S is not None)]
        self.state.call("nq_orb_smear_back", *_ptrs([self._f64(A_H, P, "A_H"), None if A_S is None else self._f64(A_S, P, "A_S")] + out))
        return tuple(out)

    def smeared_response(self, G: Optional[torch.Tensor], fermi_result: FermiResult, g_eps=None, g_occ=None, g_mu=None, g_ent=None, overlap: bool = True):
        """``dL/dH`` and (``overlap``) ``dL/dS`` of a loss with upstream gradients ``G = dL/dD`` [P] (any matrix), ``g_eps`` [M], ``g_occ`` [M], ``g_mu`` [B],
        ``g_ent`` [B] (each may be None) on the results of ``fermi`` / ``smeared_density`` of the last solve -> ``(gH, gS or None)``, packed float64 [P],
        symmetric matrices in the convention of ``weighted_gram``.  ``T = Gs C`` (``nq_orb_resp_project`` over all orbitals), ``A = K o (C^T T)``
        (``nq_orb_smear_mo``), its diagonal (``nq_orb_smear_diag``), ``A^T C^T`` (``nq_orb_smear_back``) and ``C A C^T`` (``nq_orb_syr2k`` over all orbitals):
        ``K`` holds the divided differences of F, evaluated without dividing by a difference of orbital energies, so coincident and crossed levels give finite
        gradients.  Without ``G`` the matrix ``A`` is diagonal and the result ``sum_k A_kk c_k c_k^T``: ``nq_orb_smear_diag`` and ONE ``nq_orb_wgram`` launch.
        Nothing is read back."""
        st, layout = self.state, self.full_layout()
        if G is None:
            if getattr(self, "_diag_index", None) is None:       # where element (k, k) of every block sits in a packed array
                k = np.arange(st.M) - np.repeat(st.orb_ptr_host[:-1], st.m)
                self._diag_index = torch.from_numpy(np.repeat(st.pack_ptr_host[:-1], st.m) + k * (np.repeat(st.m, st.m) + 1)).to(st.buf.device)
            A_H, A_S = self._scratch(st.P), self._scratch(st.P, overlap)
            self.smear_diag(A_H, A_S, torch.zeros(st.M, dtype=torch.float64, device=st.buf.device), fermi_result, g_eps, g_occ, g_mu, g_ent)
            if not overlap:
                return self.weighted_gram(A_H[self._diag_index]), None
            return self.weighted_gram(A_H[self._diag_index], A_S[self._diag_index])
        A_H, A_S, wdiag = self.smear_mo(self.resp_project(G, layout), fermi_result, overlap)
        self.smear_diag(A_H, A_S, wdiag, fermi_result, g_eps, g_occ, g_mu, g_ent)
        return self.syr2k(*self.smear_back(A_H, A_S), layout)

    # ---- Löwdin analysis (csrc/orblowdin.hip): what reads the levels of S; the congruences are _LayoutLaunches' --------------------------------------------------
    def overlap_weights(self):
        """After a STANDARD solve of ``S`` itself (``solve(S_packed)``: ``energies`` = the levels ``s`` of ``S``): ``a = sqrt(s)`` and ``1 / a`` float64 [M],
        ``cond = s_max / s_min`` float64 [B] and ``info`` int32 [B] (``nq_orb_low_weights``) -> ``(w_half, w_inv_half, cond, info)`` on the device.  A molecule
        the solver failed on, or with a level that is not finite or not positive, gets ``info = 1`` and NaN.  Nothing is read back."""
        st, dev = self.state, self.state.buf.device
        half, inv = self._scratch(st.M), self._scratch(st.M)
        cond = self._scratch(st.B)
        info = torch.empty(st.B, dtype=torch.int32, device=dev)
        st.call("nq_orb_low_weights", _lib.ptr(half), _lib.ptr(inv), _lib.ptr(cond), _lib.ptr(info))
        return half, inv, cond, info

    def overlap_functions(self):
        """``S^(1/2)`` and ``S^(-1/2)`` of every molecule after a standard solve of ``S`` -> ``(half, inv_half, cond, info)``: the two packed float64 [P], exactly
        symmetric, from ``overlap_weights`` and ONE ``nq_orb_wgram`` launch; ``info = 1``: NaN in that molecule's blocks."""
        w_half, w_inv, cond, info = self.overlap_weights()
        half, inv = self.weighted_gram(w_half, w_inv)
        return half, inv, cond, info

    def low_mo(self, T: torch.Tensor, kind: int) -> torch.Tensor:
        """``K o (U^T T)``, the diagonal included (``nq_orb_low_mo``), packed float64 [P]; ``kind`` 0: ``K_ij = 1 / (a_i + a_j)``, 1: ``-1 / (a_i a_j (a_i + a_j))``."""
        st = self.state
        if kind not in (0, 1):
            raise ValueError(f"low_mo: kind must be 0 (S^(1/2)) or 1 (S^(-1/2)), not {kind!r}")
        out = self._scratch(st.P)
        st.call("nq_orb_low_mo", int(kind), _lib.ptr(self._f64(T, st.P, "T")), _lib.ptr(out))
        return out

    def matfun_response(self, g: torch.Tensor, kind: int) -> torch.Tensor:
        """``dL/dS`` of a loss with ``dL/dX = g`` (any matrix; its symmetric part counts) on ``X = S^(1/2)`` (``kind`` 0) or ``S^(-1/2)`` (``kind`` 1) after a
        standard solve of ``S``: ``U [K o (U^T sym(g) U)] U^T`` in four launches over all orbital pairs -- ``nq_orb_resp_project``, ``nq_orb_low_mo``,
        ``nq_orb_smear_back``, ``nq_orb_syr2k`` -> packed float64 [P], exactly symmetric.  No difference of levels is divided: equal levels of ``S`` give
        finite gradients."""
        layout = self.full_layout()
        A = self.low_mo(self.resp_project(g, layout), kind)
        return self.syr2k(self.smear_back(A, None)[0], None, layout)[0]

    def check(self) -> "BatchedOrbitals":
        st = self.state
        bad = st.first_failure()
        if bad:
            b, status = bad
            raise RuntimeError(_failure_text(b, status, int(st.info[b]), int(st.m[b])))
        info = getattr(self, "_fermi_info", None)
        if info is not None:
            bad = np.nonzero(info.cpu().numpy())[0]
            if bad.size:
                raise RuntimeError(f"molecule {int(bad[0])}: no Fermi occupations (info 1): n_elec outside (0, 2m), kT not a positive finite number or "
                                   "non-finite orbital energies")
        return self


class LowdinBasis:
    """The symmetric orthogonalisation of a batch, reusable for prediction and target of a step and, since ``S`` belongs to the conformer, across epochs:
    ``orbitals`` (the ``BatchedOrbitals`` that holds the decomposition ``S = U diag(s) U^T``), ``half`` = ``S^(1/2)`` and ``inv_half`` = ``S^(-1/2)`` packed
    float64 [P] on the device, ``s`` [M] (ascending inside each molecule), ``cond`` = ``s_max / s_min`` [B] and ``info`` int32 [B] (1: ``S`` is not positive
    definite or its solve failed; NaN in that molecule's blocks).  ``LowdinBasis.of(S_packed, orb_ptr)`` builds one without gradients
    (``nabladft_amd.orbital_loss.lowdin_basis`` is the differentiable call).  ``check()`` reads the status once (a host synchronisation) and raises
    ``RuntimeError`` naming the molecule."""

    def __init__(self, orbitals: "BatchedOrbitals", half: torch.Tensor, inv_half: torch.Tensor, cond: torch.Tensor, info: torch.Tensor):
        self.orbitals, self.half, self.inv_half, self.cond, self.info = orbitals, half, inv_half, cond, info

    orb_ptr = property(lambda self: self.orbitals.orb_ptr)
    root = None                   # the BatchedMatrixRoot behind a basis of method "newton_schulz"

    @property
    def s(self):
        if self.root is not None:
            raise RuntimeError("LowdinBasis.s: a basis of method \"newton_schulz\" has no levels of S: there are none without a decomposition (use method=\"eigh\")")
        return self.orbitals.energies

    @classmethod
    def of(cls, S_packed: torch.Tensor, plan_or_orb_ptr, method: str = "eigh", max_iter: int = 100) -> "LowdinBasis":
        """``method="eigh"``: one standard solve of ``S`` (latency-bound) and its functions.  ``method="newton_schulz"``: ``BatchedMatrixRoot`` -- matrix
        products alone, nothing is solved; ``orbitals`` is then a layout-only ``BatchedOrbitals`` (it serves the congruence and commutator launches), ``cond``
        is None, ``s`` raises, ``info`` is the iteration's status (1: the row sums of ``S`` are unusable, 4: not converged in ``max_iter`` iterations: ``S``
        is not positive definite, or ``kappa_2(S)`` is beyond about 1e8) and ``check()`` names the molecule.  Neither carries a gradient of ``S``."""
        _require_gpu(S_packed)
        if method == "eigh":
            orb = BatchedOrbitals(plan_or_orb_ptr, S_packed.device).solve(S_packed)
            return cls(orb, *orb.overlap_functions())
        if method != "newton_schulz":
            raise ValueError(f"LowdinBasis.of: method must be \"eigh\" or \"newton_schulz\", not {method!r}")
        orb = BatchedOrbitals(plan_or_orb_ptr, S_packed.device)
        root = BatchedMatrixRoot(orb.orb_ptr, S_packed.device, state=orb.state).run(S_packed, max_iter)
        basis = cls(orb, root.half, root.inv_half, None, root.status)
        basis.root = root
        return basis

    def check(self) -> "LowdinBasis":
        if self.root is not None:
            self.root.check()
            return self
        self.orbitals.check()
        bad = np.nonzero(self.info.cpu().numpy())[0]
        if bad.size:
            b = int(bad[0])
            st = self.orbitals.state
            lo = float(st.eps[int(st.orb_ptr_host[b])])
            raise RuntimeError(f"molecule {b}: the overlap matrix is not positive definite (its lowest level is {lo:g}): no S^(1/2) (info 1)")
        return self


class BatchedMatrixRoot:
    """``S^(1/2)`` and ``S^(-1/2)`` of every molecule of a batch WITHOUT a decomposition: the coupled Newton-Schulz iteration on the float64 matrix cores
    (csrc/orbsqrt.hip).

    ``BatchedMatrixRoot(orb_ptr, device)`` as ``BatchedOrbitals`` (``state=``: an existing ``OrbitalState`` of the batch, whose layout and status words are
    then used and whose matrices are left alone).  ``run(S_packed, max_iter=100)`` enqueues the scaling ``Y_0 = S / c`` (``c`` = the largest absolute row
    sum), ``max_iter`` iterations ``T = (3 I - Z Y) / 2``, ``Y <- Y T``, ``Z <- T Z`` (two launches each; the workgroups of a finished molecule exit at once)
    and the final scaling on the current stream and returns ``self``; nothing is read back.  ``prepare(S_packed, max_iter)`` / ``step(k)`` / ``finish()`` are
    its parts (for tests: the steps in order from 0).  ``half`` / ``inv_half``: packed float64 [P], exactly symmetric.  ``iterations`` / ``status`` / ``info``
    int32 [B] and ``residuals`` float64 [B, max_iter] (``delta_k = m - tr(Z_k Y_k)``) on the device.  ``check()`` reads the status once (a host
    synchronisation) and raises ``RuntimeError`` naming the molecule whose ``S`` has unusable row sums (status 1) or did not converge (status 4: ``S`` is not
    positive definite); such a molecule has NaN in its own blocks only.  Only the lower triangle of ``S`` (float32 or float64) is read.

    About 18 iterations at ``kappa_2(S) = 1e4``, 25 at 1e6, 32 at 1e8; the stopping rule is meant for ``kappa_2(S) <= 1e8``.  Accuracy against a
    decomposition: a fraction of ``m 2^-52 kappa_2(S) max|entry|``.  No gradient of ``S``."""

    CTL = 24

    def __init__(self, orb_ptr, device="cuda", state: Optional[OrbitalState] = None):
        self.state = OrbitalState(orb_ptr, device) if state is None else state
        if state is not None and not np.array_equal(state.orb_ptr_host, _orb_ptr_of(orb_ptr)):
            raise ValueError("BatchedMatrixRoot: the state belongs to another batch")
        self._max_iter = None
        self.half = self.inv_half = None

    status = property(lambda self: self.state.status)
    info = property(lambda self: self.state.info)
    iterations = property(lambda self: self.state.iters)
    orb_ptr = property(lambda self: self.state.orb_ptr_host)
    pack_ptr = property(lambda self: self.state.pack_ptr_host)

    @property
    def residuals(self) -> torch.Tensor:
        self._prepared()
        return self.ctl[:, self.CTL:]

    def _prepared(self):
        if self._max_iter is None:
            raise RuntimeError("BatchedMatrixRoot: prepare() or run() first")

    def _iterates(self):
        return [_lib.ptr(t) for t in (self.Y, self.Z, self.T, self.Y2, self.Z2)]

    def prepare(self, S_packed: torch.Tensor, max_iter: int = 100) -> "BatchedMatrixRoot":
        """``nq_orb_sqrt_init``: ``c``, ``Y_0 = S / c``, ``Z_0 = I``, cleared ``ctl`` / ``log``, the status words."""
        st, dev = self.state, self.state.buf.device
        S = _packed(S_packed, st.P, "S_packed")
        if S.device != dev:
            raise ValueError(f"the matrices must live on {dev}")
        max_iter = int(max_iter)
        if not 1 <= max_iter <= 10000:
            raise ValueError(f"max_iter={max_iter} outside 1..10000")
        f64 = torch.float64
        self.Y, self.Z, self.T, self.Y2, self.Z2 = (torch.empty(st.P, dtype=f64, device=dev) for _ in range(5))
        self.ctl = torch.empty(st.B, self.CTL + max_iter, dtype=f64, device=dev)
        self.log = torch.empty(st.B, max_iter, dtype=torch.int32, device=dev)
        self.half = self.inv_half = None
        self._max_iter = max_iter
        self.state.call("nq_orb_sqrt_init", *_typed(S), max_iter, _lib.ptr(self.Y), _lib.ptr(self.Z), _lib.ptr(self.ctl), _lib.ptr(self.log))
        return self

    def step(self, k: int) -> "BatchedMatrixRoot":
        """Exactly one iteration, number ``k`` (``nq_orb_sqrt_step``; for tests: call them in order from 0)."""
        self._prepared()
        self.state.call("nq_orb_sqrt_step", int(k), self._max_iter, *self._iterates(), _lib.ptr(self.ctl), _lib.ptr(self.log))
        return self

    def finish(self) -> "BatchedMatrixRoot":
        """``nq_orb_sqrt_finish``: ``half`` and ``inv_half`` from the current iterates, status 4 and NaN for a molecule that did not stop."""
        self._prepared()
        st = self.state
        self.half, self.inv_half = (torch.empty(st.P, dtype=torch.float64, device=st.buf.device) for _ in range(2))
        self.state.call("nq_orb_sqrt_finish", self._max_iter, _lib.ptr(self.Y), _lib.ptr(self.Z), _lib.ptr(self.Y2), _lib.ptr(self.Z2), _lib.ptr(self.ctl),
                     _lib.ptr(self.log), _lib.ptr(self.half), _lib.ptr(self.inv_half))
        return self

    def run(self, S_packed: torch.Tensor, max_iter: int = 100) -> "BatchedMatrixRoot":
        self.prepare(S_packed, max_iter)
        self.state.call("nq_orb_sqrt_run", self._max_iter, *self._iterates(), _lib.ptr(self.ctl), _lib.ptr(self.log))
        self.finish()
        self.Y = self.Z = self.T = self.Y2 = self.Z2 = None            # five [P] arrays nobody needs after the final scaling
        return self

    def check(self) -> "BatchedMatrixRoot":
        self._prepared()
        st = self.state
        bad = st.first_failure()
        if bad:
            b, status = bad
            if status == 1:
                raise RuntimeError(f"molecule {b}: the overlap matrix is not positive definite (its largest absolute row sum is zero or not finite): no "
                                   "S^(1/2) (status 1)")
            if status == 4:
                raise RuntimeError(f"molecule {b}: the Newton-Schulz iteration did not converge in {self._max_iter} iterations: the overlap matrix is not "
                                   "positive definite, or its condition number is beyond about 1e8 (status 4)")
            raise RuntimeError(_failure_text(b, status, int(st.info[b]), int(st.m[b])))
        return self


FrontierLevels = namedtuple("FrontierLevels", "homo lumo gap coeff vectors iterations residual converged")
FrontierLevels.__doc__ = """What ``BatchedPurification.frontier`` returns, all on the device: ``homo`` / ``lumo`` / ``gap`` float64 [B] (NaN where the level does not exist or
the side did not converge), ``coeff`` float64 [2, M] (the levels' coefficient vectors ``c = W^T v`` in the atomic-orbital basis, ``c^T S c = 1``; row 0 HOMO, row 1
LUMO), ``vectors`` float64 [2, M] (``v`` in the orthonormal basis), ``iterations`` int32 [B, 2] (Lanczos steps), ``residual`` float64 [B, 2] (``beta |s_last|`` at
the stop) and ``converged`` int32 [B, 2]: 1 converged, 0 not converged, -1 the level does not exist (HOMO for ``n_occ = 0``, LUMO for ``n_occ = m``)."""


Orthogonalizer = namedtuple("Orthogonalizer", "Z status info orb_ptr")
Orthogonalizer.__doc__ = """What ``BatchedPurification.orthogonalize`` returns, reusable for any purification of the same batch: ``Z`` float64 [P] on the device
(``L^-1`` of ``S = L L^T`` per molecule, lower triangular), ``status`` / ``info`` int32 [B] copies (1: the overlap is not positive definite, ``info`` = the
1-based Cholesky pivot; that molecule's block of ``Z`` is NaN) and the host ``orb_ptr`` it was built for."""


class BatchedPurification(_LayoutLaunches):
    """Closed-shell density matrices of every molecule of a batch and their gradients WITHOUT a solve (csrc/orbpurify.hip).

    ``BatchedPurification(orb_ptr)`` as ``BatchedOrbitals``.  ``orthogonalize(S_packed)`` -> ``Orthogonalizer`` (one latency-bound launch; the object is
    reusable, also by other ``BatchedPurification`` objects of the same batch, and is remembered by this one).  ``purify(H_packed, n_occ, max_iter=100,
    orthogonalizer=None)`` enqueues the congruence ``Z H Z^T``, the bounds and ``max_iter`` SP2 iterations on the current stream and returns ``self``; nothing
    is read back (``orthogonalizer=None``: the one this object made, or the standard problem if it made none).  ``n_occ`` [B] in ``0..m``.  ``density()`` ->
    ``D = 2 Z^T X Z`` packed float64 [P], exactly symmetric.  ``response(G, overlap=True)`` -> ``(dL/dH, dL/dS or None)`` for ``G = dL/dD`` (any matrix), packed
    float64 [P], symmetric matrices in the convention of ``BatchedOrbitals.weighted_gram``; it runs the same ``X`` sequence again along the logged branches
    with no stored iterates, no eigenpairs and no division.  ``iterations`` int32 [B] on the device.  ``check()`` reads the status once (a host
    synchronisation) and raises ``RuntimeError`` naming the molecule whose overlap was not positive definite (status 1) or whose purification did not
    converge (status 4: needs an open gap).  A failed molecule has NaN in its own blocks only.  ``populations`` / ``populations_backward`` / ``bond_orders`` /
    ``bond_orders_backward`` and the layout-only Löwdin launches (``low_product`` / ``low_symprod`` / ``sym_congruence``) are ``BatchedOrbitals``'.  After ``purify``,
    ``frontier(k_max=256, tol=2**-44, transform=None)`` -> ``FrontierLevels``: HOMO, LUMO and the gap by a projected Lanczos recurrence (one launch,
    csrc/orbfrontier.hip); ``transform``: a packed float64 [P] back-transform in place of the orthogonaliser of the last purify (``S^(-1/2)`` after a purification of
    the standard problem in the Löwdin basis).  ``frontier_gradients(levels, g_homo, g_lumo, overlap=True)`` -> ``(dL/dH, dL/dS or None)``;
    ``frontier_check(levels)`` raises naming the first molecule and side that did not converge in ``k_max`` steps.  ``occupied(transform=None)`` ->
    ``OccupiedOrbitals``: all occupied levels and coefficients from a Cholesky factor of ``X`` and an ``n_occ x n_occ`` solve (csrc/orbocc.hip).  No virtual
    level other than the LUMO, no smearing, closed shells only."""

    def __init__(self, orb_ptr, device="cuda"):
        self.state = OrbitalState(orb_ptr, device)
        self.orthogonalizer = None
        self._orth = None          # the one the last purify used
        self._max_iter = None

    status = property(lambda self: self.state.status)
    info = property(lambda self: self.state.info)
    iterations = property(lambda self: self.state.iters)
    orb_ptr = property(lambda self: self.state.orb_ptr_host)
    pack_ptr = property(lambda self: self.state.pack_ptr_host)
    projector = property(lambda self: self.state.coeff)            # X [P]

    def orthogonalize(self, S_packed: torch.Tensor) -> Orthogonalizer:
        st = self.state
        S = _packed(S_packed, st.P, "S_packed")
        if S.device != st.buf.device:
            raise ValueError(f"the matrices must live on {st.buf.device}")
        Z = self._scratch(st.P)
        self.state.call("nq_orb_pur_orthogonalizer", *_typed(S), _lib.ptr(Z))
        self.orthogonalizer = Orthogonalizer(Z, st.status.clone(), st.info.clone(), st.orb_ptr_host)
        return self.orthogonalizer

    def congruence(self, Z: Optional[torch.Tensor], A: torch.Tensor, trans: bool, alpha: float = 1.0, symmetrize: bool = False, out: Optional[torch.Tensor] = None):
        """``alpha sym(Z A Z^T)`` (``trans`` False) or ``alpha sym(Z^T A Z)`` (``nq_orb_pur_congruence``) -> packed float64 [P], exactly symmetric.  ``A``: float32 or
        float64 [P]; its lower triangle is read, or ``(A + A^T) / 2`` with ``symmetrize``.  ``Z = None``: ``alpha A`` made symmetric."""
        st = self.state
        Ap = _packed(A, st.P, "A")
        out = self._scratch(st.P) if out is None else out
        tmp = None if Z is None else self._scratch(st.P)
        self.state.call("nq_orb_pur_congruence", _lib.ptr(Z), int(bool(trans)), *_typed(Ap), int(bool(symmetrize)), float(alpha),
                   _lib.ptr(tmp), _lib.ptr(out))
        return out

    def gemm(self, A: torch.Tensor, Bm: torch.Tensor, C: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 1.0) -> torch.Tensor:
        """``alpha A B + beta C`` per molecule (``nq_orb_pur_gemm``), packed float64 [P]."""
        P = self.state.P
        out = self._scratch(P)
        self.state.call("nq_orb_pur_gemm", _lib.ptr(self._f64(A, P, "A")), _lib.ptr(self._f64(Bm, P, "B")), _lib.ptr(None if C is None else self._f64(C, P, "C")),
                   float(alpha), float(beta), _lib.ptr(out))
        return out

    def _occupied(self, n_occ) -> torch.Tensor:
        st = self.state
        no = _host_ptr(n_occ).astype(np.int32)
        if no.shape != st.m.shape:
            raise ValueError(f"n_occ has {no.shape[0]} entries for {st.m.shape[0]} molecules")
        bad = np.nonzero((no < 0) | (no > st.m))[0]
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"molecule {b}: n_occ={int(no[b])} outside 0..m={int(st.m[b])}")
        self._n_occ_host = no.astype(np.int64)                       # occupied() sizes its reduced layout by it without a read-back
        return torch.from_numpy(no).to(st.buf.device)

    def _orthogonalizer(self, orth):
        orth = self.orthogonalizer if orth is None else orth
        if orth is not None and (not np.array_equal(orth.orb_ptr, self.state.orb_ptr_host) or orth.Z.device != self.state.buf.device):
            raise ValueError("the orthogonalizer belongs to another batch")
        return orth

    def prepare(self, H_packed: torch.Tensor, n_occ, max_iter: int = 100, orthogonalizer: Optional[Orthogonalizer] = None) -> "BatchedPurification":
        """What ``purify`` does before the iterations (``nq_orb_pur_congruence``, ``nq_orb_pur_init``): ``Ht`` into the state, the bounds, ``X_0``, the trivial
        cases, cleared ``ctl`` / ``log``."""
        st, dev = self.state, self.state.buf.device
        H = _packed(H_packed, st.P, "H_packed")
        if H.device != dev:
            raise ValueError(f"the matrices must live on {dev}")
        max_iter = int(max_iter)
        if not 1 <= max_iter <= 10000:
            raise ValueError(f"max_iter={max_iter} outside 1..10000")
        orth = self._orthogonalizer(orthogonalizer)
        no = self._occupied(n_occ)
        self._orth, self._max_iter, self._n_occ = orth, max_iter, no
        self.ctl = torch.empty(st.B, 40 + max_iter, dtype=torch.float64, device=dev)
        self.log = torch.empty(st.B, max_iter, dtype=torch.int32, device=dev)
        if orth is None:
            self.state.call("nq_orb_pur_init", *_typed(H), None, _lib.ptr(no), max_iter, _lib.ptr(self.ctl), _lib.ptr(self.log))
        else:
            self.congruence(orth.Z, H, False, out=st.work)
            self.state.call("nq_orb_pur_init", None, 1, _lib.ptr(orth.Z), _lib.ptr(no), max_iter, _lib.ptr(self.ctl), _lib.ptr(self.log))
        return self

    def step(self, k: int) -> "BatchedPurification":
        """Exactly one iteration, number ``k`` (``nq_orb_pur_step``; for tests: call them in order from 0)."""
        self.state.call("nq_orb_pur_step", int(k), self._max_iter, _lib.ptr(self.ctl), _lib.ptr(self.log))
        return self

    def purify(self, H_packed: torch.Tensor, n_occ, max_iter: int = 100, orthogonalizer: Optional[Orthogonalizer] = None) -> "BatchedPurification":
        self.prepare(H_packed, n_occ, max_iter, orthogonalizer)
        self.state.call("nq_orb_pur_run", self._max_iter, _lib.ptr(self.ctl), _lib.ptr(self.log))
        return self

    def _purified(self):
        if self._max_iter is None:
            raise RuntimeError("BatchedPurification: purify() first")

    def density(self) -> torch.Tensor:
        self._purified()
        return self.congruence(None if self._orth is None else self._orth.Z, self.state.coeff, True, 2.0)

    def response_start(self, G: torch.Tensor):
        """``Gt = 2 Z (G + G^T) / 2 Z^T`` and the start of the recursion (``nq_orb_pur_response_init``) -> ``(Gt, X1, Q)``; ``response_step(k, X1, Q)`` is one
        iteration (for tests)."""
        self._purified()
        P = self.state.P
        Gt = self.congruence(None if self._orth is None else self._orth.Z, self._f64(G, P, "G"), False, 2.0, symmetrize=True)
        X1, Q = self._scratch(P), self._scratch(P)
        self.state.call("nq_orb_pur_response_init", _lib.ptr(Gt), self._max_iter, _lib.ptr(self.ctl), _lib.ptr(X1))
        return Gt, X1, Q

    def response_step(self, k: int, X1: torch.Tensor, Q: torch.Tensor):
        self.state.call("nq_orb_pur_response_step", int(k), self._max_iter, _lib.ptr(self.log), _lib.ptr(Q), _lib.ptr(X1))

    def response(self, G: torch.Tensor, overlap: bool = True):
        Gt, X1, Q = self.response_start(G)
        self.state.call("nq_orb_pur_response_run", self._max_iter, _lib.ptr(self.log), _lib.ptr(Q), _lib.ptr(X1))
        st = self.state
        Z = None if self._orth is None else self._orth.Z
        gH = self.congruence(Z, X1, True)
        if not overlap or Z is None:
            return gH, None
        M2 = self.gemm(X1, self.gemm(st.coeff, st.work), alpha=2.0)                        # 2 g X Ht
        A = self.gemm(st.coeff, self.gemm(Gt, st.coeff), M2)                               # X Gt X + 2 M; its symmetric part is M + M^T + X Gt X
        return gH, self.congruence(Z, A, True, -1.0, symmetrize=True)

    def frontier(self, k_max: int = 256, tol: float = 2.0 ** -44, transform: Optional[torch.Tensor] = None) -> FrontierLevels:
        """HOMO, LUMO and the gap of the last ``purify`` (``nq_orb_front_lanczos``, one launch on the current stream, nothing is read back)."""
        self._purified()
        st, dev = self.state, self.state.buf.device
        k_max, tol = int(k_max), float(tol)
        if not 1 <= k_max <= 1024:
            raise ValueError(f"k_max={k_max} outside 1..1024")
        if not 0.0 < tol < 1.0:
            raise ValueError(f"tol={tol} outside (0, 1)")
        if transform is None:
            W = None if self._orth is None else self._orth.Z
        else:
            W = self._f64(transform, st.P, "transform")
        kk = np.minimum(st.m, k_max)
        vptr_host = np.concatenate([[0], np.cumsum(2 * kk * st.m)]).astype(np.int64)
        vptr = torch.from_numpy(vptr_host).to(dev)
        V = self._scratch(int(vptr_host[-1]))
        shift = self.ctl[:, :2].contiguous()
        eps = torch.empty(st.B, 2, dtype=torch.float64, device=dev)
        res = torch.empty(st.B, 2, dtype=torch.float64, device=dev)
        vec = torch.empty(2, st.M, dtype=torch.float64, device=dev)
        coef = torch.empty(2, st.M, dtype=torch.float64, device=dev)
        iters = torch.empty(st.B, 2, dtype=torch.int32, device=dev)
        conv = torch.empty(st.B, 2, dtype=torch.int32, device=dev)
        self.state.call("nq_orb_front_lanczos", _lib.ptr(st.work), _lib.ptr(st.coeff), _lib.ptr(shift), _lib.ptr(self._n_occ), _lib.ptr(W), k_max, tol, _lib.ptr(V),
                   _lib.ptr(vptr), _lib.ptr(eps), _lib.ptr(vec), _lib.ptr(coef), _lib.ptr(iters), _lib.ptr(res), _lib.ptr(conv))
        self._k_max = k_max
        return FrontierLevels(eps[:, 0], eps[:, 1], eps[:, 1] - eps[:, 0], coef, vec, iters, res, conv)

    def frontier_gradients(self, levels: FrontierLevels, g_homo: Optional[torch.Tensor], g_lumo: Optional[torch.Tensor], overlap: bool = True):
        """``(dL/dH, dL/dS or None)`` for the upstream gradients ``g_homo`` / ``g_lumo`` float64 [B] (None: zero) of ``levels.homo`` / ``levels.lumo``: ``sum g c c^T`` and
        ``-sum g eps c c^T`` (``nq_orb_front_gram``), packed float64 [P], exactly symmetric.  A level that does not exist contributes nothing."""
        st, dev = self.state, self.state.buf.device
        g = torch.zeros(st.B, 2, dtype=torch.float64, device=dev)
        for k, gk in enumerate((g_homo, g_lumo)):
            if gk is not None:
                g[:, k] = self._f64(gk, st.B, "g_homo" if k == 0 else "g_lumo")
        eps = torch.stack((levels.homo, levels.lumo), 1).contiguous()
        gH = self._scratch(st.P)
        gS = self._scratch(st.P, bool(overlap))
        self.state.call("nq_orb_front_gram", _lib.ptr(g), _lib.ptr(eps), _lib.ptr(self._f64(levels.coeff, 2 * st.M, "levels.coeff")), _lib.ptr(levels.converged),
                   _lib.ptr(gH), _lib.ptr(gS))
        return gH, gS

    def frontier_check(self, levels: FrontierLevels) -> "BatchedPurification":
        """Reads ``levels.converged`` once (a host synchronisation) and raises ``RuntimeError`` naming the first molecule and side that did not converge."""
        self.check()
        conv = levels.converged.cpu().numpy()
        bad = np.argwhere(conv == 0)
        if bad.size:
            b, side = int(bad[0][0]), int(bad[0][1])
            raise RuntimeError(f"molecule {b}: the {'LUMO' if side else 'HOMO'} did not converge in {int(levels.iterations[b, side])} Lanczos steps "
                               f"(k_max={getattr(self, '_k_max', None)}, m={int(self.state.m[b])})")
        return self

    def occupied(self, transform: Optional[torch.Tensor] = None) -> "OccupiedOrbitals":
        """ALL occupied levels and coefficients of the last ``purify`` WITHOUT a full solve (csrc/orbocc.hip) -> ``OccupiedOrbitals``: a pivoted Cholesky factor
        ``X = Q^T Q`` of the projector (``nq_orb_occ_factor``), ``Hs = Q Ht Q^T`` (``nq_orb_resp_project`` for ``Ht Q^T``, ``nq_orb_occ_reduce``), the standard
        problem of the ``n_occ x n_occ`` blocks (``nq_orb_solve`` on a reduced state) and ``C = V Q W`` with the solver's sign rule (``nq_orb_occ_back``), on the
        current stream; nothing is read back.  ``transform``: a packed float64 [P] back-transform ``W`` in place of the orthogonaliser of the last purify, as in
        ``frontier``."""
        self._purified()
        st = self.state
        if transform is None:
            W = None if self._orth is None else self._orth.Z
        else:
            W = self._f64(transform, st.P, "transform")
        return OccupiedOrbitals(self, W)

    def check(self) -> "BatchedPurification":
        st = self.state
        bad = st.first_failure()
        if bad:
            b, status = bad
            info = int(st.info[b])
            if status == 1 and self._orth is not None:
                info = int(self._orth.info[b])
            if status == 4:
                info = int(self._max_iter)
            raise RuntimeError(_failure_text(b, status, info, int(st.m[b])))
        return self


OCCUPIED_FIGURES = ("eps_mae_occ", "similarity", "similarity_min", "homo_abs_err")


class OccupiedOrbitals:
    """What ``BatchedPurification.occupied`` returns, all on the device: ``energies`` float64 [M] (ascending in the slots ``k < n_occ`` of each molecule, NaN in
    the others), ``coefficients`` packed float64 [P] (row k of a block = occupied orbital k, ``c^T S c = 1``, the solver's sign rule; NaN rows for ``k >= n_occ``),
    ``n_occ`` int32 [B], ``pivots`` int32 [M] (the Cholesky pivots, -1 for ``k >= n_occ``), ``min_pivot`` / ``defect`` float64 [B] (the smallest pivot, >= 1/m
    for an exact projector; the largest left-over diagonal entry) and ``status`` int32 [B]: 0, the purification's own 1 / 4, 5 where the projector is not a
    projector of rank ``n_occ`` (a pivot below 1/(2m), or a left-over diagonal entry above it), 2 where the QL iteration of the reduced block did not converge; a molecule with a non-zero status has
    NaN in its own slots only.  ``weighted_gram(w0, w1=None)`` -> ``sum_{k < n_occ} w[k] c_k c_k^T`` (one ``nq_orb_wgram`` launch); ``density()`` ->
    ``2 sum_{k < n_occ} c_k c_k^T``, the ``BatchedPurification.density()`` to rounding; ``compare(target, S_packed)`` -> float64 [4, B], the rows of
    ``OCCUPIED_FIGURES``: the occupied-energy MAE, the mean and the minimum of ``|c_k^T S c'_k|`` over the occupied k and ``|Delta HOMO|`` against another
    ``OccupiedOrbitals`` of the batch (the occupied rows of ``nq_orb_compare``, which never reads a virtual slot for them; NaN where ``n_occ = 0``);
    ``check()`` reads the status once (a host synchronisation) and raises naming the molecule.  Occupied levels only: no ``frontier``, no response chain, no
    smearing.  The inputs are detached (``nabladft_amd.orbital_loss.purified_occupied_energies`` is the differentiable call)."""

    def __init__(self, pur: "BatchedPurification", W: Optional[torch.Tensor]):
        ps, dev = pur.state, pur.state.buf.device
        no_host = self.n_occ_host = pur._n_occ_host
        self.n_occ = pur._n_occ
        self._max_iter, self._orth = pur._max_iter, pur._orth
        B, M, P = ps.B, ps.M, ps.P
        st = self.state = OrbitalState(ps.orb_ptr_host, dev)
        occ_host = np.concatenate([[0], np.cumsum(no_host * ps.m)]).astype(np.int64)
        rows = np.maximum(no_host, 1)
        red = self.reduced = OrbitalState(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), dev)
        self._layout = (self.n_occ, torch.from_numpy(occ_host).to(dev), int(occ_host[-1]))
        O = self._layout[2]
        f64, i32 = torch.float64, torch.int32
        self.pivots = torch.empty(M, dtype=i32, device=dev)
        self.min_pivot, self.defect = torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=f64, device=dev)
        self.status = torch.empty(B, dtype=i32, device=dev)
        ps.call("nq_orb_occ_factor", _lib.ptr(self.n_occ), _lib.ptr(st.coeff), _lib.ptr(self.pivots), _lib.ptr(self.min_pivot), _lib.ptr(self.defect),
                _lib.ptr(self.status))
        Gs, T = torch.empty(P, dtype=f64, device=dev), torch.empty(max(O, 1), dtype=f64, device=dev)
        st.call("nq_orb_resp_project", *_ptrs(self._layout[:2]), O, _lib.ptr(ps.work), _lib.ptr(Gs), _lib.ptr(T))
        Hs = torch.empty(red.P, dtype=f64, device=dev)
        st.call("nq_orb_occ_reduce", *_ptrs(self._layout[:2]), O, _lib.ptr(T), _lib.ptr(self.status), _lib.ptr(red.pack_ptr), red.P, _lib.ptr(Hs))
        red.solve(Hs)
        with torch.cuda.device(dev):
            # two states in front of the dimensions, like nq_orb_compare
            _lib.check(_lib.load().nq_orb_occ_back(_lib.ptr(st.buf), _lib.ptr(red.buf), *st._dims, red.M, red.P, *_ptrs(self._layout[:2]), O, _lib.ptr(W),
                                                   _lib.ptr(self.status), _lib.ptr(T), _lib.stream_ptr()))
        self._pur_header = ps.header_dev
        self._orbitals = BatchedOrbitals.__new__(BatchedOrbitals)
        self._orbitals.state = st

    energies = property(lambda self: self.state.eps)
    coefficients = property(lambda self: self.state.coeff)
    orb_ptr = property(lambda self: self.state.orb_ptr_host)
    pack_ptr = property(lambda self: self.state.pack_ptr_host)

    def weighted_gram(self, w0: torch.Tensor, w1: Optional[torch.Tensor] = None):
        return self._orbitals.weighted_gram(w0, w1, None, self.n_occ)

    def density(self) -> torch.Tensor:
        st = self.state
        return self.weighted_gram(torch.full((st.M,), 2.0, dtype=torch.float64, device=st.buf.device))

    def compare(self, target: "OccupiedOrbitals", S_packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not isinstance(target, OccupiedOrbitals):
            raise TypeError(f"compare: target must be an OccupiedOrbitals, not {type(target).__name__}")
        st, tt = self.state, target.state
        if st._dims != tt._dims or not np.array_equal(st.orb_ptr_host, tt.orb_ptr_host) or not np.array_equal(self.n_occ_host, target.n_occ_host):
            raise ValueError("the two solutions belong to different batches")
        S = None if S_packed is None else _packed(S_packed, st.P, "S_packed")
        out = torch.empty(len(FIGURES), st.B, dtype=torch.float64, device=st.buf.device)
        with torch.cuda.device(st.buf.device):
            _lib.check(_lib.load().nq_orb_compare(_lib.ptr(st.buf), _lib.ptr(tt.buf), *st._dims, *_typed(S), _lib.ptr(self.n_occ), _lib.ptr(out), _lib.stream_ptr()))
        return out[[FIGURES.index(k) for k in ("eps_mae_occ", "psi_sim_occ", "psi_sim_min_occ", "homo_abs_err")]]

    def check(self) -> "OccupiedOrbitals":
        st = self.state
        st.header()
        self.reduced.header()
        if int(self._pur_header[4]) == -3:
            raise RuntimeError("occupied(): the state does not hold a purification")
        status = self.status.cpu().numpy()
        bad = np.nonzero(status)[0]
        if bad.size:
            b, s = int(bad[0]), int(status[bad[0]])
            if s == 5:
                raise RuntimeError(f"molecule {b}: the purified matrix is not a projector of rank n_occ={int(self.n_occ_host[b])} (a Cholesky pivot below 1/(2m) or a left-over "
                                   f"diagonal entry above it, m={int(st.m[b])}; status 5)")
            info = int(self._max_iter) if s == 4 else (int(self._orth.info[b]) if s == 1 and self._orth is not None else 0)
            raise RuntimeError(_failure_text(b, s, info, int(st.m[b])))
        return self


class PurifiedOrbitalErrors:
    """The occupied-orbital figures of a test loop WITHOUT a full solve, accumulated over batches: the ``update(pred_packed, target_packed, overlap_packed,
    plan_or_orb_ptr, z, ptr)`` / ``compute()`` contract of ``OrbitalErrors``.  ``update`` sends both Hamiltonians through ONE orthogonaliser of the common overlap
    (``None``: the standard problem), two purifications and two ``occupied()`` calls and adds the four per-molecule figures of ``OCCUPIED_FIGURES``
    (``eps_mae_occ``, ``similarity``, ``similarity_min``, ``homo_abs_err``: the ``eps_mae_occ``, ``psi_sim_occ``, ``psi_sim_min_occ`` and ``homo_abs_err`` of
    ``FIGURES``) to running sums on the device; nothing is read back.  ``compute()`` first reads the status words kept of every batch and raises
    ``RuntimeError`` naming the batch, the side and the molecule for a failure in ANY batch since the last ``reset()`` (status 1: the overlap, 4: no gap, 5:
    not a projector, 2: the reduced QL iteration); otherwise -> dict of the means over all molecules seen.  ``max_iter`` caps the purification."""

    def __init__(self, charge=0, max_iter: int = 100):
        self.charge, self.max_iter = charge, int(max_iter)
        self.reset()

    def reset(self):
        self._sum = None
        self._count = None
        self._flags = []          # per update: int32 [2, B] on the device = (predicted, target) status, the overlap's pivots, and m

    def update(self, pred_packed, target_packed, overlap_packed, plan_or_orb_ptr, z, ptr):
        _require_gpu(pred_packed)
        op = _orb_ptr_of(plan_or_orb_ptr)
        n_occ = check_occupied(occupied_counts(z, ptr, self.charge), op)
        dev = pred_packed.device
        pur_p, pur_t = BatchedPurification(op, dev), BatchedPurification(op, dev)
        orth = None if overlap_packed is None else pur_p.orthogonalize(overlap_packed)
        occ_p = pur_p.purify(pred_packed, n_occ, self.max_iter, orth).occupied()
        occ_t = pur_t.purify(target_packed, n_occ, self.max_iter, orth).occupied()
        figs = occ_p.compare(occ_t, overlap_packed)
        ok = ~torch.isnan(figs)
        if self._sum is None:
            self._sum = torch.zeros(len(OCCUPIED_FIGURES), dtype=torch.float64, device=figs.device)
            self._count = torch.zeros(len(OCCUPIED_FIGURES), dtype=torch.float64, device=figs.device)
        self._sum += torch.where(ok, figs, torch.zeros_like(figs)).sum(1)
        self._count += ok.sum(1).to(torch.float64)
        info = torch.zeros_like(occ_p.status) if orth is None else orth.info
        self._flags.append((torch.stack([occ_p.status, occ_t.status, info]), occ_p.state.m))
        return self

    def compute(self) -> dict:
        if self._sum is None:
            raise RuntimeError("PurifiedOrbitalErrors.compute() before any update()")
        for i, (flags, m) in enumerate(self._flags):
            flags = flags.cpu().numpy()
            for side, name in enumerate(("predicted", "target")):
                bad = np.nonzero(flags[side])[0]
                if bad.size:
                    b, s = int(bad[0]), int(flags[side, bad[0]])
                    if s == 5:
                        raise RuntimeError(f"batch {i}, {name} Hamiltonian, molecule {b}: the purified matrix is not a projector of rank n_occ (status 5)")
                    raise RuntimeError(f"batch {i}, {name} Hamiltonian, " + _failure_text(b, s, self.max_iter if s == 4 else int(flags[2, b]), int(m[b])))
        mean = (self._sum / self._count).cpu().tolist()
        return dict(zip(OCCUPIED_FIGURES, mean))


class OrbitalErrors:
    """The orbital figures of a test loop, accumulated over batches: for QHNet ``update(net(batch, packed=True), asm.pack_targets(plan, batch.hamiltonian),
    asm.pack_targets(plan, batch.overlap), plan, batch.z, batch.ptr)``; for PhiSNet the ``*_packed`` results and targets with ``results["plan"]``.

    ``update`` solves the predicted and the target Hamiltonian under the common overlap (``None``: the identity) and adds the seven per-molecule figures of
    ``FIGURES`` to running sums on the device; nothing is read back.  It also keeps, on the device, the status words of both solves of every batch (a few
    integers per molecule; the solver states themselves are released).  ``compute()`` reads them first and raises ``RuntimeError`` naming the batch (in
    the order of the ``update`` calls), the molecule and, for an overlap that is not positive definite, the Cholesky pivot -- for a failure in ANY batch
    since the last ``reset()``, so a mean is never taken over a silent subset.  Otherwise -> dict of the means over all molecules seen (one host read).
    ``lumo_abs_err`` / ``gap_abs_err`` average over the molecules that have a virtual orbital.  No gradient flows through."""

    def __init__(self, charge=0):
        self.charge = charge
        self.reset()

    def reset(self):
        self._sum = None
        self._count = None
        self._flags = []          # per update: int32 [2, 2, B] on the device = (predicted, target) x (status, info), and the two header status words

    def update(self, pred_packed, target_packed, overlap_packed, plan_or_orb_ptr, z, ptr):
        _require_gpu(pred_packed)
        op = _orb_ptr_of(plan_or_orb_ptr)
        n_occ = check_occupied(occupied_counts(z, ptr, self.charge), op)
        pred = BatchedOrbitals(op, pred_packed.device).solve(pred_packed, overlap_packed)
        targ = BatchedOrbitals(op, pred_packed.device).solve(target_packed, overlap_packed)
        figs = pred.compare(targ, n_occ, overlap_packed)
        ok = ~torch.isnan(figs)
        if self._sum is None:
            self._sum = torch.zeros(len(FIGURES), dtype=torch.float64, device=figs.device)
            self._count = torch.zeros(len(FIGURES), dtype=torch.float64, device=figs.device)
        self._sum += torch.where(ok, figs, torch.zeros_like(figs)).sum(1)
        self._count += ok.sum(1).to(torch.float64)
        flags = torch.stack([torch.stack([o.state.status, o.state.info]) for o in (pred, targ)])       # copies: the states go away with this call
        self._flags.append((flags, torch.stack([pred.state.header_dev[4], targ.state.header_dev[4]]), pred.state.m))
        return self

    def compute(self) -> dict:
        if self._sum is None:
            raise RuntimeError("OrbitalErrors.compute() before any update()")
        for i, (flags, hdr, m) in enumerate(self._flags):
            flags, hdr = flags.cpu().numpy(), hdr.cpu().tolist()
            for side, name in enumerate(("predicted", "target")):
                if hdr[side] == -2:
                    raise RuntimeError(f"batch {i}, {name} Hamiltonian: an nq_orb call came with other dimensions than nq_orb_init prepared the state for")
                bad = np.nonzero(flags[side, 0])[0]
                if bad.size:
                    b = int(bad[0])
                    raise RuntimeError(f"batch {i}, {name} Hamiltonian, " + _failure_text(b, int(flags[side, 0, b]), int(flags[side, 1, b]), int(m[b])))
        mean = (self._sum / self._count).cpu().tolist()
        return dict(zip(FIGURES, mean))


class ScfResidualErrors:
    """The SCF residual of a test loop, accumulated over batches: ``update(pred_packed, target)`` with ``target`` an ``ScfTarget`` (``(basis, DL)``: the
    ``LowdinBasis`` of the conformers and the target's Löwdin density, ``nabladft_amd.orbital_loss.scf_target``) forms ``R^L = [S^(-1/2) H S^(-1/2), D^L]`` of
    the predicted ``H`` -- three product launches, nothing is solved -- and adds the per-molecule root mean square ``sqrt(sum R_ij^2 / m^2)`` and maximum
    ``max |R_ij|`` (the DIIS error) from ``commutator_norms`` to running sums on the device; nothing is read back.  A molecule whose figures are not finite
    (an overlap that is not positive definite, a failed decomposition, NaN in the prediction) is counted and left out of the means.  ``compute()`` -> dict
    ``scf_residual_rms``, ``scf_residual_max`` (means over the molecules kept), ``molecules`` and ``failed`` (one host read); it raises ``RuntimeError`` before
    any ``update()``.  No gradient flows through."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._sum = None          # float64 [4] on the device: sum of rms, sum of max, molecules kept, molecules left out

    def update(self, pred_packed: torch.Tensor, target):
        basis, DL = target
        if not isinstance(basis, LowdinBasis):
            raise TypeError(f"ScfResidualErrors.update: target must be an ScfTarget (basis, DL), its basis a LowdinBasis, not {type(basis).__name__}")
        _require_gpu(pred_packed)
        orb = basis.orbitals
        P = orb.state.P
        HL = orb.sym_congruence(basis.inv_half.detach(), _packed(pred_packed, P, "pred_packed"))[0]
        sumsq, top = orb.commutator_norms(orb.commutator(HL, DL.detach()))
        m = torch.from_numpy(orb.state.m.astype(np.float64)).to(sumsq.device)
        rms = torch.sqrt(sumsq) / m
        ok = torch.isfinite(rms) & torch.isfinite(top)
        zero = torch.zeros_like(rms)
        okf = ok.to(torch.float64)
        add = torch.stack([torch.where(ok, rms, zero).sum(), torch.where(ok, top, zero).sum(), okf.sum(), (1.0 - okf).sum()])
        self._sum = add if self._sum is None else self._sum + add
        return self

    def compute(self) -> dict:
        if self._sum is None:
            raise RuntimeError("ScfResidualErrors.compute() before any update()")
        s_rms, s_max, kept, failed = self._sum.cpu().tolist()
        nan = float("nan")
        return {"scf_residual_rms": s_rms / kept if kept else nan, "scf_residual_max": s_max / kept if kept else nan, "molecules": int(kept), "failed": int(failed)}


def mulliken_charges(z, atom_pop: torch.Tensor) -> torch.Tensor:
    """Mulliken charges ``q_A = Z_A - pop_A`` (float64 [N], on the device of ``atom_pop``) from the populations of ``BatchedOrbitals.populations``."""
    zz = z if isinstance(z, torch.Tensor) else torch.as_tensor(np.asarray(z))
    if zz.numel() != atom_pop.numel():
        raise ValueError(f"z has {zz.numel()} atoms, atom_pop {atom_pop.numel()}")
    return zz.to(device=atom_pop.device, dtype=torch.float64).reshape(-1) - atom_pop.to(torch.float64)


__all__ = ["BatchedOrbitals", "BatchedPurification", "Orthogonalizer", "FrontierLevels", "LowdinBasis", "BatchedMatrixRoot", "OrbitalState", "OrbitalErrors", "ScfResidualErrors", "FermiResult", "occupied_counts", "electron_counts", "check_occupied", "mulliken_charges", "bond_layout", "dense_bond_orders", "MAX_ORBITALS", "MAX_ATOM_ORBITALS", "FIGURES", "OccupiedOrbitals", "PurifiedOrbitalErrors", "OCCUPIED_FIGURES"]
