"""TEST INFRASTRUCTURE -- plain-loop, differentiable torch restatement of the PhiSNet irreps -> matrix assembly exactly as the header of
csrc/hblock.hip states it, the packed <-> dense helpers, and the batches of tests/test_hamiltonian_ops_gpu.py.  Pinned to the reference project by
tests/test_hamiltonian_ops_ref_cpu.py through tests/golden/phisnet_matrix.npz.  The QHNet side needs no new restatement: oracle/hblock_ref.build_final_matrix
is dtype-generic and differentiable already.

    block(i, j)[(n_i, m_i), (n_j, m_j)] = sum_L sqrt(2L+1) sum_M CG(l_i m_i, l_j m_j | L M) * f[row(i, j)][L^2 + M][idx(z_i, z_j, n_i, n_j, L)]

rows = the orbitals of atom idx_i, columns = those of atom idx_j, f = f_ii[atom] (i == j, idx from irreps_ii) or f_ij[pair row] (idx from irreps_ij); then the
transpose is added (symmetrize), then the diagonal is set to 1 (unit_diagonal).  Everything is evaluated in the dtype of f_ii."""
import numpy as np
import torch

from oracle import hblock_ref as HB


# ---- layout helpers ------------------------------------------------------------------------------------------------------------------------------------
def mol_orbitals(z, ptr, norb):
    """Orbitals per molecule; ``norb``: {Z: orbitals of one atom}."""
    n = [norb[int(a)] for a in z]
    return [sum(n[int(ptr[b]):int(ptr[b + 1])]) for b in range(len(ptr) - 1)]


def pack(dense, morb):
    """Dense block-diagonal [M, M] -> the diagonal blocks, molecule after molecule, row-major."""
    o, parts = 0, []
    for m in morb:
        parts.append(dense[o:o + m, o:o + m].reshape(-1))
        o += m
    return torch.cat(parts) if parts else dense.new_zeros(0)


def unpack(packed, morb, fill=0.0):
    """The inverse of ``pack``; everything off the blocks holds ``fill``."""
    M = sum(morb)
    dense = torch.full((M, M), fill, dtype=packed.dtype)
    o = q = 0
    for m in morb:
        dense[o:o + m, o:o + m] = packed[q:q + m * m].view(m, m)
        o, q = o + m, q + m * m
    return dense


# ---- the PhiSNet assembly -------------------------------------------------------------------------------------------------------------------------------
def shell_offsets(shells):
    off, o = [], 0
    for _, l in shells:
        off.append(o)
        o += 2 * l + 1
    return off, o


def irreps_blocks(z, ptr, idx_i, idx_j, atom2orbitals, irreps_ii, irreps_ij, cg, f_ii, f_ij, skip_missing=False):
    """List of the molecules' matrices before symmetrisation.  A key missing from the dictionaries raises KeyError as the reference does, or, with
    ``skip_missing``, leaves that L term out (what the kernel does while it sets bit 4 of the error word)."""
    dtype = f_ii.dtype
    row = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(idx_i, idx_j))}
    scaled = {}

    def cgs(li, lj, L):
        if (li, lj, L) not in scaled:
            scaled[(li, lj, L)] = torch.as_tensor(cg(li, lj, L)).to(dtype) * torch.tensor(2 * L + 1, dtype=dtype).sqrt()
        return scaled[(li, lj, L)]
    mats = []
    for b in range(len(ptr) - 1):
        atoms = range(int(ptr[b]), int(ptr[b + 1]))
        rows = []
        for i in atoms:
            zi = int(z[i])
            blocks = []
            for j in atoms:
                zj = int(z[j])
                f, table = (f_ii[i], irreps_ii) if i == j else (f_ij[row[(i, j)]], irreps_ij)
                shell_rows = []
                for ni, (_, li) in enumerate(atom2orbitals[zi]):
                    shell_cols = []
                    for nj, (_, lj) in enumerate(atom2orbitals[zj]):
                        blk = torch.zeros(2 * li + 1, 2 * lj + 1, dtype=dtype)
                        for L in range(abs(li - lj), li + lj + 1):
                            key = (zi, zj, ni, nj, L)
                            if key not in table:
                                if skip_missing:
                                    continue
                                raise KeyError(key)
                            blk = blk + torch.einsum("abm,m->ab", cgs(li, lj, L), f[L * L:(L + 1) * (L + 1), table[key]])
                        shell_cols.append(blk)
                    shell_rows.append(torch.cat(shell_cols, dim=1))
                blocks.append(torch.cat(shell_rows, dim=0))
            rows.append(torch.cat(blocks, dim=1))
        mats.append(torch.cat(rows, dim=0))
    return mats


def finish(mats, symmetrize, unit_diagonal):
    """Packed result of the blocks of ``irreps_blocks``: + transpose, then diagonal = 1."""
    out = []
    for H in mats:
        if symmetrize:
            H = H + H.T
        if unit_diagonal:
            eye = torch.eye(H.shape[0], dtype=H.dtype)
            H = H * (1 - eye) + eye
        out.append(H.reshape(-1))
    return torch.cat(out)


def irreps_matrix(z, ptr, idx_i, idx_j, atom2orbitals, irreps_ii, irreps_ij, cg, f_ii, f_ij, symmetrize, unit_diagonal, skip_missing=False):
    return finish(irreps_blocks(z, ptr, idx_i, idx_j, atom2orbitals, irreps_ii, irreps_ij, cg, f_ii, f_ij, skip_missing), symmetrize, unit_diagonal)


def irreps_dictionaries(atom2orbitals, compute_matrix_irreps):
    """(irreps_ii, irreps_ij) over all elements / ordered element pairs, ascending Z, as the model builds them."""
    number_L, irreps_ii = [0] * 5, {}
    for zz in sorted(atom2orbitals):
        irreps_ii, number_L = compute_matrix_irreps(atom2orbitals[zz], atom2orbitals[zz], irreps_ii, number_L)
    number_L, irreps_ij = [0] * 5, {}
    for za in sorted(atom2orbitals):
        for zb in sorted(atom2orbitals):
            irreps_ij, number_L = compute_matrix_irreps(atom2orbitals[za], atom2orbitals[zb], irreps_ij, number_L)
    return irreps_ii, irreps_ij


def columns_per_L(table):
    """[5] number of feature columns the dictionary uses of each order L (1 + its largest index of that L)."""
    n = [0] * 5
    for (_, _, _, _, L), v in table.items():
        n[L] = max(n[L], int(v) + 1)
    return n


# ---- the batches ----------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """z [N], ptr [B+1], pairs [2, P] (QHNet: row 0 = dst, row 1 = src; PhiSNet: row 0 = idx_i, row 1 = idx_j), perm: None or the permutation that
    turned the pair list of ``base`` into this one (pairs = base.pairs[:, perm])."""

    def __init__(self, mols, perm_seed=None, phisnet=False):
        self.mols = mols
        self.z = torch.tensor([a for m in mols for a in m], dtype=torch.long)
        self.ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(m) for m in mols])]), dtype=torch.long)
        fg = HB.full_graph(self.ptr)                      # [2, 0] for a batch without pairs
        self.pairs = fg.flip(0) if phisnet else fg        # PhiSNet lists (centre i, other atom j): i ascending, then j ascending
        self.perm = None
        if perm_seed is not None:
            self.perm = torch.randperm(self.pairs.shape[1], generator=torch.Generator().manual_seed(perm_seed))
            self.pairs = self.pairs[:, self.perm]
        self.N, self.B, self.P = int(self.z.numel()), len(mols), int(self.pairs.shape[1])


BR, H, C, N_, O, F, S, CL = 35, 1, 6, 7, 8, 9, 16, 17
QH_EDGES = [[BR], [H], [H, H], [O, H, H], [C, N_, F, S, CL, BR, H]]


def qh_cases():
    return {"edges": Case(QH_EDGES), "one": Case(QH_EDGES[-1:]), "atoms only": Case([[BR], [H], [C]]), "permuted": Case(QH_EDGES, perm_seed=7)}


IR_ORBITALS = {1: ((1, 0), (1, 0), (1, 1)),
               6: ((6, 0), (6, 0), (6, 0), (6, 1), (6, 1), (6, 2)),
               8: ((8, 0), (8, 0), (8, 0), (8, 1), (8, 1), (8, 2)),
               16: ((16, 0), (16, 0), (16, 0), (16, 0), (16, 1), (16, 1), (16, 1), (16, 2), (16, 2))}
IR_MOLS = [[S], [H, H], [O, H, C, S]]
IR_S_ONLY = {1: ((1, 0), (1, 0))}


def ir_cases():
    return {"batch": Case(IR_MOLS, phisnet=True), "one": Case(IR_MOLS[-1:], phisnet=True), "permuted": Case(IR_MOLS, perm_seed=11, phisnet=True),
            "s only": Case([[H], [H, H], [H, H, H]], phisnet=True)}
