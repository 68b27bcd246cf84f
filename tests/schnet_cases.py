"""TEST INFRASTRUCTURE -- the edge cases of the SchNet engine (csrc/schnet.hip), shared by tests/test_schnet_cases_cpu.py (which asserts that every
case still has the property it exists for) and tests/test_schnet_ops_gpu.py (which runs the engine on them).  Plain module, no GPU, no pytest.

Each case is the smallest shape at which one path of the engine runs:
  long_rows    rows and lower-neighbour lists longer than one wavefront: the second 64-wide chunk of k_sn_conv / k_sn_pair_rev
  small_r      n_rbf on both sides of the 13-tap window (FWIN): the zero-padded LDS copy of W1^T, nwin = R
  lds_limit    W1^T fills the 156 KB of LDS exactly (R = 156 at F = 256)
  sort_limit   the k0 sort at its 256 bins (R = 268)
  one_pair     one dimer alone: N = 2, E = 2, P = 1
  elements     z = max_z - 1 present, several elements absent (embedding-gradient rows nobody writes)
  near_cutoff  a pair a hair inside the cutoff: in the list, fcut ~ 0
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from oracle import spk_schnet_ref as S
from oracle.spk_painn_ref import full_neighbor_list

FWIN = 13                       # taps of the window record (csrc/common.h)
LDS_BYTES = 156 * 1024          # what sn_check grants W1^T
SORT_BINS = 256                 # bins of nq_k0_sort


@dataclass
class Case:
    name: str
    cfg: S.SchNetConfig
    pos: torch.Tensor           # float32 [N][3]
    z: torch.Tensor             # int64 [N]
    batch: torch.Tensor         # int64 [N]
    y: torch.Tensor             # float32 [B]
    ft: torch.Tensor            # float32 [N][3]
    param_seed: int

    @property
    def sizes(self):
        return torch.bincount(self.batch).tolist()


def box_molecule(rng, n):
    """n atoms uniform in a box of side 1.9 n^(1/3) + 1 (the recipe of test_dense_molecules_long_rows); a dimer is placed at a fixed bond length so
    that it always has its pair."""
    if n == 2:
        o = rng.uniform(0, 1.0, size=(1, 3))
        return np.concatenate([o, o + np.array([[0.9, 0.5, -0.4]])])
    return rng.uniform(0, (n ** (1 / 3)) * 1.9 + 1.0, size=(n, 3))


def _assemble(name, cfg, mols, z, rng, param_seed):
    pos = np.concatenate(mols).astype(np.float32)
    batch = np.concatenate([np.full(len(m), i) for i, m in enumerate(mols)]).astype(np.int64)
    y = rng.normal(size=len(mols)).astype(np.float32)
    ft = rng.normal(0, 0.05, size=pos.shape).astype(np.float32)
    return Case(name, cfg, torch.tensor(pos), torch.tensor(np.asarray(z, dtype=np.int64)), torch.tensor(batch), torch.tensor(y), torch.tensor(ft), param_seed)


def _boxes(name, F, L, R, cutoff, sizes, seed, elements=(1, 6, 7, 8), max_z=20, param_seed=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    mols = [box_molecule(rng, n) for n in sizes]
    z = rng.choice(list(elements), size=sum(sizes))
    cfg = S.SchNetConfig(n_atom_basis=F, n_interactions=L, n_rbf=R, cutoff=cutoff, max_z=max_z)
    return _assemble(name, cfg, mols, z, rng, F + L + R if param_seed is None else param_seed)


LONG_ROWS_SIZES = [200, 2, 70]
SMALL_R = (2, 12, 13, 14)
NEAR_CUTOFF_GAP = 2.0 ** -20


def _near_cutoff():
    """[9-atom box, a dimer at d = cutoff (1 - 2^-20) along x (exactly representable in float32: the pair is inside the cutoff in both precisions),
    5-atom box]"""
    rng = np.random.Generator(np.random.PCG64(5))
    cutoff = 4.0
    d = np.float32(cutoff * (1.0 - NEAR_CUTOFF_GAP))
    assert float(d) == cutoff * (1.0 - NEAR_CUTOFF_GAP)
    mols = [box_molecule(rng, 9), np.array([[0.0, 0.0, 0.0], [float(d), 0.0, 0.0]]), box_molecule(rng, 5)]
    z = rng.choice([1, 6, 7, 8], size=16)
    return _assemble("near_cutoff", S.SchNetConfig(n_atom_basis=64, n_interactions=1, n_rbf=20, cutoff=cutoff, max_z=20), mols, z, rng, 85)


def _elements():
    rng = np.random.Generator(np.random.PCG64(19))
    sizes = [17, 1, 12]
    mols = [box_molecule(rng, n) for n in sizes]
    z = rng.choice([1, 6, 8, 19], size=sum(sizes))
    z[:4] = [19, 1, 6, 8]                                    # every listed element is present whatever the draw
    return _assemble("elements", S.SchNetConfig(n_atom_basis=64, n_interactions=1, n_rbf=20, cutoff=4.0, max_z=20), mols, z, rng, 86)


_BUILDERS = {
    "long_rows-F64": lambda: _boxes("long_rows-F64", 64, 2, 20, 6.0, LONG_ROWS_SIZES, 77, elements=(1, 6, 7, 8, 19)),
    "long_rows-F128": lambda: _boxes("long_rows-F128", 128, 1, 20, 6.0, LONG_ROWS_SIZES, 77, elements=(1, 6, 7, 8, 19)),
    "long_rows-F256": lambda: _boxes("long_rows-F256", 256, 1, 20, 6.0, LONG_ROWS_SIZES, 77, elements=(1, 6, 7, 8, 19)),
    **{f"small_r-R{R}": (lambda R=R: _boxes(f"small_r-R{R}", 64, 2, R, 4.0, [12, 1, 2, 30], 31)) for R in SMALL_R},
    "lds_limit": lambda: _boxes("lds_limit", 256, 1, 156, 5.0, [140, 1, 2, 9], 32),
    "sort_limit": lambda: _boxes("sort_limit", 64, 1, 268, 5.0, [40, 1, 2, 9], 33),
    "one_pair": lambda: _boxes("one_pair", 64, 2, 20, 4.0, [2], 34),
    "elements": _elements,
    "near_cutoff": _near_cutoff,
}
CASE_NAMES = list(_BUILDERS)
LONG_ROWS = [n for n in CASE_NAMES if n.startswith("long_rows")]
SMALL_R_CASES = [n for n in CASE_NAMES if n.startswith("small_r")]


@functools.lru_cache(maxsize=None)
def get_case(name) -> Case:
    return _BUILDERS[name]()


def sub_case(case: Case, mol: int) -> Case:
    """Molecule `mol` of a case alone in its batch (same parameters)."""
    keep = case.batch == mol
    return Case(f"{case.name}[mol {mol}]", case.cfg, case.pos[keep], case.z[keep], torch.zeros(int(keep.sum()), dtype=torch.long), case.y[mol:mol + 1],
                case.ft[keep], case.param_seed)


def neighbor_list(case: Case):
    """(idx_i, idx_j) of the float64 restatement: every ordered pair with d < cutoff."""
    return full_neighbor_list(case.pos.double(), case.batch, case.cfg.cutoff)


def row_stats(case: Case):
    """degree [N] and number of lower neighbours (j < i) [N] of every atom."""
    ii, jj = neighbor_list(case)
    N = case.pos.shape[0]
    return torch.bincount(ii, minlength=N), torch.bincount(ii[jj < ii], minlength=N)


class Reference:
    """One training step of the restatement's four sweeps (SchNetSweeps.train_step) on a case, every buffer kept in .sw.S."""

    def __init__(self, case: Case, dtype, w_e=1.0, w_f=1.0):
        self.P = {k: v.to(dtype) for k, v in S.make_schnet_params(case.cfg, case.param_seed).items()}
        self.ii, self.jj = neighbor_list(case)
        self.sw = S.SchNetSweeps(self.P, case.cfg, case.pos.to(dtype), case.z, case.batch, self.ii, self.jj)
        self.energy, self.forces, self.loss, self.G = self.sw.train_step(case.y.to(dtype), case.ft.to(dtype), w_e, w_f)
        self.key = {(int(i), int(j)): e for e, (i, j) in enumerate(zip(self.ii.tolist(), self.jj.tolist()))}


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64, w_e=1.0, w_f=1.0) -> Reference:
    """Computed once per (case, precision, loss weights) and shared; callers leave it unchanged."""
    return Reference(get_case(name), dtype, w_e, w_f)
