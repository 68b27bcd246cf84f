"""CPU: pins the float64 restatement of the PhiSNet irreps -> matrix assembly (tests/hamiltonian_ops_ref.py), against which test_hamiltonian_ops_gpu.py
measures the kernels, to the reference project through tests/golden/phisnet_matrix.npz (written by the REAL compute_matrix_irreps / matrix_block /
generate_matrix_from_irreps, oracle/make_golden_phisnet.py --matrix); checks the batches that module runs; and checks that the shape contract of
BlockAssembler.assemble / IrrepsAssembler.assemble is refused in Python, before anything is loaded or launched.

The bound of the pin, 1e-6 array-max-relative, is the fixture's float32 storage: the restatement evaluated in float64 lands at about 1e-7 on all five arrays."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import hamiltonian_ops_ref as R
from tests.helpers import GOLDEN, rel_err
from tests.so3_helpers import FixtureCG
from tests.test_hblock_cpu import ORBITALS

F64 = torch.float64
PIN = 1e-6


@pytest.fixture(scope="module")
def pinned():
    fx = dict(np.load(os.path.join(GOLDEN, "phisnet_matrix.npz")))
    atom2orb = {k: v for k, v in R.IR_ORBITALS.items() if k in (1, 6, 8)}
    irreps_ii = {tuple(int(v) for v in k): int(x) for k, x in zip(fx["ii_keys"], fx["ii_vals"])}
    irreps_ij = {tuple(int(v) for v in k): int(x) for k, x in zip(fx["ij_keys"], fx["ij_vals"])}
    f_ii = torch.tensor(fx["f_ii"]).to(F64).requires_grad_(True)
    f_ij = torch.tensor(fx["f_ij"]).to(F64).requires_grad_(True)
    z, ptr = torch.tensor(fx["z"]), torch.tensor(fx["ptr"])
    mats = R.irreps_blocks(z, ptr, fx["idx_i"], fx["idx_j"], atom2orb, irreps_ii, irreps_ij, FixtureCG(), f_ii, f_ij)
    morb = R.mol_orbitals(z, ptr, {zz: R.shell_offsets(s)[1] for zz, s in atom2orb.items()})
    return fx, mats, morb, f_ii, f_ij


@pytest.mark.parametrize("name,symmetrize,unit_diagonal", [("H_unsym", False, False), ("H", True, False), ("overlap", True, True)])
def test_restatement_matches_reference_matrices(pinned, name, symmetrize, unit_diagonal):
    fx, mats, morb, _, _ = pinned
    got = R.unpack(R.finish(mats, symmetrize, unit_diagonal).detach(), morb)
    err = rel_err(got.numpy(), fx[name])
    print(f"MEASURED restatement float64 vs reference {name}: {err:.2e}")
    assert err < PIN, (name, err)


def test_restatement_matches_reference_gradients(pinned):
    fx, mats, morb, f_ii, f_ij = pinned
    w = R.pack(torch.tensor(fx["w"]).to(F64), morb)              # the reference's dense weights also cover the zero off-molecule region
    g_ii, g_ij = torch.autograd.grad(R.finish(mats, True, False), [f_ii, f_ij], w, retain_graph=True)
    for name, got in (("g_ii", g_ii), ("g_ij", g_ij)):
        err = rel_err(got.numpy(), fx[name])
        print(f"MEASURED restatement float64 vs reference {name}: {err:.2e}")
        assert err < PIN, (name, err)


def test_pack_and_unpack_are_inverse():
    morb = [3, 1, 4]
    p = torch.arange(26, dtype=torch.float32) + 1
    d = R.unpack(p, morb, fill=float("nan"))
    assert d.shape == (8, 8) and int(torch.isnan(d).sum()) == 64 - 26 and torch.equal(R.pack(d, morb), p)
    assert d[3, 3] == 10 and d[4, 4] == 11 and d[7, 7] == 26 and d[0, 2] == 3


def ordered_pairs(case):
    return sorted((int(a), int(b)) for a, b in zip(case.pairs[0], case.pairs[1]))


@pytest.mark.parametrize("cases", [R.qh_cases, R.ir_cases], ids=["qhnet", "phisnet"])
def test_case_generator(cases):
    cases = cases()
    for name, c in cases.items():
        want = sorted((i, j) for b in range(c.B) for i in range(int(c.ptr[b]), int(c.ptr[b + 1])) for j in range(int(c.ptr[b]), int(c.ptr[b + 1])) if i != j)
        assert ordered_pairs(c) == want, name                                          # every ordered pair of every molecule exactly once
        assert c.pairs.shape == (2, c.P) and c.pairs.dtype == torch.long and c.N == int(c.ptr[-1]) and max(len(m) for m in c.mols) <= 7
        if c.perm is not None:
            assert sorted(c.perm.tolist()) == list(range(c.P)) and c.perm.tolist() != list(range(c.P)), name
    for name, c in cases.items():
        if c.perm is not None:
            base = next(b for b in cases.values() if b.perm is None and b.mols == c.mols)
            assert torch.equal(c.pairs, base.pairs[:, c.perm]) and not torch.equal(c.pairs, base.pairs)
    assert any(c.perm is not None for c in cases.values()) and any(c.B == 1 and c.P > 0 for c in cases.values())


def test_case_generator_edges():
    qh, ir = R.qh_cases(), R.ir_cases()
    assert qh["atoms only"].P == 0 and qh["atoms only"].pairs.shape == (2, 0) and qh["atoms only"].N == 3
    assert qh["edges"].mols[0] == [35] and len(ORBITALS[35]) == 12                     # the lone Br atom: the full 32-slot mask
    assert qh["one"].B == 1 and qh["one"].mols == qh["edges"].mols[-1:]
    assert set(qh["edges"].z.tolist()) <= set(ORBITALS)
    assert ir["batch"].mols[0] == [16] and ir["one"].B == 1 and set(ir["batch"].z.tolist()) == set(R.IR_ORBITALS)
    assert sum(1 for _, l in R.IR_ORBITALS[16] if l == 2) == 2                         # one element with two d shells
    # the PhiSNet order is that of the fixture: centre atom ascending, the others ascending
    assert ir["batch"].pairs[:, :4].tolist() == [[1, 2, 3, 3], [2, 1, 4, 5]]
    assert qh["edges"].pairs[:, :4].tolist() == [[3, 2, 5, 6], [2, 3, 4, 4]]            # radius-graph order: src (row 1) ascending


# ---- the shape contract is enforced in Python ------------------------------------------------------------------------------------------------------------
def irreps_assembler():
    from nabladft_amd import hamiltonian as HM
    ii, ij = R.irreps_dictionaries(R.IR_ORBITALS, HM.compute_matrix_irreps)
    return HM.IrrepsAssembler(R.IR_ORBITALS, ii, ij, FixtureCG()), ii, ij


def test_irreps_assembler_knows_what_it_reads():
    asm, ii, ij = irreps_assembler()
    assert asm.max_index == max(max(ii.values()), max(ij.values())) and asm.max_L == 4
    from nabladft_amd import hamiltonian as HM
    s_ii, s_ij = R.irreps_dictionaries(R.IR_S_ONLY, HM.compute_matrix_irreps)
    s = HM.IrrepsAssembler(R.IR_S_ONLY, s_ii, s_ij, FixtureCG())
    assert s.max_L == 0 and s.max_index == 3


def test_irreps_assemble_refuses_mismatched_features():
    """Every refusal comes before the autograd function, which is the first thing that loads the library or touches a device pointer: host tensors and
    a stub plan are enough to reach each of them."""
    asm, _, _ = irreps_assembler()
    plan = SimpleNamespace(N=3, P=6)
    Fo = asm.max_index + 1
    ok_ii, ok_ij = torch.zeros(3, 25, Fo), torch.zeros(6, 25, Fo)
    for f_ii, f_ij, words in [(torch.zeros(2, 25, Fo), ok_ij, "2 rows"), (ok_ii, torch.zeros(5, 25, Fo), "5 rows"),
                              (ok_ii, torch.zeros(6, 25, Fo - 1), "share"),                                   # a too-narrow f_ij
                              (ok_ii, torch.zeros(6, 16, Fo), "share"),
                              (torch.zeros(3, 25, Fo - 1), torch.zeros(6, 25, Fo - 1), f"Fo = {Fo - 1}"),
                              (torch.zeros(3, 24, Fo), torch.zeros(6, 24, Fo), "ncomp = 24"),                 # a too-small ncomp
                              (torch.zeros(3, 25 * Fo), ok_ij, "[rows, ncomp, Fo]")]:
        with pytest.raises(ValueError, match=words.replace("[", r"\[").replace("]", r"\]")):
            asm.assemble(plan, f_ii, f_ij)


def test_block_assemble_refuses_mismatched_blocks():
    from nabladft_amd import hamiltonian as HM
    asm = HM.BlockAssembler(ORBITALS)
    plan = SimpleNamespace(N=3, P=6)
    ok_d, ok_n = torch.zeros(3, 32, 32), torch.zeros(6, 32, 32)
    for d, n in [(ok_d, torch.zeros(5, 32, 32)), (torch.zeros(2, 32, 32), ok_n), (torch.zeros(3, 32, 31), ok_n), (ok_d, torch.zeros(6, 32 * 32)),
                 (ok_d, torch.zeros(0, 32, 32))]:                                                            # a short nondiag
        with pytest.raises(ValueError, match="the plan needs"):
            asm.assemble(plan, d, n)
