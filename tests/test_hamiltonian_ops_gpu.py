"""The Hamiltonian assembly kernels (csrc/hblock.hip) one by one through the C ABI, called with the arguments hamiltonian.py passes, on the batches of
tests/hamiltonian_ops_ref.py: nq_hblock_tables, nq_hblock_assemble(_backward), nq_hblock_packed_dense against oracle/hblock_ref.build_final_matrix, and
nq_irreps_assemble(_backward) against the float64 restatement of tests/hamiltonian_ops_ref.py (pinned to the reference project by
test_hamiltonian_ops_ref_cpu.py); adjoints are torch.autograd.grad of the restatement.  Every output buffer starts as NaN and every call runs twice with
bitwise equal results.  The per-batch tables come from BlockAssembler.plan / IrrepsAssembler.plan and are compared exactly with a numpy construction.

Bounds.  The QHNet kernels move one input element or add two: every output is bitwise the float32 evaluation of the restatement.  The PhiSNet kernels
sum at most 25 fused multiply-adds per output: within max(3 x the error of the same restatement evaluated in float32 on the CPU, 2e-6) of the float64
value and below 1e-5, array-max-relative (helpers.assert_sum); zeros, ones and the permutation identities stay exact.  Measured on an MI355X (distance
from the float64 value: the kernel / the float32 CPU restatement on the same inputs; ranges over the cases and the four flag combinations):
    value        kernel 3.18e-8 .. 1.35e-7, restatement 3.18e-8 .. 1.35e-7
    grad f_ii    kernel 2.09e-8 .. 9.93e-8, restatement 2.09e-8 .. 9.93e-8
    grad f_ij    kernel 4.12e-8 .. 1.32e-7, restatement 4.12e-8 .. 1.32e-7
(the "s only" case without symmetrize is one product per element and exact on both sides); the kernel is never further than 1.15 x the restatement,
so the reference sits well inside the bound and the 2e-6 floor is what applies.

Branches and the tests that reach them:
  k_hb_orbmap (full 32-slot mask of Br, 5 slots of H), k_hb_lookup (radius-graph order and a permuted list, absent entries -1, P = 0), the memsets of
      nq_hblock_tables over poisoned buffers and a set error word: test_qh_tables, test_ir_tables
  hb_find_mol with B = 1, B = 3, B = 5 and molecule boundaries inside a workgroup; k_hb_assemble diagonal / pair blocks, symmetrize 0 / 1:
      test_qh_forward; the LOOK indirection under a permuted pair list: test_qh_forward[permuted-*]
  k_hb_assemble_rev symmetrize 0 / 1 from a non-symmetric seed (G[r, c] is not G[c, r]), exact zeros outside the two atoms' masks, P = 0 with NULL
      pair arguments, the permuted list: test_qh_backward; the same through BlockAssembler.assemble and autograd at P = 0: test_qh_atoms_only_autograd
  k_hb_scatter_dense both directions, zeros off the blocks, NaN off the blocks never read: test_qh_packed_dense
  error word 1 (pair joining two molecules, self pair), 2 (missing pair), 3 (both), a later plan reads 0: test_qh_error_word
  ir_elem diagonal / pair rows, every (l_i, l_j) of s, p, d with two d shells on one atom, symmetrize and unit_diagonal 0 / 1, NaN in every column the
      dictionaries do not use: test_ir_forward; k_ir_assemble_rev the same, code < 0 (unused columns: gradient exactly 0), the unit_diagonal continue:
      test_ir_backward, test_ir_unit_diagonal_seed; L >= IR_NL (ncomp = 36): test_ir_wide_ncomp; ncomp = 1: the "s only" case of the three
  error word 4 (fi < 0), KeyError from check, the L term left out: test_ir_missing_key; word 2 in ir_elem: test_ir_missing_pair
  the refusals of BlockAssembler.assemble / IrrepsAssembler.assemble (ValueError, error word untouched) and of the two backward entry points given P > 0
      and a NULL pair gradient (NQ_ERR_ARG, outputs untouched): test_qh_refusals, test_ir_refusals

No test here runs a backward kernel on a pair list that is not the full graph, and none launches with a shape that the contract excludes: k_hb_assemble_rev
and k_ir_assemble_rev index the packed gradient by the pair's atoms without a bounds check, which is exactly why the Python side refuses first."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from oracle import hblock_ref as HB  # noqa: E402
from tests import hamiltonian_ops_ref as R  # noqa: E402
from tests.helpers import DEV, P, _release_copies, assert_sum, bits, check, lib, nan_dev, rejected, rel, st, twice  # noqa: E402,F401  (_release_copies: autouse)
from tests.so3_helpers import FixtureCG  # noqa: E402
from tests.test_hblock_cpu import ORBITALS  # noqa: E402

F64, F32 = torch.float64, torch.float32
S = 32


def record(name, err, own):
    """One line per yardstick case on stdout (pytest -s): the numbers the module docstring quotes."""
    print(f"MEASURED {name}: kernel {err:.2e}, float32 CPU restatement {own:.2e}")


def HM():
    from nabladft_amd import hamiltonian
    return hamiltonian


def dev(t):
    return t.to(DEV)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def grads(out, inputs, g):
    """torch.autograd.grad that gives zeros for an input the output does not depend on."""
    got = torch.autograd.grad(out, inputs, g, allow_unused=True, retain_graph=True)
    return [torch.zeros_like(i) if x is None else x for x, i in zip(got, inputs)]


def err_word(plan):
    return int(plan.err.item())


# ---- the per-batch tables, built in numpy -----------------------------------------------------------------------------------------------------------------
def tables_np(z, ptr, pairs, slots):
    """orb_atom, orb_slot [sum M_b], look [sum n_b^2] (-1 = no such pair), and the prefix arrays, from the definitions in include/nablaq.h."""
    z, ptr = [int(a) for a in z], [int(p) for p in ptr]
    orb_atom = [i for i, a in enumerate(z) for _ in slots[a]]
    orb_slot = [s for a in z for s in slots[a]]
    n = np.diff(ptr)
    base = np.concatenate([[0], np.cumsum(n * n)])
    mol = np.repeat(np.arange(len(n)), n)
    look = np.full(int(base[-1]), -1, dtype=np.int32)
    for e, (d, s) in enumerate(zip(pairs[0].tolist(), pairs[1].tolist())):
        if mol[d] == mol[s] and d != s:
            b = mol[d]
            look[base[b] + (d - ptr[b]) * n[b] + (s - ptr[b])] = e
    norb = np.array([len(slots[a]) for a in z])
    orb_ptr = np.concatenate([[0], np.cumsum(norb)])
    mol_orb_ptr = orb_ptr[ptr]
    m = np.diff(mol_orb_ptr)
    return dict(orb_atom=np.array(orb_atom, dtype=np.int32), orb_slot=np.array(orb_slot, dtype=np.int32), look=look, pair_base=base, orb_ptr=orb_ptr,
                mol_orb_ptr=mol_orb_ptr, pack_ptr=np.concatenate([[0], np.cumsum(m * m)]), atom_mol=mol.astype(np.int32))


def assert_tables(plan, want):
    n_look = want["look"].size
    assert plan.look.numel() == max(n_look, 1)
    assert np.array_equal(plan.look.cpu().numpy()[:n_look], want["look"])
    for k in ("orb_atom", "orb_slot", "pair_base", "orb_ptr", "mol_orb_ptr", "pack_ptr", "atom_mol"):
        assert np.array_equal(getattr(plan, k).cpu().numpy(), want[k]), k
    assert plan.total == int(want["pack_ptr"][-1]) and plan.m_total == int(want["mol_orb_ptr"][-1])


def tables_again(helper, plan, look_count):
    """nq_hblock_tables itself over poisoned buffers and an error word left set by an earlier plan."""
    table, count, _ = helper._tables(torch.device(DEV))

    def call():
        orb_atom = torch.full((plan.m_total,), -7, device=DEV, dtype=torch.int32)
        orb_slot = torch.full((plan.m_total,), -7, device=DEV, dtype=torch.int32)
        look = torch.full((max(look_count, 1),), -7, device=DEV, dtype=torch.int32)
        err = torch.full((1,), 7, device=DEV, dtype=torch.int32)
        check(lib().nq_hblock_tables(P(plan.z), P(plan.atom_mol), P(plan.mol_ptr), plan.N, plan.B, P(plan.orb_ptr), P(plan.pair_base), P(plan.e_dst), P(plan.e_src),
                                     plan.P, P(table), P(count), helper.S, P(orb_atom), P(orb_slot), P(look), look_count, P(err), st()))
        return orb_atom, orb_slot, look[:look_count], err
    return twice(call)


# ---- QHNet blocks -----------------------------------------------------------------------------------------------------------------------------------------
QH = R.qh_cases()
MASKS = HB.orbital_masks(ORBITALS)[0]
QH_NAMES = list(QH)


@functools.lru_cache(maxsize=None)
def qh_asm():
    return HM().BlockAssembler(ORBITALS)


@functools.lru_cache(maxsize=None)
def qh_inputs(name):
    """diag [N, S, S], nondiag [P, S, S] and a packed seed, all random and none symmetric; a permuted case holds the rows of its base case, permuted."""
    c = QH[name]
    gen = torch.Generator().manual_seed(100 + len(c.mols))
    diag, nondiag = torch.randn(c.N, S, S, generator=gen), torch.randn(c.P, S, S, generator=gen)
    morb = R.mol_orbitals(c.z, c.ptr, {zz: len(m) for zz, m in MASKS.items()})
    G = torch.randn(sum(m * m for m in morb), generator=gen)
    if c.perm is not None:
        nondiag = nondiag[c.perm]
    return diag, nondiag, G, morb


def qh_restate(z, ptr, pairs, diag, nondiag, G, morb, sym):
    """(packed, dense, g_diag, g_nondiag) of the restatement in float32."""
    d, n = diag.clone().requires_grad_(True), nondiag.clone().requires_grad_(True)
    dense = HB.build_final_matrix(z, ptr, pairs, MASKS, d, n, symmetrize=bool(sym))
    packed = R.pack(dense, morb)
    gd, gn = grads(packed, [d, n], G)
    return packed.detach(), dense.detach(), gd, gn


@functools.lru_cache(maxsize=None)
def qh_ref(name, sym):
    c = QH[name]
    return qh_restate(c.z, c.ptr, c.pairs, *qh_inputs(name), sym)


@functools.lru_cache(maxsize=None)
def qh_plan(name):
    c = QH[name]
    return qh_asm().plan(dev(c.z), dev(c.ptr), dev(c.pairs))


def hb_forward(plan, diag, nondiag, sym):
    d, n = dev(diag), dev(nondiag)

    def call():
        out = nan_dev(plan.total)
        check(lib().nq_hblock_assemble(P(d), P(n), P(plan.mol_ptr), P(plan.pair_base), P(plan.pack_ptr), P(plan.mol_orb_ptr), P(plan.orb_atom), P(plan.orb_slot),
                                       P(plan.look), plan.B, S, sym, plan.total, P(out), P(plan.err), st()))
        return (out,)
    return twice(call)[0].cpu()


def hb_backward(plan, G, sym):
    g = dev(G)
    inv = qh_asm()._inv(torch.device(DEV))

    def call():
        gd, gn = nan_dev(plan.N, S, S), nan_dev(plan.P, S, S)
        check(lib().nq_hblock_assemble_backward(P(g), P(plan.z), P(plan.atom_mol), P(plan.orb_ptr), P(plan.pack_ptr), P(plan.mol_orb_ptr), P(inv), P(plan.e_dst),
                                                P(plan.e_src), plan.N, plan.P, S, sym, P(gd), P(gn), st()))
        return gd, gn
    gd, gn = twice(call)
    return gd.cpu(), gn.cpu()


def used_slots(z_rows, z_cols):
    """[rows, S, S] bool: slot (u, v) of the block lies inside the masks of the row atom and of the column atom."""
    m = torch.zeros(max(MASKS) + 1, S, dtype=torch.bool)
    for zz, slots in MASKS.items():
        m[zz, slots] = True
    return m[z_rows][:, :, None] & m[z_cols][:, None, :]


@pytest.mark.parametrize("name", QH_NAMES)
def test_qh_tables(name):
    c, plan = QH[name], qh_plan(name)
    want = tables_np(c.z, c.ptr, c.pairs, MASKS)
    assert_tables(plan, want)
    assert err_word(plan) == 0 and (plan.N, plan.B, plan.P) == (c.N, c.B, c.P)
    assert int((want["look"] < 0).sum()) == c.N                       # exactly the diagonal of every molecule's table is absent
    orb_atom, orb_slot, look, err = tables_again(qh_asm(), plan, want["look"].size)
    assert np.array_equal(orb_atom.cpu().numpy(), want["orb_atom"]) and np.array_equal(orb_slot.cpu().numpy(), want["orb_slot"])
    assert np.array_equal(look.cpu().numpy(), want["look"]) and int(err.item()) == 0


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("name", QH_NAMES)
def test_qh_forward(name, sym):
    diag, nondiag, _, _ = qh_inputs(name)
    plan = qh_plan(name)
    out = hb_forward(plan, diag, nondiag, sym)
    assert not torch.isnan(out).any()
    assert same_bits(out, qh_ref(name, sym)[0])
    assert err_word(plan) == 0
    if QH[name].perm is not None:                                    # the same batch with its pairs in radius-graph order: bitwise the same matrix
        base = next(k for k, b in QH.items() if b.perm is None and b.mols == QH[name].mols)
        assert same_bits(out, hb_forward(qh_plan(base), *qh_inputs(base)[:2], sym))


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("name", QH_NAMES)
def test_qh_backward(name, sym):
    c, plan = QH[name], qh_plan(name)
    _, _, G, morb = qh_inputs(name)
    Gd = R.unpack(G, morb)
    assert not torch.equal(Gd, Gd.T)
    gd, gn = hb_backward(plan, G, sym)
    assert not torch.isnan(gd).any() and not torch.isnan(gn).any()
    _, _, rd, rn = qh_ref(name, sym)
    assert same_bits(gd, rd) and same_bits(gn, rn)
    assert (bits(gd)[~used_slots(c.z, c.z)] == 0).all() and (bits(gn)[~used_slots(c.z[c.pairs[0]], c.z[c.pairs[1]])] == 0).all()
    assert (gd[used_slots(c.z, c.z)] != 0).all()                     # and every slot inside the masks received its element of the seed
    if c.perm is not None:
        base = next(k for k, b in QH.items() if b.perm is None and b.mols == c.mols)
        bd, bn = hb_backward(qh_plan(base), qh_inputs(base)[2], sym)
        assert same_bits(gd, bd) and same_bits(gn, bn[c.perm])


def test_qh_atoms_only_autograd():
    """P = 0 through BlockAssembler.assemble and autograd: an empty nondiag is a NULL pointer on both sweeps."""
    c, plan = QH["atoms only"], qh_plan("atoms only")
    diag, nondiag, G, _ = qh_inputs("atoms only")
    assert nondiag.shape == (0, S, S) and plan.P == 0
    d, n = dev(diag).requires_grad_(True), dev(nondiag).requires_grad_(True)
    for sym in (False, True):
        out = qh_asm().assemble(plan, d, n, symmetrize=sym)
        gd, gn = torch.autograd.grad(out, [d, n], dev(G))
        ref, _, rd, _ = qh_ref("atoms only", int(sym))
        assert same_bits(out, ref) and same_bits(gd, rd) and gn.shape == (0, S, S)
    qh_asm().check(plan)


@pytest.mark.parametrize("name", ["edges", "one", "atoms only"])
def test_qh_packed_dense(name):
    plan = qh_plan(name)
    _, _, _, morb = qh_inputs(name)
    packed, dense, _, _ = qh_ref(name, 0)
    M = sum(morb)
    pk = dev(packed)

    def to_dense():
        out = nan_dev(M, M)
        check(lib().nq_hblock_packed_dense(P(pk), P(out), P(plan.pack_ptr), P(plan.mol_orb_ptr), plan.B, plan.total, plan.m_total, 1, st()))
        return (out,)
    (got,) = twice(to_dense)
    assert same_bits(got, dense)                                     # +0.0 everywhere off the blocks
    holes = dev(R.unpack(packed, morb, fill=float("nan")))
    assert int(torch.isnan(holes).sum()) == M * M - plan.total

    def from_dense():
        out = nan_dev(plan.total)
        check(lib().nq_hblock_packed_dense(P(out), P(holes), P(plan.pack_ptr), P(plan.mol_orb_ptr), plan.B, plan.total, plan.m_total, 0, st()))
        return (out,)
    (back,) = twice(from_dense)
    assert not torch.isnan(back).any() and same_bits(back, packed)
    assert same_bits(qh_asm().from_dense(plan, qh_asm().to_dense(plan, pk)), packed)     # the round trip through the Python wrappers


@pytest.mark.parametrize("kind", ["two molecules", "self pair", "missing pair", "both"])
@pytest.mark.parametrize("sym", [0, 1])
def test_qh_error_word(kind, sym):
    """Forward only: the reverse kernel trusts the pair list.  The restatement of the expected matrix holds a zero block where a pair is missing."""
    c = QH["edges"]
    diag, nondiag, G, morb = qh_inputs("edges")
    asm = qh_asm()
    k = c.P - 17                                                     # a pair of the seven-atom molecule: (dst, src) = pairs[:, k]
    d_k, s_k = int(c.pairs[0, k]), int(c.pairs[1, k])
    assert d_k >= 7 and s_k >= 7
    extra_row = torch.randn(1, S, S, generator=torch.Generator().manual_seed(5))
    zeroed = nondiag.clone()
    zeroed[k] = 0
    if kind in ("two molecules", "self pair"):                       # one column more, in the middle of the list; every needed pair is still there
        col = torch.tensor([[d_k], [2 if kind == "two molecules" else d_k]])
        pairs = torch.cat([c.pairs[:, :k], col, c.pairs[:, k:]], dim=1)
        blocks = torch.cat([nondiag[:k], extra_row, nondiag[k:]])
        want, after_tables, after_launch = qh_restate(c.z, c.ptr, pairs, diag, blocks, G, morb, sym)[0], 1, 1
    elif kind == "missing pair":
        pairs, blocks = torch.cat([c.pairs[:, :k], c.pairs[:, k + 1:]], dim=1), torch.cat([nondiag[:k], nondiag[k + 1:]])
        want, after_tables, after_launch = qh_restate(c.z, c.ptr, c.pairs, diag, zeroed, G, morb, sym)[0], 0, 2
    else:                                                            # the column of (d_k, s_k) now joins d_k to an atom of another molecule
        pairs = c.pairs.clone()
        pairs[1, k] = 2
        blocks = nondiag
        want, after_tables, after_launch = qh_restate(c.z, c.ptr, c.pairs, diag, zeroed, G, morb, sym)[0], 1, 3
    plan = asm.plan(dev(c.z), dev(c.ptr), dev(pairs))
    assert err_word(plan) == after_tables
    assert_tables(plan, tables_np(c.z, c.ptr, pairs, MASKS))
    out = hb_forward(plan, diag, blocks, sym)
    assert err_word(plan) == after_launch
    assert same_bits(out, want)
    with pytest.raises(IndexError, match="every ordered atom pair" if after_launch & 2 else "joins two molecules"):
        asm.check(plan)
    good = asm.plan(dev(c.z), dev(c.ptr), dev(c.pairs))
    assert same_bits(hb_forward(good, diag, nondiag, sym), qh_ref("edges", sym)[0]) and err_word(good) == 0
    asm.check(good)


def test_qh_refusals():
    c, plan = QH["edges"], qh_asm().plan(dev(QH["edges"].z), dev(QH["edges"].ptr), dev(QH["edges"].pairs))
    diag, nondiag, G, _ = qh_inputs("edges")
    d, n = dev(diag), dev(nondiag)
    plan.err.fill_(64)
    for bad_d, bad_n in [(d, n[:-1]), (d, n[:0]), (d[:-1], n), (d[:, :, :-1], n), (d, n.view(c.P, S * S)), (n, d)]:
        with pytest.raises(ValueError, match="the plan needs"):
            qh_asm().assemble(plan, bad_d, bad_n)
    assert err_word(plan) == 64
    g = dev(G)
    inv = qh_asm()._inv(torch.device(DEV))
    gd = nan_dev(c.N, S, S)
    rejected(lambda: lib().nq_hblock_assemble_backward(P(g), P(plan.z), P(plan.atom_mol), P(plan.orb_ptr), P(plan.pack_ptr), P(plan.mol_orb_ptr), P(inv),
                                                       P(plan.e_dst), P(plan.e_src), plan.N, plan.P, S, 1, P(gd), None, st()), gd)
    gn = nan_dev(c.P, S, S)
    rejected(lambda: lib().nq_hblock_assemble_backward(P(g), P(plan.z), P(plan.atom_mol), P(plan.orb_ptr), P(plan.pack_ptr), P(plan.mol_orb_ptr), P(inv),
                                                       None, P(plan.e_src), plan.N, plan.P, S, 1, P(gd), P(gn), st()), gd, gn)
    assert err_word(plan) == 64


# ---- PhiSNet irreps ---------------------------------------------------------------------------------------------------------------------------------------
IR = R.ir_cases()
IR_NAMES = list(IR)
FLAGS = [(0, 0), (1, 0), (0, 1), (1, 1)]                             # (symmetrize, unit_diagonal)
DROPPED = (8, 1, 3, 2, 1)                                            # O 2p (shell 3) x H 2p (shell 2), the middle one of L = 0, 1, 2


def ir_orbitals(name):
    return R.IR_S_ONLY if name == "s only" else R.IR_ORBITALS


@functools.lru_cache(maxsize=None)
def ir_setup(kind):
    """(assembler, atom2orbitals, irreps_ii, irreps_ij, Fo); kind: "spd", "s only", or "dropped" = "spd" without the key DROPPED in irreps_ij."""
    a2o = R.IR_S_ONLY if kind == "s only" else R.IR_ORBITALS
    ii, ij = R.irreps_dictionaries(a2o, HM().compute_matrix_irreps)
    Fo = max(max(ii.values()), max(ij.values())) + 1 + 3
    if kind == "dropped":
        del ij[DROPPED]
    return HM().IrrepsAssembler(a2o, ii, ij, FixtureCG()), a2o, ii, ij, Fo


def ir_kind(name):
    return "s only" if name == "s only" else "spd"


@functools.lru_cache(maxsize=None)
def ir_inputs(name, ncomp):
    """f_ii [N, ncomp, Fo], f_ij [P, ncomp, Fo]: random, with NaN in every column the dictionaries do not use of that order (all of them past L = 4), and a
    random non-symmetric packed seed.  A permuted case holds the rows of its base case, permuted."""
    c = IR[name]
    _, a2o, ii, ij, Fo = ir_setup(ir_kind(name))
    gen = torch.Generator().manual_seed(200 + len(c.mols))
    f_ii, f_ij = torch.randn(c.N, ncomp, Fo, generator=gen), torch.randn(c.P, ncomp, Fo, generator=gen)
    for f, table in ((f_ii, ii), (f_ij, ij)):
        cols = R.columns_per_L(table)
        for comp in range(ncomp):
            L = int(np.sqrt(comp))
            f[:, comp, (cols[L] if L < 5 else 0):] = float("nan")
    morb = R.mol_orbitals(c.z, c.ptr, {zz: R.shell_offsets(s)[1] for zz, s in a2o.items()})
    G = torch.randn(sum(m * m for m in morb), generator=gen)
    if c.perm is not None:
        f_ij = f_ij[c.perm]
    return f_ii, f_ij, G, morb


def padding(name, ncomp):
    f_ii, f_ij, _, _ = ir_inputs(name, ncomp)
    return torch.isnan(f_ii), torch.isnan(f_ij)


@functools.lru_cache(maxsize=None)
def ir_blocks(name, ncomp, dtype, kind):
    """The restatement's molecule matrices before symmetrisation, as a graph on leaf copies of the inputs; built once per (case, dtype, dictionaries)."""
    c = IR[name]
    _, a2o, ii, ij, _ = ir_setup(kind)
    f_ii, f_ij, _, _ = ir_inputs(name, ncomp)
    a, b = f_ii.to(dtype).clone().requires_grad_(True), f_ij.to(dtype).clone().requires_grad_(True)      # .to() alone would hand back the shared float32 inputs
    mats = R.irreps_blocks(c.z, c.ptr, c.pairs[0], c.pairs[1], a2o, ii, ij, FixtureCG(), a, b, skip_missing=(kind == "dropped"))
    return mats, a, b


@functools.lru_cache(maxsize=None)
def ir_ref(name, ncomp, dtype, kind, sym, unit, diagonal_seed=False):
    """(packed, g_ii, g_ij) of the restatement in ``dtype``."""
    mats, a, b = ir_blocks(name, ncomp, dtype, kind)
    G = ir_seed(name, ncomp, diagonal_seed)
    packed = R.finish(mats, sym, unit)
    g_ii, g_ij = grads(packed, [a, b], G.to(dtype))
    assert not torch.isnan(packed).any() and not torch.isnan(g_ii).any() and not torch.isnan(g_ij).any()
    return packed.detach(), g_ii, g_ij


def ir_seed(name, ncomp, diagonal_only):
    _, _, G, morb = ir_inputs(name, ncomp)
    if diagonal_only:
        G = R.pack(torch.diag(torch.diagonal(R.unpack(G, morb))), morb)
    return G


@functools.lru_cache(maxsize=None)
def ir_plan(name, kind=None):
    c = IR[name]
    return ir_setup(kind or ir_kind(name))[0].plan(dev(c.z), dev(c.ptr), dev(c.pairs[0]), dev(c.pairs[1]))


TABLE_ARGS = ("tz", "sh_n", "sh_l", "sh_m", "sh_off")


def ir_forward(asm, plan, f_ii, f_ij, sym, unit):
    a, b = dev(f_ii), dev(f_ij)
    t = asm._tables(torch.device(DEV))
    ncomp, Fo = f_ii.shape[1], f_ii.shape[2]

    def call():
        out = nan_dev(plan.total)
        check(lib().nq_irreps_assemble(P(a), P(b), P(plan.z), P(plan.mol_ptr), P(plan.pair_base), P(plan.pack_ptr), P(plan.mol_orb_ptr), P(plan.orb_ptr),
                                       P(plan.orb_atom), P(plan.orb_slot), P(plan.look), plan.B, ncomp, Fo, *[P(t[k]) for k in TABLE_ARGS], P(t["idx_ii"]),
                                       P(t["idx_ij"]), P(t["cgt"]), asm.T, asm.S, sym, unit, plan.total, P(out), P(plan.err), st()))
        return (out,)
    return twice(call)[0].cpu()


def ir_backward(asm, plan, G, ncomp, Fo, sym, unit):
    g = dev(G)
    t = asm._tables(torch.device(DEV))
    inv_ii, inv_ij = asm._inverse(Fo, torch.device(DEV))

    def call():
        g_ii, g_ij = nan_dev(plan.N, ncomp, Fo), nan_dev(plan.P, ncomp, Fo)
        check(lib().nq_irreps_assemble_backward(P(g), P(plan.z), P(plan.atom_mol), P(plan.e_dst), P(plan.e_src), P(plan.pack_ptr), P(plan.mol_orb_ptr),
                                                P(plan.orb_ptr), P(inv_ii), P(inv_ij), plan.N, plan.P, ncomp, Fo, *[P(t[k]) for k in TABLE_ARGS], P(t["cgt"]),
                                                asm.T, asm.S, sym, unit, P(g_ii), P(g_ij), st()))
        return g_ii, g_ij
    g_ii, g_ij = twice(call)
    return g_ii.cpu(), g_ij.cpu()


def ncomp_of(name):
    return 1 if name == "s only" else 25


def base_of(name):
    return next(k for k, b in IR.items() if b.perm is None and b.mols == IR[name].mols)


def diagonal_positions(morb):
    q, pos = 0, []
    for m in morb:
        pos.extend(q + r * (m + 1) for r in range(m))
        q += m * m
    return torch.tensor(pos)


def measured(name, got, ref64, ref32):
    err = assert_sum(name, got, ref64, ref32)
    record(name, err, rel(ref32.detach().double().numpy(), ref64.detach().numpy()))


@pytest.mark.parametrize("name", IR_NAMES)
def test_ir_tables(name):
    c, plan = IR[name], ir_plan(name)
    asm, a2o, _, _, _ = ir_setup(ir_kind(name))
    want = tables_np(c.z, c.ptr, c.pairs, {zz: list(range(R.shell_offsets(s)[1])) for zz, s in a2o.items()})
    assert_tables(plan, want)
    assert err_word(plan) == 0
    orb_atom, orb_slot, look, err = tables_again(asm._plan_helper, plan, want["look"].size)
    assert np.array_equal(orb_atom.cpu().numpy(), want["orb_atom"]) and np.array_equal(orb_slot.cpu().numpy(), want["orb_slot"])
    assert np.array_equal(look.cpu().numpy(), want["look"]) and int(err.item()) == 0


@pytest.mark.parametrize("sym,unit", FLAGS)
@pytest.mark.parametrize("name", IR_NAMES)
def test_ir_forward(name, sym, unit):
    ncomp, kind = ncomp_of(name), ir_kind(name)
    asm, plan = ir_setup(kind)[0], ir_plan(name)
    f_ii, f_ij, _, morb = ir_inputs(name, ncomp)
    assert torch.isnan(f_ii[:, :, -3:]).all() and torch.isnan(f_ij[:, :, -3:]).all()
    out = ir_forward(asm, plan, f_ii, f_ij, sym, unit)
    base = base_of(name)                                             # a permuted pair list has the values of its base case
    measured(f"value {name} sym={sym} unit={unit}", out, ir_ref(base, ncomp, F64, kind, sym, unit)[0], ir_ref(base, ncomp, F32, kind, sym, unit)[0])
    assert err_word(plan) == 0
    if unit:
        assert (bits(out)[diagonal_positions(morb)] == bits(torch.ones(1))[0]).all()
    if base != name:
        assert same_bits(out, ir_forward(asm, ir_plan(base), *ir_inputs(base, ncomp)[:2], sym, unit))


@pytest.mark.parametrize("sym,unit", FLAGS)
@pytest.mark.parametrize("name", IR_NAMES)
def test_ir_backward(name, sym, unit):
    ncomp, kind = ncomp_of(name), ir_kind(name)
    asm, _, _, _, Fo = ir_setup(kind)
    c, plan = IR[name], ir_plan(name)
    _, _, G, morb = ir_inputs(name, ncomp)
    Gd = R.unpack(G, morb)
    assert not torch.equal(Gd, Gd.T)
    g_ii, g_ij = ir_backward(asm, plan, G, ncomp, Fo, sym, unit)
    base = base_of(name)
    _, r_ii, r_ij = ir_ref(base, ncomp, F64, kind, sym, unit)
    _, s_ii, s_ij = ir_ref(base, ncomp, F32, kind, sym, unit)
    if c.perm is not None:
        r_ij, s_ij = r_ij[c.perm], s_ij[c.perm]
    measured(f"grad f_ii {name} sym={sym} unit={unit}", g_ii, r_ii, s_ii)
    measured(f"grad f_ij {name} sym={sym} unit={unit}", g_ij, r_ij, s_ij)
    pad_ii, pad_ij = padding(name, ncomp)
    assert pad_ii.any() and pad_ij.any() and (g_ii[pad_ii] == 0).all() and (g_ij[pad_ij] == 0).all()
    if c.perm is not None:
        b_ii, b_ij = ir_backward(asm, ir_plan(base), ir_inputs(base, ncomp)[2], ncomp, Fo, sym, unit)
        assert same_bits(g_ii, b_ii) and same_bits(g_ij, b_ij[c.perm])


@pytest.mark.parametrize("sym", [0, 1])
def test_ir_unit_diagonal_seed(sym):
    """A seed that lives on the diagonal only: with unit_diagonal the matrix does not depend on the features there, so both gradients are exactly 0; without
    it the same seed gives the restatement's non-zero gradient."""
    name, ncomp = "batch", 25
    asm, _, _, _, Fo = ir_setup("spd")
    G = ir_seed(name, ncomp, True)
    assert int((G != 0).sum()) == sum(ir_inputs(name, ncomp)[3])
    g_ii, g_ij = ir_backward(asm, ir_plan(name), G, ncomp, Fo, sym, 1)
    assert (g_ii == 0).all() and (g_ij == 0).all()
    g_ii, g_ij = ir_backward(asm, ir_plan(name), G, ncomp, Fo, sym, 0)
    _, r_ii, r_ij = ir_ref(name, ncomp, F64, "spd", sym, 0, True)
    _, s_ii, s_ij = ir_ref(name, ncomp, F32, "spd", sym, 0, True)
    assert float(r_ii.abs().max()) > 0
    measured(f"grad f_ii diagonal seed sym={sym}", g_ii, r_ii, s_ii)
    assert (g_ij == 0).all() and (r_ij == 0).all()                  # no pair block touches the diagonal


def test_ir_wide_ncomp():
    """ncomp = 36: components 25..35 (L = 5) are NaN on input, never read, and their gradient is exactly 0; the rest is the ncomp = 25 result bit for bit."""
    name, sym, unit = "one", 1, 0
    asm, _, _, _, Fo = ir_setup("spd")
    plan = ir_plan(name)
    f_ii, f_ij, G, _ = ir_inputs(name, 25)
    nan_rows = lambda f: torch.cat([f, torch.full((f.shape[0], 11, Fo), float("nan"))], dim=1)
    w_ii, w_ij = nan_rows(f_ii), nan_rows(f_ij)
    assert w_ii.shape[1] == 36 and torch.isnan(w_ij[:, 25:]).all()
    out = ir_forward(asm, plan, w_ii, w_ij, sym, unit)
    measured("value ncomp=36", out, ir_ref(name, 25, F64, "spd", sym, unit)[0], ir_ref(name, 25, F32, "spd", sym, unit)[0])
    assert same_bits(out, ir_forward(asm, plan, f_ii, f_ij, sym, unit))
    g_ii, g_ij = ir_backward(asm, plan, G, 36, Fo, sym, unit)
    assert (bits(g_ii[:, 25:]) == 0).all() and (bits(g_ij[:, 25:]) == 0).all()
    n_ii, n_ij = ir_backward(asm, plan, G, 25, Fo, sym, unit)
    assert same_bits(g_ii[:, :25], n_ii) and same_bits(g_ij[:, :25], n_ij)
    _, r_ii, r_ij = ir_ref(name, 25, F64, "spd", sym, unit)
    _, s_ii, s_ij = ir_ref(name, 25, F32, "spd", sym, unit)
    measured("grad f_ii ncomp=36", g_ii[:, :25], r_ii, s_ii)
    measured("grad f_ij ncomp=36", g_ij[:, :25], r_ij, s_ij)


@pytest.mark.parametrize("sym", [0, 1])
def test_ir_missing_key(sym):
    name, ncomp = "one", 25
    asm, _, _, ij, Fo = ir_setup("dropped")
    assert DROPPED not in ij and DROPPED in ir_setup("spd")[3]
    plan = ir_plan(name, "dropped")
    f_ii, f_ij, G, _ = ir_inputs(name, ncomp)
    out = ir_forward(asm, plan, f_ii, f_ij, sym, 0)
    assert err_word(plan) == 4
    with pytest.raises(KeyError):
        asm.check(plan)
    full64, full32 = ir_ref(name, ncomp, F64, "spd", sym, 0)[0], ir_ref(name, ncomp, F32, "spd", sym, 0)[0]
    skip64, skip32 = ir_ref(name, ncomp, F64, "dropped", sym, 0)[0], ir_ref(name, ncomp, F32, "dropped", sym, 0)[0]
    affected = full64 != skip64
    assert int(affected.sum()) == 6 * (2 if sym else 1)             # the 3 x 3 block of the two p shells less its diagonal (CG(1 m, 1 m | 1 M) = 0), and its mirror image
    measured(f"value missing key sym={sym}: elements without the key", out[~affected], full64[~affected], full32[~affected])
    measured(f"value missing key sym={sym}: all, against the restatement without that L term", out, skip64, skip32)
    scale = float(skip64.abs().max())
    assert float((out[affected].double() - skip64[affected]).abs().max()) <= 2e-6 * scale < 0.01 * float((full64 - skip64)[affected].abs().max())
    g_ii, g_ij = ir_backward(asm, plan, G, ncomp, Fo, sym, 0)       # the column of the dropped key has no inverse entry: code < 0
    _, r_ii, r_ij = ir_ref(name, ncomp, F64, "dropped", sym, 0)
    _, s_ii, s_ij = ir_ref(name, ncomp, F32, "dropped", sym, 0)
    measured(f"grad f_ii missing key sym={sym}", g_ii, r_ii, s_ii)
    measured(f"grad f_ij missing key sym={sym}", g_ij, r_ij, s_ij)
    good = ir_setup("spd")[0].plan(dev(IR[name].z), dev(IR[name].ptr), dev(IR[name].pairs[0]), dev(IR[name].pairs[1]))
    ir_forward(ir_setup("spd")[0], good, f_ii, f_ij, sym, 0)
    assert err_word(good) == 0


def test_ir_missing_pair():
    """Forward only.  Without the row of pair k its block is 0 (and the mirror image gets only the other pair's term): the restatement on a zero row."""
    name, ncomp, sym = "one", 25, 1
    c = IR[name]
    asm = ir_setup("spd")[0]
    f_ii, f_ij, _, _ = ir_inputs(name, ncomp)
    k = 4
    keep = [e for e in range(c.P) if e != k]
    plan = asm.plan(dev(c.z), dev(c.ptr), dev(c.pairs[0, keep]), dev(c.pairs[1, keep]))
    out = ir_forward(asm, plan, f_ii, f_ij[keep], sym, 0)
    assert err_word(plan) == 2
    with pytest.raises(IndexError, match="every ordered atom pair"):
        asm.check(plan)
    want = []
    for dtype in (F64, F32):
        z_ij = f_ij.to(dtype).clone()
        z_ij[k] = 0
        want.append(R.irreps_matrix(c.z, c.ptr, c.pairs[0], c.pairs[1], R.IR_ORBITALS, *ir_setup("spd")[2:4], FixtureCG(), f_ii.to(dtype), z_ij, sym, 0))
    measured("value missing pair", out, *want)


def test_ir_refusals():
    name, ncomp = "one", 25
    c = IR[name]
    asm, _, _, _, Fo = ir_setup("spd")
    plan = asm.plan(dev(c.z), dev(c.ptr), dev(c.pairs[0]), dev(c.pairs[1]))
    f_ii, f_ij, G, _ = ir_inputs(name, ncomp)
    a, b = dev(f_ii), dev(f_ij)
    plan.err.fill_(64)
    tight = asm.max_index + 1
    assert Fo == tight + 3
    for bad_a, bad_b in [(a, b[:, :, :-1]),                          # a too-narrow f_ij
                         (a, b[:, :16]), (a[:, :24], b[:, :24]),     # a too-small ncomp, in one tensor and in both
                         (a[:, :, :tight - 1], b[:, :, :tight - 1]), (a[:-1], b), (a, b[:-1]), (a, b[:0]), (a.view(c.N, -1), b)]:
        with pytest.raises(ValueError):
            asm.assemble(plan, bad_a, bad_b)
    assert err_word(plan) == 64
    t = asm._tables(torch.device(DEV))
    inv_ii, inv_ij = asm._inverse(Fo, torch.device(DEV))
    g, g_ii, g_ij = dev(G), nan_dev(c.N, ncomp, Fo), nan_dev(c.P, ncomp, Fo)
    for e_i, out_ij in ((P(plan.e_dst), None), (None, P(g_ij))):
        rejected(lambda: lib().nq_irreps_assemble_backward(P(g), P(plan.z), P(plan.atom_mol), e_i, P(plan.e_src), P(plan.pack_ptr), P(plan.mol_orb_ptr),
                                                           P(plan.orb_ptr), P(inv_ii), P(inv_ij), plan.N, plan.P, ncomp, Fo, *[P(t[k]) for k in TABLE_ARGS],
                                                           P(t["cgt"]), asm.T, asm.S, 1, 0, P(g_ii), out_ij, st()), g_ii, g_ij)
    assert err_word(plan) == 64
    # the tightest width the contract admits runs, and gives the same matrix
    plan.err.zero_()
    out = asm.assemble(plan, a[:, :, :tight].contiguous(), b[:, :, :tight].contiguous(), symmetrize=True)
    measured("value at the tightest Fo", out.cpu(), ir_ref(name, ncomp, F64, "spd", 1, 0)[0], ir_ref(name, ncomp, F32, "spd", 1, 0)[0])
    asm.check(plan)
