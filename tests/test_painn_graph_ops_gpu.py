"""The PaiNN neighbour-list kernels (csrc/graph.hip: k_graph_count, k_scan2, k_graph_fill) through nq_graph_count / nq_graph_fill and through
build_neighbor_list, against the tables tests/painn_graph_cases.py derives from the CPU oracle's canonical edge list (oracle/painn_ref.py: build_graph),
on batches built to reach what the six clouds of tests/golden/graph_cases.npz never reach.  Every output buffer of the direct calls starts as a sentinel
(-1 for index arrays, a negative garbage value for counters and pointers, NaN for geometry), so an element a kernel never writes fails; count + fill run
twice into fresh buffers and must agree bitwise; build_neighbor_list (canonical or not) must return the same bits.

Bounds: none.  Every integer output is compared exactly, and edge_dist / edge_vector / geom bit for bit with the IEEE float32 evaluation of the
reference's formulas by numpy (DESIGN.md row a1-a3 in its stronger form).  tests/test_painn_graph_cases_cpu.py asserts on the oracle alone that every
batch still has the property named below.

Branches and the cases that reach them (test_graph_tables[case]):
  build_adjacency  the K trim inside the first word: complete130-K1; of the whole second word: -K64; inside the second word: -K65, -K70; past it: -K100;
                   inside and of whole later words of molecules of 63 .. 193 atoms: words-K5; the cutoff alone selecting: words-K100; W = 8: limit512;
                   d^2 == r^2 excluded, one ulp inside kept: at_cutoff; the upper half (j > i) of rows longer than a word: complete130-*
  k_graph_count    n <= 0: empty-ptr, empty-batch; the opt-in dynamic-LDS launch (71,680 B): limit512, limit512-offset (atom offset 3)
  k_scan2          N = 8191 / 8192 / 8193 / 16385: one element short of a trip, exactly one, a second trip of one element, a third; entry N: all
  k_graph_fill     n <= 0 writes neighbors[g] = 0: empty-*; the d <= 1e-6 branch at d == 0 and d = 4.77e-7: coincident; positions of magnitude 300:
                   far_offset; rank_in_row / slots across words: complete130-*, words-*, limit512; E == 0 (atom_mol and neighbors still written): no_pairs
  refusals (before any launch): max_neighbors = 0, a molecule of 513 atoms (count and fill), NULL outputs, canonical outputs partly given: test_refusals"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from tests import painn_graph_cases as GC  # noqa: E402
from tests.helpers import DEV, P, _LIVE, _lib, _release_copies, check, lib, nan_dev, rejected, st, twice  # noqa: E402,F401  (_release_copies: autouse)

GARBAGE = -7777
COUNT_OUT = ("deg", "lowdeg", "row_ptr", "lowptr")
SLOT_OUT = ("col", "dst", "rev", "slot2canon")
CANON_OUT = ("edge_index", "edge_dist", "edge_vector", "id_swap")
INT_OUT = ("edge_index", "neighbors", "id_swap", "row_ptr", "lowptr", "deg", "lowdeg", "col", "dst", "rev", "slot2canon", "atom_mol")
FLOAT_OUT = ("edge_dist", "edge_vector", "geom")


def full(shape, value, dtype=torch.int32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=DEV)


def inputs(name):
    pos, sizes, cutoff, K = GC.case(name)
    posd, mol_ptr = torch.tensor(pos, device=DEV), torch.tensor(GC.ptr_of(sizes), dtype=torch.int32, device=DEV)
    _LIVE.extend([posd, mol_ptr])
    return posd, mol_ptr, len(pos), len(sizes), max(sizes), cutoff, K


def count_buffers(N):
    return dict(deg=full(N, GARBAGE), lowdeg=full(N, GARBAGE), row_ptr=full(N + 1, GARBAGE), lowptr=full(N + 1, GARBAGE))


def fill_buffers(N, B, E, canonical=True):
    out = {k: full(E, -1) for k in SLOT_OUT}
    out.update(geom=nan_dev(E, 4), atom_mol=full(N, -1), neighbors=full(B, GARBAGE, torch.int64))
    if canonical:
        out.update(edge_index=full((2, E), -1, torch.int64), edge_dist=nan_dev(E), edge_vector=nan_dev(E, 3), id_swap=full(E, -1, torch.int64))
    return out


def call_fill(posd, mol_ptr, N, B, E, max_n, cutoff, K, cnt, out):
    return lib().nq_graph_fill(P(posd), P(mol_ptr), N, B, E, max_n, cutoff, K, P(cnt["row_ptr"]), P(cnt["lowptr"]), P(out["col"]), P(out["dst"]),
                               P(out["rev"]), P(out["geom"]), P(out["slot2canon"]), P(out["atom_mol"]), P(out.get("edge_index")),
                               P(out.get("edge_dist")), P(out.get("edge_vector")), P(out.get("id_swap")), P(out["neighbors"]), st())


def count_and_fill(name):
    """name -> device tensor of one nq_graph_count + nq_graph_fill into fresh sentinel-filled buffers."""
    posd, mol_ptr, N, B, max_n, cutoff, K = inputs(name)
    cnt = count_buffers(N)
    e_host = C.c_int32(GARBAGE)
    check(lib().nq_graph_count(P(posd), P(mol_ptr), N, B, max_n, cutoff, K, P(cnt["deg"]), P(cnt["lowdeg"]), P(cnt["row_ptr"]), P(cnt["lowptr"]),
                               C.byref(e_host), st()))
    E = int(e_host.value)
    assert E == GC.tables(name)["E"], (E, GC.tables(name)["E"])     # before anything is sized by it
    out = fill_buffers(N, B, E)
    check(call_fill(posd, mol_ptr, N, B, E, max_n, cutoff, K, cnt, out))
    out.update(cnt)
    return out


def host(t):
    a = t.detach().cpu().numpy()
    return a.astype(np.int64) if a.dtype == np.int32 else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def compare(label, h, T, names):
    for k in names:
        if k in INT_OUT:
            assert h[k].shape == T[k].shape and np.array_equal(h[k], T[k]), (label, k)
        else:
            assert not np.isnan(h[k]).any(), (label, k, "never written")
            assert same_bits(h[k], T[k]), (label, k, int((h[k].view(np.int32) != T[k].view(np.int32)).sum()))


def product(name, canonical, via_ptr):
    from nabladft_amd.painn import build_neighbor_list
    pos, sizes, cutoff, K = GC.case(name)
    posd = torch.tensor(pos, device=DEV)
    batch = torch.tensor(GC.batch_of(sizes), device=DEV)
    ptr = torch.tensor(GC.ptr_of(sizes), device=DEV) if via_ptr else None
    nl = build_neighbor_list(posd, batch, None, cutoff, K, ptr=ptr, canonical=canonical)
    h = {k: host(nl.t[k]) for k in ("row_ptr", "lowptr", "deg", "col", "dst", "rev", "slot2canon", "atom_mol", "geom")}
    h["neighbors"] = host(nl.neighbors)
    if canonical:
        h.update(edge_index=host(nl.edge_index), edge_dist=host(nl.edge_dist), edge_vector=host(nl.edge_vector), id_swap=host(nl.id_swap))
    else:
        assert nl.edge_index is None and nl.edge_dist is None and nl.edge_vector is None and nl.id_swap is None
    assert (nl.N, nl.B, nl.E) == (len(pos), len(sizes), len(h["col"])) and nl.c.max_mol_atoms == max(sizes)
    return h


@pytest.mark.parametrize("name", GC.CASES)
def test_graph_tables(name):
    pos, sizes, cutoff, K = GC.case(name)
    T = GC.tables(name)
    names = []

    def call():
        out = count_and_fill(name)
        names[:] = list(out)
        return [out[k] for k in names]

    h = {k: host(v) for k, v in zip(names, twice(call))}
    print(f"{name}: N {T['N']}  B {T['B']}  E {T['E']}  largest degree {int(T['deg'].max())}  distances <= 1e-6: {int((T['edge_dist'] <= 1e-6).sum())}")
    compare(name, h, T, INT_OUT + FLOAT_OUT)
    if T["E"]:
        GC.check_invariants(dict(h, N=T["N"], E=T["E"]))
    # build_neighbor_list: the same bits, with and without the canonical outputs, through ``ptr`` and (where it can say the batch) through ``batch``
    csr = tuple(k for k in INT_OUT + FLOAT_OUT if k not in CANON_OUT and k != "lowdeg")
    for via_ptr in ((True,) if GC.needs_ptr(sizes) else (False, True)):
        full_, bare = product(name, True, via_ptr), product(name, False, via_ptr)
        compare(f"{name} canonical ptr={via_ptr}", full_, T, csr + CANON_OUT)
        compare(f"{name} bare ptr={via_ptr}", bare, T, csr)
    if T["E"] == 0:
        assert h["edge_index"].shape == (2, 0) and not h["neighbors"].any()


def test_empty_molecules_leave_the_others_unchanged():
    """neighbors[g] == 0 for the empty molecules; every other output equals that of the batch without them (atoms keep their numbers)."""
    ref = product("empty-none", True, False)
    for name, via_ptr in (("empty-ptr", True), ("empty-batch", False), ("empty-batch", True)):
        sizes = np.array(GC.case(name)[1])
        h = product(name, True, via_ptr)
        assert (h["neighbors"][sizes == 0] == 0).all() and np.array_equal(h["neighbors"][sizes > 0], ref["neighbors"])
        for k in ("edge_index", "id_swap", "row_ptr", "lowptr", "deg", "col", "dst", "rev", "slot2canon"):
            assert np.array_equal(h[k], ref[k]), (name, k)
        for k in FLOAT_OUT:
            assert same_bits(h[k], ref[k]), (name, k)
        assert np.array_equal(h["atom_mol"], np.nonzero(sizes > 0)[0][ref["atom_mol"]])


def test_refusals():
    """Argument checks that return before any launch: no buffer is touched."""
    L = _lib()
    posd, mol_ptr, N, B, max_n, cutoff, K = inputs("words-K5")
    E = GC.tables("words-K5")["E"]
    cnt, out = count_buffers(N), fill_buffers(N, B, E)
    e_host = C.c_int32(GARBAGE)

    def untouched():
        assert e_host.value == GARBAGE and (out["neighbors"] == GARBAGE).all()
        for k in COUNT_OUT:
            assert (cnt[k] == GARBAGE).all(), k
        for k in SLOT_OUT + ("atom_mol", "edge_index", "id_swap"):
            assert (out[k] == -1).all(), k

    def refused(code, call):
        rejected(call, out["geom"], out["edge_dist"], out["edge_vector"])
        assert L.load().nq_last_error() and call() == code
        untouched()

    def count(k=K, max_atoms=max_n, deg=cnt["deg"], e=C.byref(e_host)):
        return lib().nq_graph_count(P(posd), P(mol_ptr), N, B, max_atoms, cutoff, k, P(deg), P(cnt["lowdeg"]), P(cnt["row_ptr"]), P(cnt["lowptr"]), e, st())

    refused(L.NQ_ERR_ARG, lambda: count(k=0))
    refused(L.NQ_ERR_ARG, lambda: count(k=-3))
    refused(L.NQ_ERR_ARG, lambda: count(deg=None))
    refused(L.NQ_ERR_ARG, lambda: count(e=None))
    refused(L.NQ_ERR_MOL_TOO_LARGE, lambda: count(max_atoms=513))
    # fill: the count-stage tables are the case's own (valid), so that a call that were not refused would still stay inside its buffers
    T = GC.tables("words-K5")
    good = dict(row_ptr=torch.tensor(T["row_ptr"], dtype=torch.int32, device=DEV), lowptr=torch.tensor(T["lowptr"], dtype=torch.int32, device=DEV))
    for k in SLOT_OUT + ("geom", "atom_mol"):
        refused(L.NQ_ERR_ARG, lambda: call_fill(posd, mol_ptr, N, B, E, max_n, cutoff, K, good, dict(out, **{k: None})))
    for k in ("edge_dist", "edge_vector", "id_swap"):                # canonical outputs only partly given
        refused(L.NQ_ERR_ARG, lambda: call_fill(posd, mol_ptr, N, B, E, max_n, cutoff, K, good, dict(out, **{k: None})))
    refused(L.NQ_ERR_ARG, lambda: call_fill(posd, mol_ptr, N, B, E, max_n, cutoff, K, dict(good, row_ptr=None), out))
    refused(L.NQ_ERR_MOL_TOO_LARGE, lambda: call_fill(posd, mol_ptr, N, B, E, 513, cutoff, K, good, out))


def test_molecule_of_513_atoms_is_refused():
    """One atom past NQ_MAX_MOL_ATOMS: NQ_ERR_MOL_TOO_LARGE from nq_graph_count, from nq_graph_fill and from build_neighbor_list, nothing written.  The
    atoms sit 10 apart on a line with cutoff 1 (no pair, every table zero), so that the buffers given to the refused calls describe this very batch."""
    from nabladft_amd.painn import build_neighbor_list
    L = _lib()
    N = GC.NQ_MAX_MOL_ATOMS + 1
    pos = np.zeros((N, 3), dtype=np.float32)
    pos[:, 0] = 10.0 * np.arange(N)
    posd, mol_ptr = torch.tensor(pos, device=DEV), torch.tensor([0, N], dtype=torch.int32, device=DEV)
    cnt, out = count_buffers(N), fill_buffers(N, 1, 64)
    e_host = C.c_int32(GARBAGE)
    zeros = dict(row_ptr=torch.zeros(N + 1, dtype=torch.int32, device=DEV), lowptr=torch.zeros(N + 1, dtype=torch.int32, device=DEV))
    calls = (lambda: lib().nq_graph_count(P(posd), P(mol_ptr), N, 1, N, 1.0, 100, P(cnt["deg"]), P(cnt["lowdeg"]), P(cnt["row_ptr"]), P(cnt["lowptr"]),
                                          C.byref(e_host), st()),
             lambda: call_fill(posd, mol_ptr, N, 1, 0, N, 1.0, 100, zeros, out))
    for call in calls:
        rejected(call, out["geom"], out["edge_dist"], out["edge_vector"])
        assert call() == L.NQ_ERR_MOL_TOO_LARGE
        assert e_host.value == GARBAGE and (out["neighbors"] == GARBAGE).all() and (out["atom_mol"] == -1).all()
        for k in COUNT_OUT:
            assert (cnt[k] == GARBAGE).all(), k
        for k in SLOT_OUT + ("edge_index", "id_swap"):
            assert (out[k] == -1).all(), k
    with pytest.raises(L.NablaqError) as e:
        build_neighbor_list(posd, torch.zeros(N, dtype=torch.long, device=DEV), None, 1.0, 100, canonical=True)
    assert e.value.code == L.NQ_ERR_MOL_TOO_LARGE
    nl = build_neighbor_list(posd[:512], torch.zeros(512, dtype=torch.long, device=DEV), None, 1.0, 100, canonical=True)    # 512 of them are taken
    assert nl.E == 0 and int(nl.neighbors[0]) == 0 and not nl.t["atom_mol"].any()
