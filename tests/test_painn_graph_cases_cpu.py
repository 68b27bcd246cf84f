"""The batches of tests/painn_graph_cases.py must keep the properties the GPU tests of csrc/graph.hip rely on (test_painn_graph_ops_gpu.py): asserted here
on the CPU oracle alone (oracle/painn_ref.py: build_graph, edge_geometry, both pinned bit-exactly to the real reference by tests/test_oracle_golden.py),
so that a later edit of a seed or a size cannot silently turn a case into an easy one.  If one of these fails, change the batch, not the assertion.
The CSR tables the GPU test compares the kernels with (painn_graph_cases.tables) are held to the engine's invariants here too."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import painn_ref as R  # noqa: E402
from tests import painn_graph_cases as GC  # noqa: E402


def word_counts(name):
    """[N, words] number of kept lower neighbours (source < target) of every atom per 64-bit adjacency word of its molecule."""
    pos, sizes, _, _ = GC.case(name)
    T = GC.tables(name)
    start = GC.ptr_of(sizes)[T["atom_mol"]]
    src, dst = T["edge_index"]
    lo = src < dst
    out = np.zeros((T["N"], (max(sizes) + 63) // 64), dtype=np.int64)
    np.add.at(out, (dst[lo], (src[lo] - start[dst[lo]]) // 64), 1)
    return out


def lower_sources(T, atom):
    src, dst = T["edge_index"]
    return np.sort(src[(dst == atom) & (src < dst)])


def ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", GC.CASES + ["empty-none"])
def test_tables_hold_the_engine_invariants(name):
    """rev an involution that flips (col, dst), rows sorted by source, slot2canon a permutation onto the oracle's list; the IEEE float32 geometry within
    1 / 2 ulp of the oracle's (torch's vectorised sqrt is only faithful) and the oracle's isclose mask the same set as ``d <= 1e-6``."""
    pos, sizes, cutoff, K = GC.case(name)
    T = GC.tables(name)
    GC.check_invariants(T)
    assert T["N"] == len(pos) == sum(sizes) and T["B"] == len(sizes) and max(sizes) <= GC.NQ_MAX_MOL_ATOMS
    assert np.array_equal(T["atom_mol"], np.repeat(np.arange(len(sizes)), sizes))
    p = torch.tensor(pos)
    d, v = R.edge_geometry(p, torch.tensor(T["edge_index"]))
    assert ulps(T["edge_dist"], d.numpy()).max(initial=0) <= 1
    big = T["edge_dist"] > 1e-6
    assert ulps(T["edge_vector"][big], v.numpy()[big]).max(initial=0) <= 2
    assert np.array_equal(torch.isclose(d, torch.zeros(()), atol=1e-6).numpy(), ~big)
    for g, n in enumerate(sizes):                                    # neighbors[g] = canonical edges of molecule g
        assert T["neighbors"][g] == int((T["atom_mol"][T["edge_index"][1]] == g).sum())
        assert n > 0 or T["neighbors"][g] == 0


@pytest.mark.parametrize("K", GC.COMPLETE_K)
def test_complete130(K):
    name = f"complete130-K{K}"
    pos, sizes, cutoff, _ = GC.case(name)
    T = GC.tables(name)
    d2 = ((pos[:, None, :].astype(np.float64) - pos[None, :, :]) ** 2).sum(-1)
    assert sizes == [130] and d2.max() < 3.0 < cutoff ** 2            # a unit cube: every pair inside
    i = np.arange(130)
    assert np.array_equal(T["lowdeg"], np.minimum(i, K))
    assert T["E"] == GC.COMPLETE_E[K] == 2 * int(np.minimum(i, K).sum())
    assert T["deg"].max() == 129 and (T["deg"] > 64).any()           # rows of the symmetric list longer than one word
    for a in (1, 63, 64, 65, 66, 70, 71, 100, 101, 129):              # the kept ones are the LOWEST min(i, K) indices
        assert np.array_equal(lower_sources(T, a), np.arange(min(a, K))), a
    w = word_counts(name)
    assert w.shape == (130, 3)
    if K == 1:
        assert (w[1:, 0] == 1).all() and (w[:, 1:] == 0).all()       # cut inside the first word
    if K == 64:
        assert (w[64:, 0] == 64).all() and (w[:, 1:] == 0).all()     # the whole second (and third) word trimmed
    if K in (65, 70):
        assert (w[K:, 1] == K - 64).all() and (w[:, 2] == 0).all()   # cut inside the second word
    if K == 100:
        assert (w[128:, 1] == 36).all() and (w[:, 2] == 0).all()


def test_words():
    pos, sizes, cutoff, _ = GC.case("words-K100")
    assert sizes == [63, 64, 65, 128, 129, 192, 193] and cutoff == 4.0
    full, kept = word_counts("words-K100"), word_counts("words-K5")
    T5, T100 = GC.tables("words-K5"), GC.tables("words-K100")
    print(f"words: E {T5['E']} / {T100['E']}  largest degree {T5['deg'].max()} / {T100['deg'].max()}  largest lower degree {T100['lowdeg'].max()}")
    assert T100["lowdeg"].max() < 100                                 # K = 100: the cutoff alone selects
    assert full.shape[1] == 4 and (full.sum(0)[:3] > 0).all()        # lower neighbours in three adjacency words ...
    assert T100["lowdeg"][-1] > 0                                     # ... and the 193rd atom is the one bit of the fourth word of the symmetric rows
    assert T100["deg"].max() > 64
    assert np.array_equal(T5["lowdeg"], np.minimum(T100["lowdeg"], 5)) and (T100["lowdeg"] > 5).any() and (T100["lowdeg"] < 5).any()
    assert ((kept[:, 1:] > 0) & (kept[:, 1:] < full[:, 1:])).any()   # K = 5 cuts inside a later word,
    assert ((kept[:, 1:] == 0) & (full[:, 1:] > 0)).any()            # drops whole later words
    assert ((kept[:, 0] > 0) & (kept[:, 0] < full[:, 0])).any()      # and cuts inside the first
    a = int(np.argmax(T100["lowdeg"]))                                # the kept ones are the lowest indices
    assert np.array_equal(lower_sources(T5, a), lower_sources(T100, a)[:5])


def test_limit512():
    pos, sizes, cutoff, K = GC.case("limit512")
    T = GC.tables("limit512")
    W = (512 + 63) // 64
    assert sizes == [512] == [GC.NQ_MAX_MOL_ATOMS] and 512 * W * 8 * 2 + 512 * 3 * 4 == 71680 > 64 * 1024      # the opt-in dynamic-LDS launch
    print(f"limit512: E {T['E']}  largest degree {T['deg'].max()}  largest lower degree {T['lowdeg'].max()}")
    assert (T["E"], int(T["deg"].max())) == GC.LIMIT_E_DEG
    assert T["lowdeg"].max() < K and T["deg"].min() > 0
    w = word_counts("limit512")
    assert w.shape == (512, 8) and (w.sum(0) > 0).all()              # bits in all eight words
    O = GC.tables("limit512-offset")
    assert GC.case("limit512-offset")[1] == [3, 512] and O["E"] == T["E"] + 6 and list(O["neighbors"]) == [6, T["E"]]
    assert np.array_equal(O["edge_index"][:, 6:], T["edge_index"] + 3) and np.array_equal(O["lowptr"][3:], T["lowptr"] + 3)
    assert np.array_equal(O["geom"][O["row_ptr"][3]:].view(np.int32), T["geom"].view(np.int32))


def test_at_cutoff():
    pos, sizes, cutoff, K = GC.case("at_cutoff")
    T = GC.tables("at_cutoff")
    r2 = np.float32(cutoff) * np.float32(cutoff)
    w = pos[1] - pos[0]
    assert np.float32(np.float32(w[0] * w[0]) + np.float32(w[1] * w[1])) + np.float32(w[2] * w[2]) == r2 == 25.0     # d^2 == r^2 exactly: excluded (<)
    assert pos[2, 2] < 5.0 and np.float32(pos[2, 2] * pos[2, 2]) < r2                                               # one float32 ulp inside
    assert T["edge_index"].tolist() == [[0, 2], [2, 0]] and list(T["neighbors"]) == [2]
    assert T["edge_dist"].tolist() == [float(pos[2, 2])] * 2


def test_coincident():
    pos, sizes, cutoff, K = GC.case("coincident")
    T = GC.tables("coincident")
    assert T["E"] == 12                                               # all six pairs
    src, dst = T["edge_index"]
    d, v = T["edge_dist"], T["edge_vector"]
    gap = float(np.float32(3.0 + 5e-7) - np.float32(3.0))
    assert abs(gap - 4.77e-7) < 1e-9
    for e in range(12):
        pair = {int(src[e]), int(dst[e])}
        if pair == {0, 1}:
            assert d[e] == 0.0 and v[e].tolist() == [0.0, 0.0, 0.0]
        elif pair in ({0, 2}, {1, 2}):                                # vector = pos[src] - pos[dst]
            sign = 1.0 if src[e] == 2 else -1.0
            assert d[e] == np.float32(gap) and v[e, 0] == 0.0 and v[e, 1] == 0.0 and abs(v[e, 2] - sign * 0.32287729) < 1e-7
        else:
            assert d[e] > 0.49
    assert int((d <= 1e-6).sum()) == 6                                # the + 1e-6 branch, at d == 0 and at d > 0
    dt, vt = R.edge_geometry(torch.tensor(pos), torch.tensor(T["edge_index"]))
    assert np.array_equal(vt.numpy()[d <= 1e-6], v[d <= 1e-6])


def test_far_offset():
    pos, sizes, cutoff, K = GC.case("far_offset")
    near = GC.case("words-K100")[0]
    assert np.array_equal(pos, (near + GC.FAR_SHIFT).astype(np.float32)) and np.abs(pos).min() > 90.0
    T, T0 = GC.tables("far_offset"), GC.tables("words-K100")
    assert T["E"] > 20000 and T["deg"].max() > 64
    # the shift rounds the positions (ulp 7.6e-6 .. 3.1e-5): the geometry is that of the shifted float32 positions, not of the near ones
    if np.array_equal(T["edge_index"], T0["edge_index"]):
        assert (T["edge_dist"] != T0["edge_dist"]).mean() > 0.5


def test_empty_molecules():
    ref = GC.tables("empty-none")
    assert ref["E"] > 0 and (ref["neighbors"] > 0).all()
    for name, sizes in (("empty-ptr", [0, 5, 0, 0, 9, 30, 0]), ("empty-batch", [0, 5, 0, 9, 30])):
        assert GC.case(name)[1] == sizes and GC.needs_ptr(sizes) == (name == "empty-ptr")
        T = GC.tables(name)
        full = np.array(sizes) > 0
        assert (T["neighbors"][~full] == 0).all() and np.array_equal(T["neighbors"][full], ref["neighbors"])
        for k in ("edge_index", "id_swap", "row_ptr", "lowptr", "col", "dst", "rev", "slot2canon", "deg"):   # atoms keep their numbers
            assert np.array_equal(T[k], ref[k]), k
        assert np.array_equal(T["geom"].view(np.int32), ref["geom"].view(np.int32))
        assert np.array_equal(T["atom_mol"], np.nonzero(full)[0][ref["atom_mol"]])
    assert (ref["lowdeg"] == 4).any() and (ref["lowdeg"] < 4).any()  # K = 4 selects in the 30-atom molecule


def test_no_pairs():
    pos, sizes, cutoff, K = GC.case("no_pairs")
    T = GC.tables("no_pairs")
    assert sizes == [1, 1, 2, 1] and np.linalg.norm(pos[3] - pos[2]) > cutoff > np.linalg.norm(pos[1] - pos[0])    # close atoms, other molecules
    assert T["E"] == 0 and T["edge_index"].shape == (2, 0) and list(T["neighbors"]) == [0, 0, 0, 0]
    assert list(T["row_ptr"]) == [0] * 6 and list(T["lowptr"]) == [0] * 6 and T["geom"].shape == (0, 4)


@pytest.mark.parametrize("N", GC.SCAN_N)
def test_scan(N):
    pos, sizes, cutoff, K = GC.case(f"scan-N{N}")
    T = GC.tables(f"scan-N{N}")
    assert T["N"] == N == sum(sizes) and set(sizes) <= {7, 8} and cutoff == 2.0
    assert (N == 8192) == (set(sizes) == {8})
    trip = 1024 * 8                                                   # elements per trip of k_scan2
    assert {8191: N == trip - 1, 8192: N == trip, 8193: N == trip + 1, 16385: N == 2 * trip + 1}[N]
    assert np.array_equal(T["row_ptr"], GC.excl(T["deg"])) and np.array_equal(T["lowptr"], GC.excl(T["lowdeg"])) and len(T["row_ptr"]) == N + 1
    assert T["row_ptr"][N] == T["E"] == 2 * T["lowptr"][N] > 0
    assert T["deg"].max() == 7 and (T["deg"] == 0).any()             # full and empty rows
    if N > trip:                                                      # the carry into the second (third) trip and what the last element adds to it
        assert 0 < T["row_ptr"][trip] < T["row_ptr"][N] and T["deg"][N - 1] > 0 and T["lowdeg"][N - 1] > 0
    assert T["deg"][min(N, trip) - 1] > 0
