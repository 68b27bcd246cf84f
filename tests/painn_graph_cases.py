"""TEST INFRASTRUCTURE -- the batches of the PaiNN neighbour-list tests (csrc/graph.hip: k_graph_count, k_scan2, k_graph_fill) as seeded numpy
constructions, and what both sides share: test_painn_graph_cases_cpu.py asserts on the CPU oracle (oracle/painn_ref.py: build_graph, edge_geometry)
that every case still has the property it exists for, test_painn_graph_ops_gpu.py runs the kernels on the same inputs and compares with ``tables``.
A plain module (not a conftest): nothing here touches a GPU.

A case is (pos float32 [N, 3], sizes, cutoff, K); ``sizes`` may hold zeros (empty molecules).
  complete130-K{1,64,65,70,100}  130 atoms inside a unit cube, cutoff 5: every pair inside, atom i keeps min(i, K) lower neighbours; K = 64 trims the whole
                  second adjacency word, 65 and 70 cut inside it, 1 inside the first; rows of the symmetric list up to 129 entries
  words-K{5,100}  molecules of 63 / 64 / 65 / 128 / 129 / 192 / 193 atoms (either side of a 64-bit adjacency word), random clouds, cutoff 4
  limit512        one molecule of 512 atoms (the most the kernels take; 71,680 B of LDS), uniform(0, 12), cutoff 3, K = 100
  limit512-offset the same molecule behind a 3-atom one (atom offset 3)
  at_cutoff       one pair at d^2 == r^2 exactly (excluded: strict <) and one a float32 ulp inside
  coincident      distances 0 and 4.77e-7: the ``d <= 1e-6`` branch of the unit vector
  far_offset      the words geometry shifted by (100, -200, 300)
  empty-ptr       empty molecules first, in the middle and last (only ``ptr`` can say that); empty-batch: first and in the middle, through a skipped index
  no_pairs        single atoms and a 2-atom molecule farther apart than the cutoff: E = 0
  scan-N{8191,8192,8193,16385}   molecules of 8 and 7 atoms: k_scan2 one element short of a full trip, exactly one, one element into and one past two"""
import numpy as np
import torch

from oracle import painn_ref as R

NQ_MAX_MOL_ATOMS = 512
WORD_SIZES = [63, 64, 65, 128, 129, 192, 193]
FAR_SHIFT = np.array([100.0, -200.0, 300.0], dtype=np.float32)
LIMIT_SEED = 270                      # numpy RandomState (MT19937: a stable stream)
LIMIT_E_DEG = (12214, 43)             # canonical edges and largest degree of limit512 on the oracle


def _cloud(rng, n, side=None):
    """The random clouds of oracle/make_golden.py (graph-only cases)."""
    return rng.uniform(0, max(2.0, n ** (1 / 3) * 1.6) if side is None else side, size=(n, 3)).astype(np.float32)


def _clouds(seed, sizes):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.concatenate([_cloud(rng, n) for n in sizes]).astype(np.float32).reshape(-1, 3)


def _complete130():
    return np.random.Generator(np.random.PCG64(130)).uniform(0, 1, size=(130, 3)).astype(np.float32), [130]


def _limit512():
    return np.random.RandomState(LIMIT_SEED).uniform(0, 12, size=(512, 3)).astype(np.float32)


def _scan(N):
    k7 = next(k for k in range(8) if (N - 7 * k) % 8 == 0)
    sizes = [8] * ((N - 7 * k7) // 8)
    for k in range(k7):                                              # the 7-atom molecules spread over the batch
        sizes.insert((k * len(sizes)) // max(k7, 1), 7)
    assert sum(sizes) == N
    return np.random.Generator(np.random.PCG64(N)).uniform(0, 2.5, size=(N, 3)).astype(np.float32), sizes


AT_CUTOFF = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, np.nextafter(np.float32(5.0), np.float32(0.0))]], dtype=np.float32)
COINCIDENT = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0 + 5e-7], [1.5, 2.0, 3.0]], dtype=np.float32)
EMPTY_PARTS = [5, 9, 30]                                              # the non-empty molecules of the empty_* cases


def _build(name):
    if name.startswith("complete130-K"):
        pos, sizes = _complete130()
        return pos, sizes, 5.0, int(name[len("complete130-K"):])
    if name.startswith("words-K"):
        return _clouds(7, WORD_SIZES), list(WORD_SIZES), 4.0, int(name[len("words-K"):])
    if name == "limit512":
        return _limit512(), [512], 3.0, 100
    if name == "limit512-offset":
        return np.concatenate([np.array([[0, 0, 0], [1, 0, 0], [0, 1.5, 0]], dtype=np.float32), _limit512()]), [3, 512], 3.0, 100
    if name == "at_cutoff":
        return AT_CUTOFF.copy(), [3], 5.0, 100
    if name == "coincident":
        return COINCIDENT.copy(), [4], 2.0, 100
    if name == "far_offset":
        return (_clouds(7, WORD_SIZES) + FAR_SHIFT).astype(np.float32), list(WORD_SIZES), 4.0, 100
    if name == "empty-none":                                          # what the two empty_* cases must reduce to
        return _clouds(11, EMPTY_PARTS), list(EMPTY_PARTS), 2.0, 4
    if name == "empty-ptr":
        return _clouds(11, EMPTY_PARTS), [0, 5, 0, 0, 9, 30, 0], 2.0, 4
    if name == "empty-batch":
        return _clouds(11, EMPTY_PARTS), [0, 5, 0, 9, 30], 2.0, 4
    if name == "no_pairs":
        pos = np.array([[0, 0, 0], [0.1, 0, 0], [5, 5, 5], [5, 5, 6.5], [9, 0, 0]], dtype=np.float32)
        return pos, [1, 1, 2, 1], 1.25, 100
    if name.startswith("scan-N"):
        pos, sizes = _scan(int(name[len("scan-N"):]))
        return pos, sizes, 2.0, 100
    raise KeyError(name)


COMPLETE_K = (1, 64, 65, 70, 100)
COMPLETE_E = {1: 258, 64: 12480, 65: 12610, 70: 13230, 100: 15900}
SCAN_N = (8191, 8192, 8193, 16385)
CASES = ([f"complete130-K{k}" for k in COMPLETE_K] + ["words-K5", "words-K100", "limit512", "limit512-offset", "at_cutoff", "coincident", "far_offset",
                                                       "empty-ptr", "empty-batch", "no_pairs"] + [f"scan-N{n}" for n in SCAN_N])
_CASE, _TABLES = {}, {}


def case(name):
    """(pos float32 [N, 3], sizes, cutoff, K); built once."""
    if name not in _CASE:
        pos, sizes, cutoff, K = _build(name)
        assert pos.dtype == np.float32 and pos.shape == (sum(sizes), 3)
        pos.setflags(write=False)
        _CASE[name] = (pos, sizes, cutoff, K)
    return _CASE[name]


def batch_of(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def needs_ptr(sizes):
    """A trailing empty molecule cannot be said through ``batch``."""
    return sizes[-1] == 0


def excl(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def ieee_geometry(pos, edge_index):
    """edge_dist / edge_vector of the reference formulas evaluated in IEEE float32 by numpy, one correctly rounded operation at a time:
    ((dx^2 + dy^2) + dz^2), sqrt, + 1e-6 where d <= 1e-6, division (tests/test_engine_gpu.py: _ieee_geometry)."""
    p = np.asarray(pos, np.float32)
    j, i = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    w = (p[i] - p[j]).astype(np.float32)
    d2 = ((w[:, 0] * w[:, 0]).astype(np.float32) + (w[:, 1] * w[:, 1]).astype(np.float32)).astype(np.float32)
    d2 = (d2 + (w[:, 2] * w[:, 2]).astype(np.float32)).astype(np.float32)
    d = np.sqrt(d2).astype(np.float32)
    den = (d + np.where(d <= 1e-6, np.float32(1e-6), np.float32(0))).astype(np.float32)
    v = ((p[j] - p[i]).astype(np.float32) / den[:, None]).astype(np.float32)
    return d, v


def tables(name):
    """Everything build_neighbor_list returns for the case, from the oracle's canonical edge list: edge_index / neighbors / id_swap as the oracle gives
    them (neighbors padded with the trailing empty molecules), the IEEE geometry, and the CSR by target atom the engine consumes (header of
    csrc/graph.hip): slots ordered by (target, source), ``rev`` the slot of the flipped edge, ``slot2canon`` the canonical position of a slot,
    ``lowptr`` the exclusive sums of the number of kept lower neighbours (source < target), ``geom`` = unit vector | distance per slot."""
    if name in _TABLES:
        return _TABLES[name]
    pos, sizes, cutoff, K = case(name)
    N, B = len(pos), len(sizes)
    batch = batch_of(sizes)
    ei, nb, swap = R.build_graph(torch.tensor(pos), torch.tensor(batch), cutoff, K)
    ei, nb, swap = ei.numpy(), nb.numpy(), swap.numpy()
    nb = np.concatenate([nb, np.zeros(B - len(nb), dtype=np.int64)])
    src, dst = ei
    E = len(src)
    order = np.lexsort((src, dst))                                   # by target, then source
    col, tgt = src[order], dst[order]
    deg = np.bincount(dst, minlength=N).astype(np.int64)
    low = np.bincount(dst[src < dst], minlength=N).astype(np.int64)
    rev = np.searchsorted(tgt * N + col, col * N + tgt)
    d, v = ieee_geometry(pos, ei)
    T = dict(N=N, B=B, E=E, edge_index=ei, neighbors=nb, id_swap=swap, edge_dist=d, edge_vector=v, deg=deg, lowdeg=low, row_ptr=excl(deg), lowptr=excl(low),
             col=col, dst=tgt, rev=rev, slot2canon=order.astype(np.int64), atom_mol=batch,
             geom=np.concatenate([v[order], d[order, None]], axis=1).astype(np.float32).reshape(E, 4))
    _TABLES[name] = T
    return T


def check_invariants(T):
    """The CSR invariants of tests/test_engine_gpu.py (test_graph_cases_bit_exact) on a set of tables, the restatement's or the device's."""
    col, dst, rev, rp, s2c, E, N = T["col"], T["dst"], T["rev"], T["row_ptr"], T["slot2canon"], T["E"], T["N"]
    assert np.array_equal(rev[rev], np.arange(E)) and np.array_equal(col[rev], dst) and np.array_equal(dst[rev], col)
    assert np.array_equal(np.repeat(np.arange(N), np.diff(rp)), dst) and rp[-1] == E
    same = dst[1:] == dst[:-1]
    assert (col[1:][same] > col[:-1][same]).all()
    assert np.array_equal(T["edge_index"][0][s2c], col) and np.array_equal(T["edge_index"][1][s2c], dst)
    assert np.array_equal(np.sort(s2c), np.arange(E))
    assert T["lowptr"][-1] * 2 == E and int(T["neighbors"].sum()) == E
