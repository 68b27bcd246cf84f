"""TEST INFRASTRUCTURE -- the batches and configurations of the GemNet-OC graph-kernel tests (csrc/gemnet_graph.hip) as seeded numpy constructions, and
the numpy restatements both sides share: test_gemnet_graph_cases_cpu.py asserts on the CPU oracle that every case still has the property it exists for,
test_gemnet_graph_ops_gpu.py runs the kernels on the same inputs.  A plain module (not a conftest): nothing here touches a GPU.

Batches
  chunks   1110 atoms (k_gn_scan carries across its 1024-thread passes): a 2-atom molecule, the *cutoff* molecule (one pair at exactly 3.0 = cutoff_qint of
           "caps", one pair one float32 ulp outside it), the *tie* molecule (six atoms at exactly 1.5 from the centre), molecules of 70 / 130 / 64 / 65 atoms
           (a2a rows of 63, 64, 69 and 129 entries: one, exactly one, two and three 64-lane chunks) and twelve of 64 atoms;
  largest  one molecule of 512 atoms inside a box whose diagonal is below cutoff_aint = 12 (every a2a row has 511 entries: eight chunks, sd[GN_MAXDEG] full
           but for one entry) and a 3-atom molecule whose last atom has no a2a neighbour.
Configurations (max_neighbors_aint = 1000 throughout)
  caps     cutoffs 5 / 4 / 3 with K = 80 / 20 / 4: cutoff and cap both select, kept edges beyond row position 64 and 128;
  yaml     config/model/gemnet-oc.yaml: cutoffs 12, K = 30 / 20 / 8 -- only the cap selects in the big molecules;
  k1       the cutoffs of caps, K = 1;          nocap    the cutoffs of caps, K = 1 << 20: only the cutoff selects."""
import numpy as np


def _random_molecule(rng, n, side):
    return (rng.uniform(0.0, side, size=(n, 3)) + rng.normal(size=3) * 5.0).astype(np.float32)


CUTOFF_MOLECULE = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, float(np.nextafter(np.float32(3.0), np.float32(4.0))), 0.0], [0.0, 0.0, 1.0]],
                           dtype=np.float32)
TIE_MOLECULE = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [-1.5, 0.0, 0.0], [0.0, 1.5, 0.0], [0.0, -1.5, 0.0], [0.0, 0.0, 1.5], [0.0, 0.0, -1.5]],
                        dtype=np.float32)
CHUNKS_RANDOM = [(70, 3.2), (130, 3.6), (64, 3.0), (65, 3.0)] + [(64, 4.0)] * 12


def chunks():
    """(pos float32 [1110, 3], sizes, named) -- ``named``: first atom of the cutoff, tie and 130-atom molecules."""
    rng = np.random.default_rng(21)
    parts = [_random_molecule(rng, 2, 1.0), CUTOFF_MOLECULE, TIE_MOLECULE] + [_random_molecule(rng, n, side) for n, side in CHUNKS_RANDOM]
    sizes = [len(p) for p in parts]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    return np.concatenate(parts).astype(np.float32), sizes, dict(cutoff=int(starts[1]), tie=int(starts[2]), big=int(starts[4]), big_n=130)


def largest():
    """(pos float32 [515, 3], sizes, named) -- ``named``: the atom of the 3-atom molecule that has no a2a neighbour."""
    rng = np.random.default_rng(5)
    big = rng.uniform(0.0, 6.9, size=(512, 3)).astype(np.float32)
    small = np.array([[50.0, 0.0, 0.0], [51.0, 0.0, 0.0], [70.0, 0.0, 0.0]], dtype=np.float32)
    return np.concatenate([big, small]), [512, 3], dict(lonely=514)


BATCHES = {"chunks": chunks, "largest": largest}


def _cfg(cutoffs, ks, aint):
    return dict(cutoff=cutoffs[0], cutoff_aeaint=cutoffs[1], cutoff_qint=cutoffs[2], max_neighbors=ks[0], max_neighbors_aeaint=ks[1],
                max_neighbors_qint=ks[2], cutoff_aint=aint, max_neighbors_aint=1000)


CONFIGS = {
    "caps": _cfg((5.0, 4.0, 3.0), (80, 20, 4), 6.0),
    "yaml": _cfg((12.0, 12.0, 12.0), (30, 20, 8), 12.0),
    "k1": _cfg((5.0, 4.0, 3.0), (1, 1, 1), 6.0),
    "nocap": _cfg((5.0, 4.0, 3.0), (1 << 20,) * 3, 6.0),
}
CASES = [("chunks", "caps"), ("chunks", "yaml"), ("chunks", "k1"), ("chunks", "nocap"), ("largest", "yaml")]
SUBGRAPHS = (("main", "cutoff", "max_neighbors"), ("a2ee2a", "cutoff_aeaint", "max_neighbors_aeaint"), ("qint", "cutoff_qint", "max_neighbors_qint"))

_BATCH = {}


def batch(name):
    if name not in _BATCH:
        _BATCH[name] = BATCHES[name]()
    return _BATCH[name]


# ---- numpy restatements -------------------------------------------------------------------------------------------------------------------------
def radius_graph(pos, sizes, r):
    """Brute-force float32 radius graph per molecule: (source, target) kept iff source != target and (dx^2 + dy^2) + dz^2 < r^2, every operation rounded
    to float32 in that order; target ascending, sources ascending.  Returns (src, dst, row_ptr) int64."""
    pos = np.asarray(pos, dtype=np.float32)
    r2 = np.float32(r) * np.float32(r)
    src, dst = [], []
    a0 = 0
    for n in sizes:
        p = pos[a0:a0 + n]
        d = p[:, None, :] - p[None, :, :]                          # d[i, j] = pos[i] - pos[j] (the squares do not see the sign)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        ok = (d2 < r2) & ~np.eye(n, dtype=bool)
        i, j = np.nonzero(ok)                                       # row-major: target i ascending, source j ascending
        src.append(a0 + j); dst.append(a0 + i)
        a0 += n
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=len(pos)))]).astype(np.int64)
    return src, dst, row_ptr


def select(dist, dst, row_ptr, cutoff, K):
    """The strict rule of the reference's get_max_neighbors_mask (utils.py:452-500) on a CSR by target: an edge is kept iff its distance is <= cutoff and
    fewer than K edges of its row with distance <= cutoff precede it in (distance, row position) order.  All rows at once."""
    dist = np.asarray(dist, dtype=np.float32)
    E = len(dist)
    order = np.lexsort((np.arange(E), dist, dst))                   # by target, then distance, then position: every row stays one segment
    el = dist[order] <= np.float32(cutoff)
    c = np.cumsum(el) - el                                          # eligible edges before this one, over all rows
    before = c - c[row_ptr[dst[order]]]                             # ... inside its own row
    keep = np.zeros(E, dtype=bool)
    keep[order] = el & (before < K)
    return keep


def excl(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def row_sum(x, row_ptr):
    return np.add.reduceat(np.concatenate([x.astype(np.int64), [0]]), row_ptr[:-1]) * (np.diff(row_ptr) > 0)


def tables(col, dst, row_ptr, rev, dist, cfg):
    """Every array nq_gn_graph_count / nq_gn_graph_fill write except the geometry, from the a2a CSR, its distances and the configuration."""
    E = len(col)
    keep = {name: select(dist, dst, row_ptr, cfg[c], cfg[k]) for name, c, k in SUBGRAPHS}
    km, ka, kq = keep["main"], keep["a2ee2a"], keep["qint"]
    T = dict(flags=(km * 1 + ka * 2 + kq * 4).astype(np.uint8))
    member = np.where(col < dst, km, km[rev])                       # symmetrised main graph: the kept source < target edges and their flips
    T["cnt_a"], T["cnt_q"], T["degm"], T["lowm"] = (row_sum(x, row_ptr) for x in (ka, kq, member, member & (col < dst)))
    T["tin_atom"] = row_sum(np.where(kq, T["degm"][col], 0), row_ptr)
    for p, c in (("ptr_m", "degm"), ("lowptr_m", "lowm"), ("ptr_a", "cnt_a"), ("ptr_q", "cnt_q"), ("tin_aptr", "tin_atom")):
        T[p] = excl(T[c])
    T["totals"] = [int(T[p][-1]) for p in ("ptr_m", "ptr_a", "ptr_q", "tin_aptr")]
    for pre, mask, posname in (("m", member, "mpos"), ("a", ka, "apos"), ("q", kq, "qpos")):
        slot = np.nonzero(mask)[0]
        T[pre + "_slot"], T[pre + "_src"], T[pre + "_dst"] = slot, col[slot], dst[slot]
        T[posname] = np.full(E, -1, dtype=np.int64)
        T[posname][slot] = np.arange(len(slot))
    T["m_rev"] = T["mpos"][rev[T["m_slot"]]]
    T["a_of_rev"], T["q_of_rev"] = T["apos"][rev], T["qpos"][rev]
    n_in = T["degm"][T["q_src"]]                                    # rows of the (qint edge, main in-edge of its source) table
    T["tin_ptr"] = excl(n_in)
    q_of_row = np.repeat(np.arange(len(n_in)), n_in)
    T["tin_main"] = T["ptr_m"][T["q_src"][q_of_row]] + (np.arange(int(n_in.sum())) - T["tin_ptr"][q_of_row])
    T["keep"] = keep
    return T


# ---- what each case exists for: statements on edge lists (source, target), asserted on the CPU oracle and on the device result alike ----------------
def sources(edges, atom):
    src, dst = edges
    return sorted(int(s) for s in np.asarray(src)[np.asarray(dst) == atom])


def assert_named_chunks(cfg_name, named, qint, N):
    a, t = named["cutoff"], named["tie"]
    if cfg_name in ("caps", "nocap"):
        # atom 1 sits at exactly 3.0 = cutoff_qint from atom 0 (kept: <=), atom 2 one float32 ulp further (dropped), atom 3 at 1.0
        assert sources(qint, a) == [a + 1, a + 3]
        assert sources(qint, a + 2) == []                           # 3.0000002, sqrt(18), sqrt(10) away from the others: an empty qint row
    if cfg_name == "k1":
        assert sources(qint, a) == [a + 3]
    if cfg_name == "caps":
        assert sources(qint, t) == [t + 1, t + 2, t + 3, t + 4]     # six exact ties at 1.5, K = 4: the lower row positions win
        assert int((np.bincount(qint[1], minlength=N) == 0).sum()) == 1   # ... and the only one of the batch
    if cfg_name == "k1":
        assert sources(qint, t) == [t + 1]
    if cfg_name == "nocap":
        assert sources(qint, t) == [t + k for k in range(1, 7)]


def assert_named_largest(named, a2a, N):
    deg = np.bincount(a2a[1], minlength=N)
    assert deg[:512].min() == 511 and deg[:512].max() == 511       # the 512-atom limit: in-degree 511 everywhere
    lonely = named["lonely"]
    assert deg[lonely] == 0 and deg[lonely - 1] == 1 and deg[lonely - 2] == 1      # an empty a2a row inside a molecule that has an edge
