"""The batches of tests/gemnet_graph_cases.py must keep the properties the GPU tests of csrc/gemnet_graph.hip rely on (test_gemnet_graph_ops_gpu.py):
asserted here on the CPU oracle (oracle/gemnet_ref.py: build_graphs), so that a later edit of a seed or a size cannot silently turn a case into an easy
one.  If one of these fails, change the batch, not the assertion.  The numpy restatement the GPU test compares the kernels with (gemnet_graph_cases.tables)
is held against the oracle's edge lists here too, on the oracle's own distances."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gemnet_ref as R  # noqa: E402
from tests import gemnet_graph_cases as GC  # noqa: E402

_ORACLE = {}


class Case:
    pass


def oracle(bname, cname):
    key = (bname, cname)
    if key in _ORACLE:
        return _ORACLE[key]
    pos, sizes, named = GC.batch(bname)
    c = Case()
    c.pos, c.sizes, c.named, c.cfg, c.N = pos, sizes, named, GC.CONFIGS[cname], len(pos)
    c.G = R.build_graphs(torch.tensor(pos), sizes, c.cfg)
    c.src, c.dst = c.G["a2a"]
    c.row_ptr = GC.excl(np.bincount(c.dst, minlength=c.N))
    p = torch.tensor(pos)
    c.dist = (p[c.src] - p[c.dst]).norm(dim=-1).numpy()
    c.pos_in_row = np.arange(len(c.src)) - c.row_ptr[c.dst]
    c.rev = np.searchsorted(c.dst * c.N + c.src, c.src * c.N + c.dst)
    c.T = GC.tables(c.src, c.dst, c.row_ptr, c.rev, c.dist, c.cfg)
    _ORACLE[key] = c
    return c


def kept_positions(c, name):
    """Row positions (inside the a2a row of the target) of the edges the sub-graph ``name`` keeps."""
    return c.pos_in_row[c.T["keep"][name]]


def inside(c, name, cutoff):
    return GC.row_sum(c.dist <= np.float32(c.cfg[cutoff]), c.row_ptr)


@pytest.mark.parametrize("bname,cname", GC.CASES)
def test_restatement_equals_oracle(bname, cname):
    """radius_graph / select / tables of gemnet_graph_cases.py (what the GPU test compares the kernels with) against the oracle's edge lists."""
    c = oracle(bname, cname)
    src, dst, row_ptr = GC.radius_graph(c.pos, c.sizes, c.cfg["cutoff_aint"])
    assert np.array_equal(src, c.src) and np.array_equal(dst, c.dst) and np.array_equal(row_ptr, c.row_ptr)
    assert np.array_equal(c.src[c.rev], c.dst) and np.array_equal(c.dst[c.rev], c.src)
    T = c.T
    assert np.array_equal(np.stack([T["a_src"], T["a_dst"]]), np.stack(c.G["a2ee2a"]))
    assert np.array_equal(np.stack([T["q_src"], T["q_dst"]]), np.stack(c.G["qint"]))
    ms, md = c.G["main"]                                             # the oracle's main graph is in the reference's order: compare as sets of pairs
    assert len(ms) == len(T["m_src"]) == T["totals"][0]
    assert np.array_equal(np.sort(ms * c.N + md), np.sort(T["m_src"] * c.N + T["m_dst"]))
    assert np.array_equal(T["m_dst"] * c.N + T["m_src"], np.sort(T["m_dst"] * c.N + T["m_src"]))       # CSR by target, sources ascending
    assert T["totals"][3] == int(T["degm"][T["q_src"]].sum()) == len(T["tin_main"])


def test_chunks_caps():
    c = oracle("chunks", "caps")
    T = c.T
    deg_a2a = np.diff(c.row_ptr)
    pa, pq = kept_positions(c, "a2ee2a"), kept_positions(c, "qint")
    member_pos = c.pos_in_row[T["m_slot"]]
    empty_q = int((T["cnt_q"] == 0).sum())
    print(f"chunks x caps: N {c.N}  a2a in-degree max {deg_a2a.max()}, {int((deg_a2a > 64).sum())} rows > 64 | main rows max {T['degm'].max()}, "
          f"{int((T['degm'] > 64).sum())} rows > 64, members at position >= 64 / 128: {int((member_pos >= 64).sum())} / {int((member_pos >= 128).sum())} | "
          f"a2ee2a kept at position >= 64 / 128: {int((pa >= 64).sum())} / {int((pa >= 128).sum())} | qint: {int((pq >= 64).sum())} / {int((pq >= 128).sum())} | "
          f"empty qint rows {empty_q}")
    assert c.N > 1024                                                # k_gn_scan: a second 1024-thread pass
    assert deg_a2a.max() > 128 and (deg_a2a > 64).any() and (deg_a2a == 64).any() and (deg_a2a == 63).any()     # 1, exactly 1, 2 and 3 chunks
    assert T["degm"].max() > 64                                      # main rows longer than a wavefront (the tin_main loop, j += 64)
    assert (member_pos >= 64).any() and (member_pos >= 128).any()    # om carried into the second and third chunk
    assert (pa >= 64).any() and (pa >= 128).any()                    # oa ...
    assert (pq >= 64).any() and (pq >= 128).any()                    # oq ...
    # both the cutoff and the cap select: rows cut by K and rows cut by the cutoff alone, in every sub-graph
    for name, cut, k in GC.SUBGRAPHS:
        n_in, kept = inside(c, name, cut), GC.row_sum(T["keep"][name], c.row_ptr)
        assert (n_in > c.cfg[k]).any() and ((n_in < c.cfg[k]) & (n_in > 0)).any() and (n_in < deg_a2a).any(), name
        assert np.array_equal(kept, np.minimum(n_in, c.cfg[k])), name
    assert empty_q == 1
    GC.assert_named_chunks("caps", c.named, c.G["qint"], c.N)
    a = c.named["cutoff"]
    d = {int(s): float(x) for s, x in zip(c.src[c.dst == a], c.dist[c.dst == a])}
    assert d[a + 1] == 3.0 and d[a + 2] == float(np.nextafter(np.float32(3.0), np.float32(4.0))) and d[a + 3] == 1.0
    t = c.named["tie"]
    assert set(c.dist[c.dst == t].tolist()) == {1.5} and int((c.dst == t).sum()) == 6


def test_chunks_yaml():
    """All three caps bind on the 130-atom molecule: every atom has its 129 neighbours inside the cutoffs and keeps exactly K of them."""
    c = oracle("chunks", "yaml")
    big = slice(c.named["big"], c.named["big"] + c.named["big_n"])
    assert (np.diff(c.row_ptr)[big] == 129).all()
    for name, cut, k in GC.SUBGRAPHS:
        assert (inside(c, name, cut)[big] == 129).all() and (GC.row_sum(c.T["keep"][name], c.row_ptr)[big] == c.cfg[k]).all(), name
    assert (kept_positions(c, "qint") >= 64).any() and (kept_positions(c, "a2ee2a") >= 128).any()
    assert c.T["degm"][big].max() > 30                               # the flips lengthen main rows past the cap


def test_chunks_k1():
    """K = 1: every non-empty selected row has one entry; the main rows still exceed 1 through the flips."""
    c = oracle("chunks", "k1")
    for name, cut, k in GC.SUBGRAPHS:
        kept = GC.row_sum(c.T["keep"][name], c.row_ptr)
        assert np.array_equal(kept, np.minimum(inside(c, name, cut), 1)) and (kept == 1).any(), name
    assert c.T["degm"].max() > 1 and c.T["lowm"].max() == 1
    assert (kept_positions(c, "main") >= 64).any()                   # the nearest neighbour sits in the second chunk of some row
    GC.assert_named_chunks("k1", c.named, c.G["qint"], c.N)


def test_chunks_nocap():
    """K = 1 << 20: the selected row length equals the number of neighbours inside the cutoff."""
    c = oracle("chunks", "nocap")
    for name, cut, k in GC.SUBGRAPHS:
        n_in = inside(c, name, cut)
        assert np.array_equal(GC.row_sum(c.T["keep"][name], c.row_ptr), n_in) and n_in.max() > 64, name
        assert np.array_equal(c.T["keep"][name], c.dist <= np.float32(c.cfg[cut])), name
    GC.assert_named_chunks("nocap", c.named, c.G["qint"], c.N)


def test_largest_yaml():
    c = oracle("largest", "yaml")
    T = c.T
    print(f"largest x yaml: a2a in-degree max {np.diff(c.row_ptr).max()}  main in-degree max {T['degm'].max()}  Tin {T['totals'][3]}")
    GC.assert_named_largest(c.named, c.G["a2a"], c.N)
    assert np.diff(c.row_ptr).max() == 511                           # GN_MAXDEG - 1: eight chunks, the last one short by one lane
    assert T["degm"].max() > 30                                      # the flips
    for name in ("main", "a2ee2a", "qint"):
        assert (kept_positions(c, name) >= 448).any(), name           # a kept edge in the eighth chunk
    assert T["totals"][3] > T["totals"][2]                           # the (qint edge, main in-edge of its source) table has rows
