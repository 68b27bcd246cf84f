"""Keeps the references of the Clebsch-Gordan operator tests honest (tests/cg_ref.py): the two halves of NormGate against oracle/qhnet_ref.norm_gate, the
two-piece bfloat16 mirror of the fused generator against the exact product with a derived bound, the conventions that are choices, and the Python
mirrors of the host-side launch rules (so3_rows_per_block after the F = 1 fix; the LDS sizes of the expansion launchers)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import qhnet_ref as Q  # noqa: E402
from tests import cg_ref as G  # noqa: E402


def test_gate_of_normcat_is_norm_gate():
    gen = torch.Generator().manual_seed(0)
    rows, C = 13, 6
    x = torch.randn(rows, 25, C, generator=gen, dtype=torch.float64)
    x[3, 4:9] = 0.0                                                              # an all-zero l = 2 block
    P = {"g.fc.0.weight": torch.randn(7, 5 * C, generator=gen, dtype=torch.float64), "g.fc.0.bias": torch.randn(7, generator=gen, dtype=torch.float64),
         "g.fc.2.weight": torch.randn(5 * C, 7, generator=gen, dtype=torch.float64), "g.fc.2.bias": torch.randn(5 * C, generator=gen, dtype=torch.float64)}
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = G.gate_ref(xa, Q.mlp(P, "g.fc", G.normcat_ref(xa)))
    yb = Q.norm_gate(P, "g", xb)
    assert float((ya - yb).detach().abs().max()) <= 1e-12 * float(yb.detach().abs().max())
    w = torch.randn(rows, 25, C, generator=gen, dtype=torch.float64)
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    assert float((xa.grad - xb.grad).abs().max()) <= 1e-12 * float(xb.grad.abs().max())


def test_conventions_norm_gradient_at_zero_and_softplus_above_20():
    x = torch.zeros(2, 9, 3, dtype=torch.float64)
    x[1] = 1.0
    x.requires_grad_(True)
    f = G.normcat_ref(x)
    assert torch.equal(f[0, 3:], torch.zeros(6, dtype=torch.float64))
    f.sum().backward()
    assert torch.equal(x.grad[0, 1:], torch.zeros(8, 3, dtype=torch.float64))    # exactly 0, not NaN
    assert torch.equal(x.grad[0, 0], torch.ones(3, dtype=torch.float64))
    for dt in (torch.float64, torch.float32):
        hi = torch.tensor([20.0, 30.0, 88.0], dtype=dt)
        hi[0] = torch.nextafter(hi[0], torch.tensor(100.0, dtype=dt))
        assert torch.equal(G.act_ref(hi, 1, 1.0), hi - math.log(2.0))            # softplus(x) = x above 20
        at = torch.tensor([20.0], dtype=dt)
        assert torch.equal(G.act_ref(at, 1, 1.0), torch.log1p(torch.exp(at)) - math.log(2.0))
    assert abs(float(G.act_ref(torch.zeros(1, dtype=torch.float64), 1, 1.0))) < 1e-15      # shifted: ssp(0) = 0


def test_pair_reduce_ref_against_index_add():
    rng = np.random.default_rng(1)
    row_ptr = np.array([0, 2, 2, 3, 4])
    own, col = np.array([0, 0, 2, 3]), np.array([2, 3, 0, 0])
    rev = np.array([2, 3, 0, 1])
    a, b, base = (torch.tensor(rng.normal(size=s)) for s in ((4, 5), (4, 5), (4, 5)))
    out = G.pair_reduce_ref(a, b, base, row_ptr, rev, 4, 5, torch.float64)
    ref = base.clone().index_add_(0, torch.tensor(own), a).index_add_(0, torch.tensor(col), b)     # b[rev[r]] is the row owned by col[r] that points at n
    assert float((out - ref).abs().max()) < 1e-14
    assert torch.equal(G.pair_reduce_ref(a, None, None, row_ptr, rev, 4, 5, torch.float64)[1], torch.zeros(5, dtype=torch.float64))


@pytest.mark.parametrize("K", [32, 64, 128])
def test_split2_mirror_within_the_derived_bound(K):
    """A first bfloat16 piece is within 2^-9 of its value, two pieces within 2^-18 (relative); hi hi' + hi lo' + lo hi' drops lo lo' <= 2^-18 |h||W| and
    carries the two operands' two-piece errors: |mirror - exact| <= 3 * 2^-18 * (1 + 2^-7) * (|h| @ |W|), element by element.  Derived, not measured.
    (2^-9 and 2^-18 are relative to the top of a value's binade; for a single value at the bottom of its binade the pieces are within 2^-8 and 2^-16, which
    is what is asserted per element below.  The bound on the product is the one above.)"""
    rng = np.random.default_rng(K)
    h = rng.standard_normal((70, K)).astype(np.float32)
    W = rng.standard_normal((K, 1040)).astype(np.float32)
    hi, lo = G.split2(h)
    assert (np.abs(h - hi) <= 2.0 ** -8 * np.abs(h)).all() and (np.abs(h.astype(np.float64) - hi - lo) <= 2.0 ** -16 * np.abs(h)).all()
    exact = h.astype(np.float64) @ W.astype(np.float64)
    mirror = G.split2_mirror(h, W)
    bound = 3 * 2.0 ** -18 * (1 + 2.0 ** -7) * (np.abs(h).astype(np.float64) @ np.abs(W).astype(np.float64))
    ratio = float((np.abs(mirror - exact) / bound).max())
    print(f"split2_mirror K={K}: max |mirror - exact| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert float(np.abs(mirror - exact).max()) > 0.0                             # the mirror is not the exact product in disguise


def test_so3_rows_per_block_mirror():
    for F in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        for rows in (1, 255, 1024, 10 ** 5, 10 ** 7):
            k = G.so3_rows_per_block(rows, F)
            assert k > 0 and k % (256 // F) == 0, (rows, F, k)
            assert k <= max(128, 256 // F)
            nb = G.so3_partial_blocks(rows, F)
            assert (nb - 1) * k < rows <= nb * k
    assert G.so3_rows_per_block(300, 1) == 256                                   # one pass of 256 rows, above the 128-row cap
    assert G.so3_rows_per_block(140000, 32) == 128 and G.so3_rows_per_block(4099, 64) == 8
    assert G.so3_partial_blocks(10, 48) == 0 and G.so3_partial_blocks(0, 32) == 0


def test_expansion_lds_mirrors():
    # the def2-SVP layout of the model (5 s, 4 p, 3 d shells, 32 bottleneck channels): 8320 weights per row, the "33 kB" of the kernel comment
    nw, nb, S, res, combos = G.expansion_layout((5, 4, 3), 32)
    assert (nw, nb, S, res, combos) == (8320, 50, 32, 32 * 32, 144)
    assert G.expansion_lds_forward((5, 4, 3), 32) == 4 * (8320 + 800 + 50 + 4)
    assert G.expansion_lds_backward((5, 4, 3), 32) == 4 * (8320 + 800 + 1024 + 1024 + 4)
    assert G.expansion_layout((1, 1, 1), 4)[:2] == (19 * 4, 3) and len(G.EXP_INSTRUCTIONS) == 19
    assert G.expansion_lds_forward((8, 6, 4), 32) > 64 * 1024 and G.expansion_lds_backward((8, 6, 4), 32) > 64 * 1024
    assert G.expansion_layout((8, 6, 4), 32)[4] > 256
