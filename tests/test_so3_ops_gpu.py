"""The SO(3) mixing kernels of csrc/so3.hip (PhiSNet PairMixing / SelfMixing) one by one through the C ABI against a float64 restatement that shares no
code with them: the reference's own Clebsch-Gordan table (tests/so3_helpers.FixtureCG, from tests/golden/phisnet_cg_l4.npz) contracted by einsum, with the
kernel's coefficients multiplied by cg.path_signs(FixtureCG(), paths) as nabladft_amd/so3.py does.  Adjoints come from torch.autograd on the float64
evaluation.  Every output buffer starts as NaN.

Bounds (the convention of test_escn_ops_gpu.py): every summing kernel within max(3 x the error of the same formula in float32 on the CPU, 2e-6) of the
float64 value AND below 1e-5, array-relative; every kernel runs twice with bitwise equal results; gathers and "same arithmetic" comparisons are bitwise.

Branches and the tests that reach them:
  k_so3_mix<false> / <true> component counts 1 / 9 / 25 on each side, F = 1 .. 200 (rows * F not a multiple of 256), all / half / one path enabled,
      coefficients per row and broadcast (stride 0), keep NULL and keep_orders 1 .. min(o1, oy) + 1, x1 == x2 as one buffer: test_mix
  k_so3_keep_grad: test_mix (keep given), test_backward_shared[F32-one-row-keep]
  k_so3_mix<true, true> one workgroup / ragged last workgroup / several passes per workgroup / the 128-row cap / F = 1 (one pass of 256 rows, above the
      cap: needs so3_rows_per_block never below one pass) / LDS slab above 64 kB (65 paths): test_backward_shared (each case asserts the block rule it names)
  host rule so3_rows_per_block / nq_so3_mix_partial_blocks against its Python mirror: test_partial_blocks_agree_with_the_mirror; F = 1 through
      so3.SelfMixing (forward, backward, parameter gradients): test_self_mixing_with_one_feature_trains
  argument checks: test_mix_rejects_bad_arguments, test_backward_shared_rejects_F_48"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

from nabladft_amd import cg  # noqa: E402
from tests import cg_ref as G  # noqa: E402
from tests.helpers import DEV, D, P, _release_copies, assert_sum, check, lib, nan_dev, rejected, rnd, st, twice  # noqa: E402,F401
from tests.so3_helpers import FixtureCG  # noqa: E402

_CG = {}


def table():
    if not _CG:
        _CG["t"] = FixtureCG()
    return _CG["t"]


def path_index(enabled):
    arr = (C.c_int8 * 65)(*([-1] * 65))
    for i, p in enumerate(enabled):
        arr[cg.ALL_PATHS.index(p)] = i
    return arr


def mix_ref(x1, x2, c, keep, enabled, oy, dt):
    """y_L[r, M, f] = sum_paths c[r, path, f] sum_{m1 m2} CG[m1, m2, M] x1_{l1}[r, m1, f] x2_{l2}[r, m2, f] (+ keep_L[r, f] x1_L[r, M, f]); c and keep per
    row ([rows, n, F]), CG the reference's table."""
    rows, F = x1.shape[0], x1.shape[-1]
    ys = [x1.new_zeros(rows, 2 * L + 1, F) for L in range(oy + 1)]
    for i, (l1, l2, L) in enumerate(enabled):
        t = table()(l1, l2, L).to(dt)
        ys[L] = ys[L] + c[:, i, None, :] * torch.einsum("abm,raf,rbf->rmf", t, x1[:, G.sl(l1)], x2[:, G.sl(l2)])
    if keep is not None:
        for L in range(keep.shape[1]):
            ys[L] = ys[L] + keep[:, L, None, :] * x1[:, G.sl(L)]
    return torch.cat(ys, dim=1)


def mix_refs(x1, x2, c_model, keep, enabled, oy, gy):
    """[(y, gx1, gx2, gc rows, gkeep rows)] in float64 and float32; c_model [rows or 1, n, F], keep [ko, F] or None: both expanded to per-row leaves."""
    rows = x1.shape[0]
    out = []
    for dt in (torch.float64, torch.float32):
        a, b = x1.to(dt).requires_grad_(True), x2.to(dt).requires_grad_(True)
        c = c_model.to(dt).expand(rows, -1, -1).clone().requires_grad_(True)
        k = None if keep is None else keep.to(dt)[None].expand(rows, -1, -1).clone().requires_grad_(True)
        y = mix_ref(a, b, c, k, enabled, oy, dt)
        (y * gy.to(dt)).sum().backward()
        out.append((y.detach(), a.grad, b.grad, c.grad, None if k is None else k.grad))
    return out


def select_paths(o1, o2, oy, which, seed):
    feasible = cg.paths(o1, o2, oy)
    rng = np.random.default_rng(seed)
    if which == "all" or len(feasible) == 1:
        return feasible
    if which == "half":
        keep = sorted(rng.choice(len(feasible), size=max(1, len(feasible) // 2), replace=False))
        return [feasible[i] for i in keep]
    return [feasible[int(rng.integers(len(feasible)))]]


ORDERS = [(0, 0, 0), (2, 2, 2), (2, 1, 4), (0, 4, 4), (4, 0, 2), (4, 4, 4)]
FS = [1, 32, 48, 128, 200]
ROWS = [1, 37, 1000]
WHICH = ["all", "half", "one"]


def mix_cases():
    """For every (orders, F): three sub-cases that rotate rows, the enabled paths, per-row / broadcast coefficients and the keep orders, so that every
    value of every axis occurs with every order triple and every F; 1000 rows with all 65 paths only up to F = 48 (CPU time of the reference)."""
    cases = []
    for io, (o1, o2, oy) in enumerate(ORDERS):
        for jf, F in enumerate(FS):
            for s in range(3):
                rows = ROWS[(s + io + jf) % 3]
                which = WHICH[(s + jf) % 3]
                if rows == 1000 and which == "all" and F > 48 and (o1, o2, oy) == (4, 4, 4):
                    which = "half"
                per_row = (s + io) % 2 == 0
                kmax = min(o1, oy) + 1
                keep_orders = 0 if s == 0 else 1 + (io + jf + s) % kmax
                same = o1 == o2 and s == 1
                cases.append((o1, o2, oy, F, rows, which, per_row, keep_orders, same))
    return cases


MIX_CASES = mix_cases()


def test_mix_cases_cover_every_axis():
    for o1, o2, oy in ORDERS:
        sub = [c for c in MIX_CASES if c[:3] == (o1, o2, oy)]
        assert {c[3] for c in sub} == set(FS) and {c[4] for c in sub} == set(ROWS) and {c[5] for c in sub} >= ({"all"} if len(cg.paths(o1, o2, oy)) == 1 else set(WHICH))
        assert {c[6] for c in sub} == {True, False}
        assert {c[7] for c in sub} == set(range(0, min(o1, oy) + 2)), (o1, o2, oy, {c[7] for c in sub})
    assert any(c[8] for c in MIX_CASES)


@pytest.mark.parametrize("o1,o2,oy,F,rows,which,per_row,keep_orders,same", MIX_CASES,
                         ids=[f"o{c[0]}{c[1]}{c[2]}-F{c[3]}-r{c[4]}-{c[5]}-{'rowc' if c[6] else 'bcast'}-k{c[7]}{'-same' if c[8] else ''}" for c in MIX_CASES])
def test_mix(o1, o2, oy, F, rows, which, per_row, keep_orders, same):
    n1, n2, ny = (o1 + 1) ** 2, (o2 + 1) ** 2, (oy + 1) ** 2
    enabled = select_paths(o1, o2, oy, which, o1 * 100 + o2 * 10 + oy + F)
    n_en = len(enabled)
    gen = torch.Generator().manual_seed(rows * 7 + F + n_en)
    x1 = rnd(gen, rows, n1, F)
    x2 = x1 if same else rnd(gen, rows, n2, F)
    c_model = rnd(gen, rows if per_row else 1, n_en, F)
    keep = rnd(gen, keep_orders, F) if keep_orders else None
    gy = rnd(gen, rows, ny, F)
    sign = torch.tensor(cg.path_signs(lambda a, b, c: table()(a, b, c).numpy(), enabled), dtype=torch.float32).view(1, -1, 1)
    c_k = (c_model * sign).contiguous()                                           # what so3.py hands to the kernel
    pidx = path_index(enabled)
    x1d = D(x1)
    x2d = x1d if same else D(x2)
    cd, kd, gyd = D(c_k), (D(keep) if keep is not None else None), D(gy)
    stride = n_en * F if per_row else 0

    def fwd():
        y = nan_dev(rows, ny, F)
        check(lib().nq_so3_mix_forward(x1d, x2d, cd, kd, rows, F, o1, o2, oy, pidx, stride, keep_orders, P(y), st()))
        return (y,)

    def bwd():
        gx1, gx2, gc = nan_dev(rows, n1, F), nan_dev(rows, n2, F), nan_dev(rows, n_en, F)
        gk = nan_dev(rows, max(keep_orders, 1), F)
        check(lib().nq_so3_mix_backward(x1d, x2d, cd, kd, gyd, rows, F, o1, o2, oy, pidx, stride, keep_orders, P(gx1), P(gx2), P(gc), P(gk) if keep_orders else None,
                                        st()))
        return gx1, gx2, gc, gk
    (y,) = twice(fwd)
    gx1, gx2, gc, gk = twice(bwd)
    r64, r32 = mix_refs(x1, x2, c_model, keep, enabled, oy, gy)
    assert_sum("so3 y", y, r64[0], r32[0])
    assert_sum("so3 grad_x1", gx1, r64[1], r32[1])
    assert_sum("so3 grad_x2", gx2, r64[2], r32[2])
    assert_sum("so3 grad_coeff", gc.cpu() * sign, r64[3], r32[3])                  # d/d c_model = sign * d/d c_kernel
    if keep_orders:
        assert_sum("so3 grad_keep", gk, r64[4], r32[4])
    else:
        assert torch.isnan(gk).all()


def test_mix_rejects_bad_arguments():
    rows, F = 3, 8
    x = torch.zeros(rows, 25, F, device=DEV)
    c = torch.zeros(rows, 65, F, device=DEV)
    pidx = path_index(cg.ALL_PATHS)
    for o1, o2, oy, f, pi in [(5, 0, 0, F, pidx), (0, 5, 0, F, pidx), (0, 0, 5, F, pidx), (4, 4, 4, 0, pidx), (4, 4, 4, F, None)]:
        y = nan_dev(rows, 36, F)
        rejected(lambda: lib().nq_so3_mix_forward(P(x), P(x), P(c), None, rows, f, o1, o2, oy, pi, 65 * F, 0, P(y), st()), y)
        gx1, gx2, gc = nan_dev(rows, 36, F), nan_dev(rows, 36, F), nan_dev(rows, 65, F)
        rejected(lambda: lib().nq_so3_mix_backward(P(x), P(x), P(c), None, P(x), rows, f, o1, o2, oy, pi, 65 * F, 0, P(gx1), P(gx2), P(gc), None, st()), gx1, gx2, gc)


# (name, F, rows, orders, paths, keep_orders, expected (rows per block, blocks), what the case is for)
SHARED_CASES = [
    ("F1-one-pass-of-256", 1, 300, (4, 4, 4), "all", 2, (256, 2)),               # needs the fix: 128 / 256 * 256 = 0 rows per block before it
    ("F1-one-workgroup", 1, 200, (2, 2, 2), "half", 0, (256, 1)),
    ("F2-one-workgroup", 2, 128, (2, 2, 2), "half", 0, (128, 1)),
    ("F32-cap-128", 32, 140000, (0, 0, 0), "all", 1, (128, 1094)),               # ceil(140000 / 1024) = 137 -> 144 > 128: capped, ragged last workgroup
    ("F64-two-passes-ragged", 64, 4099, (2, 1, 4), "half", 0, (8, 513)),          # 8 rows per block = two passes of 256 / 64
    ("F256-65-paths", 256, 37, (4, 4, 4), "all", 5, (1, 37)),
    ("F32-one-row-keep", 32, 1, (4, 4, 4), "all", 3, (8, 1)),
    ("F64-65-paths-ragged", 64, 1030, (4, 4, 4), "all", 0, (4, 258)),
]


@pytest.mark.parametrize("name,F,rows,orders,which,keep_orders,plan", SHARED_CASES, ids=[c[0] for c in SHARED_CASES])
def test_backward_shared(name, F, rows, orders, which, keep_orders, plan):
    o1, o2, oy = orders
    n1, n2, ny = (o1 + 1) ** 2, (o2 + 1) ** 2, (oy + 1) ** 2
    k, nblk = G.so3_rows_per_block(rows, F), G.so3_partial_blocks(rows, F)
    assert (k, nblk) == plan and int(lib().nq_so3_mix_partial_blocks(rows, F)) == nblk
    rpp = 256 // F
    if "one-workgroup" in name or "one-row" in name:
        assert nblk == 1
    if "ragged" in name or "cap" in name:
        assert nblk > 1 and rows % k != 0
    if "two-passes" in name:
        assert k == 2 * rpp
    if "cap" in name:
        assert k == 128 and (rows + 1023) // 1024 > 128
    enabled = select_paths(o1, o2, oy, which, F + rows)
    n_en = len(enabled)
    if "65-paths" in name or name.startswith("F1-one-pass"):
        assert n_en == 65 and 4 * rpp * n_en * F > 64 * 1024                        # LDS slab above 64 kB
    gen = torch.Generator().manual_seed(F * 3 + rows)
    x1, x2 = rnd(gen, rows, n1, F), rnd(gen, rows, n2, F)
    c_model = rnd(gen, 1, n_en, F)
    keep = rnd(gen, keep_orders, F) if keep_orders else None
    gy = rnd(gen, rows, ny, F)
    sign = torch.tensor(cg.path_signs(lambda a, b, c: table()(a, b, c).numpy(), enabled), dtype=torch.float32).view(1, -1, 1)
    c_k = (c_model * sign).contiguous()
    pidx = path_index(enabled)
    x1d, x2d, cd, kd, gyd = D(x1), D(x2), D(c_k), (D(keep) if keep is not None else None), D(gy)

    def shared():
        gx1, gx2, part = nan_dev(rows, n1, F), nan_dev(rows, n2, F), nan_dev(nblk, n_en, F)
        gk = nan_dev(rows, max(keep_orders, 1), F)
        check(lib().nq_so3_mix_backward_shared(x1d, x2d, cd, kd, gyd, rows, F, o1, o2, oy, pidx, keep_orders, P(gx1), P(gx2), P(part), P(gk) if keep_orders else None,
                                               st()))
        return gx1, gx2, part, gk
    gx1, gx2, part, gk = twice(shared)
    gx1r, gx2r, gcr = nan_dev(rows, n1, F), nan_dev(rows, n2, F), nan_dev(rows, n_en, F)
    check(lib().nq_so3_mix_backward(x1d, x2d, cd, kd, gyd, rows, F, o1, o2, oy, pidx, 0, keep_orders, P(gx1r), P(gx2r), P(gcr), None, st()))
    torch.cuda.synchronize()
    assert not torch.isnan(part).any()                                            # every partial row written
    assert torch.equal(gx1.view(torch.int32), gx1r.view(torch.int32)) and torch.equal(gx2.view(torch.int32), gx2r.view(torch.int32))
    r64, r32 = mix_refs(x1, x2, c_model, keep, enabled, oy, gy)
    assert_sum("so3 shared grad_x1", gx1, r64[1], r32[1])
    assert_sum("so3 shared grad_coeff", part.cpu().double().sum(0).float() * sign[0], r64[3].sum(0), r32[3].sum(0))
    if keep_orders:
        assert_sum("so3 shared grad_keep", gk, r64[4], r32[4])


def test_self_mixing_with_one_feature_trains():
    """The way the F = 1 case is reached in practice: so3.SelfMixing takes the shared-coefficient reverse kernel whenever 256 % F == 0; before the fix
    of so3_rows_per_block its backward divided by zero on the host."""
    from nabladft_amd import so3
    oi, oo, rows = 3, 2, 300
    m = so3.SelfMixing(oi, oo, 1, FixtureCG()).to(DEV)
    gen = torch.Generator().manual_seed(9)
    x = rnd(gen, rows, (oi + 1) ** 2, 1)
    gy = rnd(gen, rows, (oo + 1) ** 2, 1)
    xs = [x[:, G.sl(l)].to(DEV).requires_grad_(True) for l in range(oi + 1)]
    ys = m(xs)
    sum((y * gy[:, G.sl(L)].to(DEV)).sum() for L, y in enumerate(ys)).backward()
    enabled = list(m._paths)
    c_model = torch.stack([m.mixcoeff(*p).detach().cpu() for p in enabled])[None]                     # [1, n, 1]
    keep = torch.stack([m.keepcoeff(L).detach().cpu() for L in range(min(oi, oo) + 1)])
    r64, r32 = mix_refs(x, x, c_model, keep, enabled, oo, gy)
    assert_sum("SelfMixing F=1 y", torch.cat([y.detach() for y in ys], dim=1), r64[0], r32[0])
    assert_sum("SelfMixing F=1 grad_x", torch.cat([t.grad for t in xs], dim=1), r64[1] + r64[2], r32[1] + r32[2])
    assert_sum("SelfMixing F=1 grad_mix", torch.stack([m.mixcoeff(*p).grad for p in enabled]), r64[3].sum(0), r32[3].sum(0))
    assert_sum("SelfMixing F=1 grad_keep", torch.stack([m.keepcoeff(L).grad for L in range(min(oi, oo) + 1)]), r64[4].sum(0), r32[4].sum(0))


def test_partial_blocks_agree_with_the_mirror():
    for F in (1, 2, 4, 8, 16, 32, 64, 128, 256, 48, 0):
        for rows in (0, 1, 255, 256, 257, 1024, 10 ** 5, 10 ** 7):
            assert int(lib().nq_so3_mix_partial_blocks(rows, F)) == G.so3_partial_blocks(rows, F), (rows, F)


def test_backward_shared_rejects_F_48():
    rows, F = 5, 48
    x = torch.zeros(rows, 25, F, device=DEV)
    c = torch.zeros(65, F, device=DEV)
    gx1, gx2, part = nan_dev(rows, 25, F), nan_dev(rows, 25, F), nan_dev(rows, 65, F)
    assert int(lib().nq_so3_mix_partial_blocks(rows, F)) == 0
    rejected(lambda: lib().nq_so3_mix_backward_shared(P(x), P(x), P(c), None, P(x), rows, F, 4, 4, 4, path_index(cg.ALL_PATHS), 0, P(gx1), P(gx2), P(part), None,
                                                      st()), gx1, gx2, part)
