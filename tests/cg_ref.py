"""Test helper: small literal restatements for the Clebsch-Gordan operator tests (test_qhnet_ops_gpu.py, test_so3_ops_gpu.py), only where
oracle/qhnet_ref.py has no function of its own, and Python mirrors of the host-side launch rules the tests name their cases by.  Everything works in
the dtype of its inputs (float64 for the reference value, float32 for the yardstick); adjoints come from torch.autograd on these functions.

Conventions that are choices (asserted exactly in test_cg_ref_cpu.py):
  * the gradient of a norm is 0 where the norm is 0 (normcat_ref);
  * the shifted softplus returns x - log 2 above x = 20 (act_ref kind 1), as torch.nn.functional.softplus does."""
import math

import numpy as np
import torch

from tests.test_split_math_cpu import bf16_rne


def sl(l):
    return slice(l * l, (l + 1) * (l + 1))


def lmax_of(ncomp):
    lmax = int(round(math.sqrt(ncomp))) - 1
    assert (lmax + 1) ** 2 == ncomp
    return lmax


def pad25(x):
    """[rows, ncomp, C] -> [rows, 25, C], the missing degrees zero."""
    if x.shape[1] == 25:
        return x
    return torch.cat([x, x.new_zeros(x.shape[0], 25 - x.shape[1], x.shape[2])], dim=1)


def pair_reduce_ref(a, b, base, row_ptr, rev, N, W, dt):
    """out[n] = base[n] + sum over the rows r of atom n, ascending, of (a[r] + b[rev[r]]); every operand may be None."""
    out = torch.zeros(N, W, dtype=dt) if base is None else base.to(dt).clone()
    for n in range(N):
        for r in range(int(row_ptr[n]), int(row_ptr[n + 1])):
            if a is not None:
                out[n] = out[n] + a[r].to(dt)
            if b is not None:
                out[n] = out[n] + b[int(rev[r])].to(dt)
    return out


def normcat_ref(x):
    """x [rows, (lmax+1)^2, C] -> [rows, (lmax+1) C] = [x_0 | |x_1| | ... | |x_lmax|]; d|x_l| = 0 where |x_l| = 0."""
    lmax = lmax_of(x.shape[1])
    parts = [x[:, 0]]
    for l in range(1, lmax + 1):
        s = x[:, sl(l)].pow(2).sum(1)
        pos = s > 0
        parts.append(torch.where(pos, torch.where(pos, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s)))
    return torch.cat(parts, dim=-1)


def gate_ref(x, gates):
    """y = [gates_0 | x_l * gates_l, l = 1..lmax]; x [rows, (lmax+1)^2, C], gates [rows, (lmax+1) C]."""
    lmax, C = lmax_of(x.shape[1]), x.shape[-1]
    out = [gates[:, None, :C]] + [x[:, sl(l)] * gates[:, None, l * C:(l + 1) * C] for l in range(1, lmax + 1)]
    return torch.cat(out, dim=1)


def act_ref(x, kind, cst):
    """cst * silu(x) (kind 0) or cst * (softplus(x) - log 2) (kind 1; softplus(x) = x above 20)."""
    if kind == 0:
        return cst * torch.nn.functional.silu(x)
    return cst * (torch.nn.functional.softplus(x, beta=1.0, threshold=20.0) - math.log(2.0))


def split2(a):
    """float32 array -> its two bfloat16 pieces (as float32): round to nearest even of the value, then of the (exact) remainder."""
    a = np.asarray(a, np.float32)
    hi = bf16_rne(a)
    lo = bf16_rne((a - hi).astype(np.float32))
    return hi, lo


def split2_mirror(h, W):
    """h [R, K] @ W [K, n] with the arithmetic of the fused generator: hi hi' + hi lo' + lo hi' on two-piece operands, piece products summed in
    float64.  Returns float64 [R, n]."""
    hh, hl = (p.astype(np.float64) for p in split2(h))
    wh, wl = (p.astype(np.float64) for p in split2(W))
    return hh @ wh + hh @ wl + hl @ wh


# ---- mirrors of host-side launch rules ----------------------------------------------------------------------------------------------------------------
def so3_rows_per_block(rows, F):
    """csrc/so3.hip so3_rows_per_block: rows one workgroup of the shared-coefficient reverse kernel walks."""
    rpp = 256 // F
    k = (rows + 1023) // 1024
    k = (k + rpp - 1) // rpp * rpp
    if k > 128:
        k = 128 // rpp * rpp
    if k < rpp:
        k = rpp
    return k


def so3_partial_blocks(rows, F):
    if F <= 0 or 256 % F != 0 or rows <= 0:
        return 0
    k = so3_rows_per_block(rows, F)
    return (rows + k - 1) // k


EXP_INSTRUCTIONS = [(li, l1, l2) for li in range(5) for l1 in range(3) for l2 in range(3) if abs(l1 - l2) <= li <= l1 + l2]


def expansion_layout(counts, Cb):
    """(n_weights, n_bias, S, res_total, combos) of the expansion for shell counts (n_s, n_p, n_d)."""
    nw = sum(Cb * counts[l1] * counts[l2] for _, l1, l2 in EXP_INSTRUCTIONS)
    nb = sum(counts[l1] * counts[l2] for li, l1, l2 in EXP_INSTRUCTIONS if li == 0)
    S = counts[0] + 3 * counts[1] + 5 * counts[2]
    res = sum(counts[l1] * counts[l2] * (2 * li + 1) for li, l1, l2 in EXP_INSTRUCTIONS)
    return nw, nb, S, res, sum(counts) ** 2


def expansion_lds_forward(counts, Cb):
    """bytes of dynamic LDS nq_qh_expansion_forward asks for."""
    nw, nb, _, _, _ = expansion_layout(counts, Cb)
    return 4 * ((nw + 3) // 4 * 4 + 25 * Cb + nb + 4)


def expansion_lds_backward(counts, Cb):
    """bytes of dynamic LDS nq_qh_expansion_backward asks for."""
    nw, _, S, res, _ = expansion_layout(counts, Cb)
    return 4 * ((nw + 3) // 4 * 4 + 25 * Cb + S * S + res + 4)
