"""Plain torch restatements of the PhiSNet basis, activation and linear operations, written from the formulas and sharing no code with
nabladft_amd.  Every function takes a dtype: the float64 evaluation is the reference of the operator tests (tests/test_phisnet_ops_gpu.py), the float32
evaluation of the same text on the CPU is their yardstick, and torch.autograd on either gives the adjoints.  tests/test_phisnet_ops_ref_cpu.py pins these
functions to vectors recorded from the reference project (tests/golden/geometry_bases.npz).

Conventions: real spherical harmonics without the 1 / sqrt(4 pi), Condon-Shortley phase, m = -l..l, Y_1 = sqrt(3) (y, z, x); they are POLYNOMIALS of a free
vector (x, y, z) -- the extensions off the unit sphere that the reference project writes down (3 z^2 - 1, not 2 z^2 - x^2 - y^2) -- so their gradient has a
radial component.  Every radial basis is multiplied by the smooth cutoff exp(-r^2 / ((c - r)(c + r))) and is exactly 0 at r >= c."""
import math

import torch

SQ = math.sqrt

# Y_lm as {(i, j, k): coefficient} of the monomials x^i y^j z^k, components in the order m = -l..l
SPH_POLY = [
    [{(0, 0, 0): 1.0}],
    [{(0, 1, 0): SQ(3)}, {(0, 0, 1): SQ(3)}, {(1, 0, 0): SQ(3)}],
    [{(1, 1, 0): SQ(15)},
     {(0, 1, 1): SQ(15)},
     {(0, 0, 2): 3 * SQ(5) / 2, (0, 0, 0): -SQ(5) / 2},
     {(1, 0, 1): SQ(15)},
     {(2, 0, 0): SQ(15) / 2, (0, 2, 0): -SQ(15) / 2}],
    [{(2, 1, 0): 3 * SQ(70) / 4, (0, 3, 0): -SQ(70) / 4},
     {(1, 1, 1): SQ(105)},
     {(0, 1, 2): 5 * SQ(42) / 4, (0, 1, 0): -SQ(42) / 4},
     {(0, 0, 3): 5 * SQ(7) / 2, (0, 0, 1): -3 * SQ(7) / 2},
     {(1, 0, 2): 5 * SQ(42) / 4, (1, 0, 0): -SQ(42) / 4},
     {(2, 0, 1): SQ(105) / 2, (0, 2, 1): -SQ(105) / 2},
     {(3, 0, 0): SQ(70) / 4, (1, 2, 0): -3 * SQ(70) / 4}],
    [{(3, 1, 0): 3 * SQ(35) / 2, (1, 3, 0): -3 * SQ(35) / 2},
     {(2, 1, 1): 9 * SQ(70) / 4, (0, 3, 1): -3 * SQ(70) / 4},
     {(1, 1, 2): 7 * SQ(45) / 2, (1, 1, 0): -SQ(45) / 2},
     {(0, 1, 3): 21 * SQ(10) / 4, (0, 1, 1): -9 * SQ(10) / 4},
     {(0, 0, 4): 105 / 8, (0, 0, 2): -90 / 8, (0, 0, 0): 9 / 8},
     {(1, 0, 3): 21 * SQ(10) / 4, (1, 0, 1): -9 * SQ(10) / 4},
     {(2, 0, 2): 7 * SQ(45) / 4, (0, 2, 2): -7 * SQ(45) / 4, (2, 0, 0): -SQ(45) / 4, (0, 2, 0): SQ(45) / 4},
     {(3, 0, 1): 3 * SQ(70) / 4, (1, 2, 1): -9 * SQ(70) / 4},
     {(4, 0, 0): 3 * SQ(35) / 8, (2, 2, 0): -18 * SQ(35) / 8, (0, 4, 0): 3 * SQ(35) / 8}],
]


def sph_harm(order, u, dtype):
    """[P, (order + 1)^2]: Y_0..Y_order of the free vectors u [P, 3], every monomial evaluated in ``dtype``."""
    u = u.to(dtype)
    pw = [[torch.ones_like(u[:, a]), u[:, a], u[:, a] ** 2, u[:, a] ** 3, u[:, a] ** 4] for a in range(3)]
    cols = []
    for l in range(order + 1):
        for poly in SPH_POLY[l]:
            acc = torch.zeros_like(u[:, 0])
            for (i, j, k), c in poly.items():
                acc = acc + torch.tensor(c, dtype=dtype) * pw[0][i] * pw[1][j] * pw[2][k]
            cols.append(acc)
    return torch.stack(cols, dim=1)


def smooth_cutoff(r, cutoff):
    """exp(-r^2 / ((c - r)(c + r))) below the cutoff, exactly 0 from it on (r: [P, 1] or [P])."""
    inside = r < cutoff
    rs = torch.where(inside, r, torch.zeros_like(r))
    return torch.where(inside, torch.exp(-rs * rs / ((cutoff - rs) * (cutoff + rs))), torch.zeros_like(r))


def log_binomials(K):
    """(log C(K - 1, k), n_k = K - 1 - k, v_k = k) for k = 0..K-1 as Python floats, from lgamma."""
    logc = [math.lgamma(K) - math.lgamma(k + 1) - math.lgamma(K - k) for k in range(K)]
    return logc, [float(K - 1 - k) for k in range(K)], [float(k) for k in range(K)]


def bernstein_tables(K, dtype):
    return tuple(torch.tensor(t, dtype=torch.float64).to(dtype) for t in log_binomials(K))


def _bernstein_of_x(x, r, K, cutoff, dtype):
    """fc(r) exp(log C_k + n_k x + v_k log(1 - e^x)) for x < 0 given per row; rows at / beyond the cutoff are exactly 0 (and carry no gradient)."""
    logc, n, v = bernstein_tables(K, dtype)
    val = smooth_cutoff(r, cutoff) * torch.exp(logc + n * x + v * torch.log(-torch.expm1(x)))
    return torch.where(r < cutoff, val, torch.zeros_like(val))


def _inside(r, cutoff):
    """r [P] -> (r [P, 1], a copy that is harmless where r >= cutoff): the branch that is masked out must not produce NaN for autograd to multiply by 0."""
    r = r.reshape(-1, 1)
    return r, torch.where(r < cutoff, r, torch.full_like(r, 0.5 * cutoff))


def exp_bernstein(r, K, cutoff, alpha, dtype):
    """Exponential Bernstein basis [P, K]: x = -alpha r.  ``alpha`` = softplus(_alpha): a number or a tensor ([] or [P, 1])."""
    r, rs = _inside(r.to(dtype), cutoff)
    alpha = torch.as_tensor(alpha, dtype=dtype)
    return torch.where(r < cutoff, _bernstein_of_x(-alpha * rs, rs, K, cutoff, dtype), torch.zeros_like(r))


def gaussian(r, K, cutoff, dtype):
    """fc exp(-width (r - center_k)^2), centers linspace(0, c, K), width K / c."""
    r, rs = _inside(r.to(dtype), cutoff)
    center = torch.linspace(0, cutoff, K, dtype=torch.float64).to(dtype)
    val = smooth_cutoff(rs, cutoff) * torch.exp(-torch.tensor(K / cutoff, dtype=dtype) * (rs - center) ** 2)
    return torch.where(r < cutoff, val, torch.zeros_like(val))


def exp_gaussian(r, K, cutoff, alpha, dtype):
    """fc exp(-width (e^{-alpha r} - center_k)^2), centers linspace(1, 0, K), width K."""
    r, rs = _inside(r.to(dtype), cutoff)
    alpha = torch.as_tensor(alpha, dtype=dtype)
    center = torch.linspace(1, 0, K, dtype=torch.float64).to(dtype)
    val = smooth_cutoff(rs, cutoff) * torch.exp(-torch.tensor(float(K), dtype=dtype) * (torch.exp(-alpha * rs) - center) ** 2)
    return torch.where(r < cutoff, val, torch.zeros_like(val))


def overlap_bernstein(r, K, cutoff, alpha, dtype):
    """Bernstein polynomials of the overlap-like variable: x = log(1 + alpha r) - alpha r."""
    r, rs = _inside(r.to(dtype), cutoff)
    alpha = torch.as_tensor(alpha, dtype=dtype)
    ar = alpha * rs
    return torch.where(r < cutoff, _bernstein_of_x(torch.log1p(ar) - ar, rs, K, cutoff, dtype), torch.zeros_like(r))


def bernstein(r, K, cutoff, dtype):
    """Plain Bernstein polynomials of r / c: x = log(r / c)."""
    r, rs = _inside(r.to(dtype), cutoff)
    return torch.where(r < cutoff, _bernstein_of_x(torch.log(rs / cutoff), rs, K, cutoff, dtype), torch.zeros_like(r))


def radial_basis(kind, r, K, cutoff, alpha, dtype):
    """The kinds of nq_radial_basis: 1 gaussian, 2 exp-gaussian, 3 overlap-bernstein, 4 bernstein."""
    if kind == 1:
        return gaussian(r, K, cutoff, dtype)
    if kind == 2:
        return exp_gaussian(r, K, cutoff, alpha, dtype)
    if kind == 3:
        return overlap_bernstein(r, K, cutoff, alpha, dtype)
    return bernstein(r, K, cutoff, dtype)


def radial_tables(kind, K, cutoff, dtype):
    """(t0, t1, t2, width) the kinds of nq_radial_basis read: centers and width (1, 2) or the Bernstein tables (3, 4)."""
    if kind == 1:
        return torch.linspace(0, cutoff, K, dtype=torch.float64).to(dtype), None, None, K / cutoff
    if kind == 2:
        return torch.linspace(1, 0, K, dtype=torch.float64).to(dtype), None, None, float(K)
    return (*bernstein_tables(K, dtype), 0.0)


def activation(kind, x, alpha, beta, dtype):
    """kind 0: swish alpha x sigmoid(beta x); kind 1: shifted softplus alpha (softplus(beta x) - ln 2) / beta, defined as alpha x / 2 where beta == 0.
    x [..., F]; alpha, beta [F] or broadcastable to x (per-row copies give per-row gradients)."""
    x, alpha, beta = x.to(dtype), alpha.to(dtype), beta.to(dtype)
    if kind == 0:
        return alpha * x * torch.sigmoid(beta * x)
    safe = torch.where(beta != 0, beta, torch.ones_like(beta))
    soft = torch.logaddexp(safe * x, torch.zeros_like(x))          # log(1 + e^t), stable on both tails
    return alpha * torch.where(beta != 0, (soft - math.log(2.0)) / safe, 0.5 * x)


def packed_activation(kind, x, alpha, beta, dtype):
    """x [rows, ncomp, F]: the scalar rows (component 0) activated, every other component copied."""
    x = x.to(dtype)
    return torch.cat([activation(kind, x[:, :1], alpha, beta, dtype), x[:, 1:]], dim=1)


def sph_linear(x, weights, bias, dtype):
    """y[:, sl(L)] = x[:, sl(L)] @ W_L^T for L = 0..order (sl(L) = components L^2 .. (L+1)^2), the bias on the scalar row only.
    x [rows, (order + 1)^2, Fin], W_L [Fout, Fin], bias [Fout] or None."""
    x = x.to(dtype)
    ys = [x[:, L * L:(L + 1) * (L + 1)] @ W.to(dtype).T for L, W in enumerate(weights)]
    if bias is not None:
        ys[0] = ys[0] + bias.to(dtype)
    return torch.cat(ys, dim=1)
