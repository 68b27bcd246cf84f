"""Pins the restatements of tests/phisnet_ops_ref.py to vectors recorded from the reference project (tests/golden/geometry_bases.npz, written by
oracle/make_golden_phisnet.py --bases): they are the reference's functions, not a copy of the kernels.  Float32 evaluations at the tolerances the GPU
tests of the same fixture use (test_so3_gpu.py); the rows where the reference's plain Bernstein basis is NaN (r >= cutoff) are left out, as there."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import hblock_ref  # noqa: E402
from tests import phisnet_ops_ref as R  # noqa: E402
from tests.helpers import GOLDEN, rel_err  # noqa: E402

F32, F64 = torch.float32, torch.float64


def fixture():
    return np.load(os.path.join(GOLDEN, "geometry_bases.npz"))


def test_spherical_harmonics_match_reference():
    fx = fixture()
    y = R.sph_harm(4, torch.tensor(fx["u"]), F32).numpy()
    for l in range(5):
        ref = fx[f"Y_{l}"]
        assert y[:, l * l:(l + 1) ** 2].shape == ref.shape and np.abs(y[:, l * l:(l + 1) ** 2] - ref).max() < 5e-6, l
    for L in range(4):                                        # a lower order is the leading block of a higher one
        assert torch.equal(R.sph_harm(L, torch.tensor(fx["u"]), F32), torch.tensor(y[:, :(L + 1) ** 2]))


def test_spherical_harmonics_norm():
    """sum_m Y_lm(u)^2 = 2l + 1 on unit vectors (no 1 / sqrt(4 pi)), the axis directions and (1, 1, 1) / sqrt(3) included."""
    gen = torch.Generator().manual_seed(5)
    u = torch.randn(200, 3, generator=gen, dtype=F64)
    u = torch.cat([torch.eye(3, dtype=F64), -torch.eye(3, dtype=F64), torch.ones(1, 3, dtype=F64), u])
    u = u / u.norm(dim=1, keepdim=True)
    y = R.sph_harm(4, u, F64)
    for l in range(5):
        assert float(((y[:, l * l:(l + 1) ** 2] ** 2).sum(1) - (2 * l + 1)).abs().max()) < 1e-13, l


def test_exponential_bernstein_matches_reference():
    fx = fixture()
    for tag in ("phisnet128", "qhnet32", "small"):
        K, cutoff, ini = fx[f"{tag}:cfg"]
        K = int(K)
        logc, n, v = R.bernstein_tables(K, F64)
        assert np.allclose(logc.numpy(), fx[f"{tag}:logc"], rtol=1e-6, atol=1e-5)
        assert n.tolist() == list(range(K - 1, -1, -1)) and v.tolist() == list(range(K))
        raw = torch.tensor(float(fx[f"{tag}:_alpha"]), dtype=F32, requires_grad=True)
        out = R.exp_bernstein(torch.tensor(fx[f"{tag}:r"]).reshape(-1), K, float(cutoff), torch.nn.functional.softplus(raw), F32)
        assert abs(float(torch.nn.functional.softplus(raw.detach())) - float(ini)) < 1e-6           # _alpha is softplus^-1 of the initial alpha
        assert out.shape == fx[f"{tag}:rbf"].shape and rel_err(out.detach().numpy(), fx[f"{tag}:rbf"]) < 2e-5, tag
        assert float(out.detach()[-1].abs().max()) == 0.0 and float(out.detach()[-2].abs().max()) == 0.0     # r >= cutoff -> exactly 0
        (out * torch.tensor(fx[f"{tag}:w"])).sum().backward()
        ref = float(fx[f"{tag}:g_alpha"])
        assert abs(float(raw.grad) - ref) < 5e-5 * max(1.0, abs(ref)), tag


def test_other_radial_bases_match_reference():
    fx = fixture()
    for kind, tag in ((1, "gaussian"), (2, "exp-gaussian"), (3, "overlap-bernstein"), (4, "bernstein")):
        args = fx[f"rb:{tag}:args"]
        K, cutoff = int(args[0]), float(args[1])
        x = torch.tensor(float(args[2]) if len(args) > 2 else 1.0, dtype=F64)
        raw = (x + torch.log(-torch.expm1(-x))).to(F32).requires_grad_(True)               # softplus^-1 of the initial alpha
        out = R.radial_basis(kind, torch.tensor(fx[f"rb:{tag}:r"]).reshape(-1), K, cutoff, torch.nn.functional.softplus(raw), F32)
        ref = fx[f"rb:{tag}:rbf"]
        inside = ~np.isnan(ref).any(axis=-1)
        assert inside.sum() >= 30 and (tag == "bernstein" or inside.all())
        assert out.shape == ref.shape and rel_err(out.detach().numpy()[inside], ref[inside]) < 1e-5, tag
        assert float(out.detach()[-1].abs().max()) == 0.0 and float(out.detach()[-2].abs().max()) == 0.0
        if kind in (2, 3):
            (out * torch.tensor(fx[f"rb:{tag}:w"])).sum().backward()
            g = float(fx[f"rb:{tag}:g_alpha"])
            assert abs(float(raw.grad) - g) < 2e-5 * max(1.0, abs(g)), (tag, float(raw.grad), g)


def test_activations():
    """The definitions at their fixed points: beta == 0 (alpha x / 2 for both kinds), the far tails, and the packed form."""
    x = torch.tensor([[-90.0, -30.0, -1.0, 0.0, 0.5, 30.0, 90.0]], dtype=F64).T.repeat(1, 3)
    alpha, beta = torch.tensor([1.0, 0.7, -1.3], dtype=F64), torch.tensor([1.0, 0.0, -2.0], dtype=F64)
    sw, sp = R.activation(0, x, alpha, beta, F64), R.activation(1, x, alpha, beta, F64)
    assert torch.equal(sw[:, 1], 0.35 * x[:, 1]) and torch.equal(sp[:, 1], 0.35 * x[:, 1])
    assert torch.allclose(sw[:, 0], x[:, 0] / (1 + torch.exp(-x[:, 0])), rtol=1e-14, atol=0)
    assert torch.allclose(sp[:, 0], torch.nn.functional.softplus(x[:, 0]) - np.log(2.0), rtol=1e-14, atol=1e-15)
    assert abs(float(sp[-1, 2]) - (-1.3) * (0.0 - np.log(2.0)) / (-2.0)) < 1e-15 and abs(float(sp[0, 2]) - (-1.3) * (180.0 - np.log(2.0)) / (-2.0)) < 1e-12
    xp = torch.randn(4, 9, 3, dtype=F64, generator=torch.Generator().manual_seed(1))
    yp = R.packed_activation(1, xp, alpha, beta, F64)
    assert torch.equal(yp[:, 1:], xp[:, 1:]) and torch.equal(yp[:, 0], R.activation(1, xp[:, 0], alpha, beta, F64))


def test_sph_linear_and_loss():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(5, 9, 4, dtype=F64, generator=gen)
    ws = [torch.randn(3, 4, dtype=F64, generator=gen) for _ in range(3)]
    b = torch.randn(3, dtype=F64, generator=gen)
    y = R.sph_linear(x, ws, b, F64)
    assert y.shape == (5, 9, 3)
    for c in range(9):
        L = int(np.sqrt(c))
        assert torch.allclose(y[:, c], torch.nn.functional.linear(x[:, c], ws[L], b if c == 0 else None), rtol=1e-14, atol=1e-14)
    d = torch.tensor([3.0, -4.0, 0.0, 0.0], dtype=F64)
    loss = hblock_ref.hamiltonian_loss(d, torch.zeros(4, dtype=F64), torch.ones(4, dtype=F64))
    assert abs(float(loss) - (2.5 + 1.75)) < 1e-15                                          # rmse + mae
