"""The Graphormer3D kernels of csrc/graphormer.hip one by one through the C ABI against the float64 ragged restatement (tests/graphormer_ref.py), built from the
kernel's own float32 inputs promoted to float64.  Every output buffer starts as NaN, so an element a kernel never writes fails the comparison; the
accumulated bias adjoint starts from random finite values that the restatement adds.

Bounds (the convention of test_gemnet_ops_gpu.py / tests/helpers.assert_sum): copies and layouts are exact; every summing kernel must stay within
max(3 x the error of the same formula evaluated in float32 on the CPU, 2e-6) of the float64 value AND below 1e-5, array-relative (max |a - b| / max |b|).
Every backward runs twice and must give bitwise equal results.

Shapes: H = 2, d = 16 and 32, K = 32; molecules of 1, 2, 63, 64, 65 and 129 atoms in one batch (N = 324, P = 28 936): a single key (softmax of one element), a
wavefront with one idle lane, exactly full, one lane in the second row tile, and a third key tile with one key.  The first molecule is a lone Br and the second
S-Cl, so three edge types occur once while H-H occurs thousands of times.  Plus one molecule at the built size limit and one above it."""
import numpy as np
import pytest
import torch

from tests import graphormer_ref as G
from tests.helpers import DEV, P, _release_copies, assert_sum, bits, check, lib, nan_dev, rejected, st, twice  # noqa: F401  (_release_copies: autouse)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 129)
H, K = 2, 32
_CASE = {}


def _structure(sizes):
    ptr, pair_ptr, atom_mol = G.structure(sizes)
    return dict(ptr=ptr, pair_ptr=pair_ptr, sizes=sizes, N=int(ptr[-1]), P=int(pair_ptr[-1]), B=len(sizes), max_mol=max(sizes),
                d_ptr=ptr.to(torch.int32).to(DEV), d_pair_ptr=pair_ptr.to(DEV), d_atom_mol=atom_mol.to(torch.int32).to(DEV))


def case(d):
    """Inputs (float32, host), their device copies and the batch structure for head dimension d; built once."""
    if d in _CASE:
        return _CASE[d]
    g = torch.Generator().manual_seed(100 + d)
    s = _structure(SIZES)
    b = G.make_batch(SIZES, 5)
    z = b["z"].clone()
    z[0], z[1], z[2] = 35, 16, 17
    z[3:] = torch.tensor(np.random.default_rng(1).choice([1, 1, 1, 6, 6, 7, 8], size=s["N"] - 3))
    E = H * d
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)          # noqa: E731
    c = dict(s, d=d, E=E, z=z, pos=b["pos"].float(), scaling=d ** -0.5, qkv=r(s["N"], 3 * E), bias=r(s["P"], H), W3=r(3, E) / d ** 0.5, b3=r(3), g_out=r(s["N"], E),
             g_f=r(s["N"], 3), acc0=r(s["P"] * H), keep=(torch.rand(s["P"] * H, generator=g) >= 0.1).to(torch.uint8), r=r)
    c["unit"] = G.pair_geometry(c["pos"].double(), z, s["ptr"])[1].float()                # the kernel's own float32 unit vectors are tested in test_pair_forward
    c["bias_hm"] = G.to_heads(c["bias"], SIZES)
    c["keep_pm"] = G.from_heads(c["keep"], SIZES, H)
    _CASE[d] = c
    return c


def dev(c, *names):
    return [c[n].to(DEV).contiguous() for n in names]


def both(fn):
    """fn(dtype) -> tensor or tuple of tensors: evaluated in float64 and in float32 on the CPU."""
    return fn(torch.float64), fn(torch.float32)


def compare(name, got, ref):
    r64, r32 = ref
    if torch.is_tensor(r64):
        got, r64, r32 = (got,), (r64,), (r32,)
    errs = [assert_sum(f"{name}[{i}]", g, a, b) for i, (g, a, b) in enumerate(zip(got, r64, r32))]
    print(name, " ".join(f"{e:.2e}" for e in errs))


# ---- pair featuriser ----------------------------------------------------------------------------------------------------------------------------------------
def _gauss_params(c):
    g = torch.Generator().manual_seed(7)
    mul = 1.0 + 0.2 * torch.randn(G.EDGE_TYPES, 1, generator=g)
    bias = 0.2 * torch.randn(G.EDGE_TYPES, 1, generator=g)
    means = torch.rand(1, K, generator=g) * 3
    stds = (0.3 + 2.7 * torch.rand(1, K, generator=g)) * torch.where(torch.rand(1, K, generator=g) < 0.25, -1.0, 1.0)
    stds[0, 1] = -abs(stds[0, 1])
    stds[0, 5], means[0, 5] = 0.0, -5.0                                 # |.| at exactly 0 (std = 1e-5, torch's convention: gradient 0), its mean far from every x
    return mul, bias, means, stds


def _pair_forward(c, prm, max_mol=None):
    d_pos, d_z = c["pos"].to(DEV), c["z"].to(torch.int32).to(DEV)
    dp = [t.to(DEV) for t in prm]
    outs = nan_dev(c["P"], K), nan_dev(c["P"], 3), nan_dev(c["P"]), nan_dev(c["N"], K)
    rc = lib().nq_g3d_pair_forward(P(d_pos), P(d_z), P(c["d_ptr"]), P(c["d_atom_mol"]), P(c["d_pair_ptr"]), P(dp[0]), P(dp[1]), P(dp[2]), P(dp[3]), c["N"], K,
                                   c["max_mol"] if max_mol is None else max_mol, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), st())
    return rc, outs


def test_pair_forward():
    c = case(16)
    prm = _gauss_params(c)
    rc, (gbf, unit, dist, efeat) = _pair_forward(c, prm)
    check(rc)
    ref = both(lambda dt: G.pair_features(c["pos"].to(dt), c["z"], c["ptr"], *[t.to(dt) for t in prm]))
    compare("pair_forward gbf unit dist efeat", (gbf, unit, dist, efeat), ref)
    selfp = torch.cat([c["pair_ptr"][b] + torch.arange(n) * (n + 1) for b, n in enumerate(SIZES)])
    assert float(dist.cpu()[selfp].abs().max()) == 0.0 and float(unit.cpu()[selfp].abs().max()) == 0.0
    # the reference's truncated pi: against the float64 value the mean ratio sits at 1, with the true pi it would sit 4.2e-7 below
    r64 = ref[0][0]
    big = r64 > 1e-3
    assert abs(float((gbf.cpu().double()[big] / r64[big]).mean()) - 1.0) < 1e-7
    with_pi = r64 * (2 * 3.14159) ** 0.5 / (2 * np.pi) ** 0.5
    assert abs(float((gbf.cpu().double()[big] / with_pi[big]).mean()) - 1.0) > 3e-7


@pytest.mark.parametrize("which", ["both", "efeat_only", "gbf_only"])
def test_pair_backward(which):
    c = case(16)
    prm = _gauss_params(c)
    g_gbf = c["r"](c["P"], K) if which != "efeat_only" else None
    g_ef = c["r"](c["N"], K) if which != "gbf_only" else None
    d_pos, d_z = c["pos"].to(DEV), c["z"].to(torch.int32).to(DEV)
    dp = [t.to(DEV) for t in prm]
    rc, (_, _, dist, _) = _pair_forward(c, prm)
    check(rc)
    _, _, et, _ = G.pair_geometry(c["pos"].double(), c["z"], c["ptr"])
    counts = torch.bincount(et, minlength=G.EDGE_TYPES)
    assert int((counts == 1).sum()) >= 3 and int(counts.max()) > 1000          # edge types that occur once and many times
    order = torch.sort(et, stable=True).indices.to(DEV)
    type_ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(DEV)
    dg, de = (None if g_gbf is None else g_gbf.to(DEV)), (None if g_ef is None else g_ef.to(DEV))
    scr = torch.empty(int(lib().nq_g3d_pair_scratch_floats(c["N"], c["P"], K)), device=DEV)

    def call():
        outs = nan_dev(K), nan_dev(K), nan_dev(G.EDGE_TYPES), nan_dev(G.EDGE_TYPES)
        check(lib().nq_g3d_pair_backward(P(d_pos), P(d_z), P(c["d_ptr"]), P(c["d_atom_mol"]), P(c["d_pair_ptr"]), P(dp[0]), P(dp[1]), P(dp[2]), P(dp[3]), P(dist),
                                         P(order), P(type_ptr), c["N"], c["P"], K, P(dg), P(de), P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), P(scr), st()))
        return outs
    got = twice(call)
    ref = both(lambda dt: G.pair_features_backward(c["pos"].to(dt), c["z"], c["ptr"], *[t.to(dt) for t in prm], None if g_gbf is None else g_gbf.to(dt),
                                                   None if g_ef is None else g_ef.to(dt)))
    compare(f"pair_backward[{which}] means stds mul bias", got, ref)
    assert float(got[1].cpu()[5]) == 0.0 and float(got[1].cpu()[1]) != 0.0
    assert float(got[2].cpu()[counts == 0].abs().max()) == 0.0


# ---- bias layout --------------------------------------------------------------------------------------------------------------------------------------------
def test_bias_layout_round_trip_is_exact():
    c = case(16)
    pm = c["bias"].to(DEV)
    hm, back = nan_dev(c["P"] * H), nan_dev(c["P"], H)
    check(lib().nq_g3d_bias_to_heads(P(pm), P(c["d_ptr"]), P(c["d_atom_mol"]), P(c["d_pair_ptr"]), c["N"], H, P(hm), st()))
    check(lib().nq_g3d_bias_from_heads(P(hm), P(c["d_ptr"]), P(c["d_atom_mol"]), P(c["d_pair_ptr"]), c["N"], H, P(back), st()))
    assert torch.equal(bits(hm), bits(c["bias_hm"])) and torch.equal(bits(back), bits(c["bias"]))


# ---- attention ----------------------------------------------------------------------------------------------------------------------------------------------
def _mask(c, masked):
    return (c["keep"].to(DEV), 1.0 / 0.9, c["keep_pm"]) if masked else (None, 1.0, None)


def _attention_forward(c, qkv, bias_hm, mask, scale, max_mol=None):
    out, lse = nan_dev(c["N"], c["E"]), nan_dev(c["N"], H)
    rc = lib().nq_g3d_attention_forward(P(qkv), P(bias_hm), P(mask), scale, P(c["d_ptr"]), P(c["d_pair_ptr"]), c["B"], c["N"], H, c["d"],
                                        c["max_mol"] if max_mol is None else max_mol, c["scaling"], P(out), P(lse), st())
    return rc, out, lse


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d", [16, 32])
def test_attention_forward_backward(d, masked):
    c = case(d)
    qkv, bias_hm, g_out = dev(c, "qkv", "bias_hm", "g_out")
    mask, scale, keep_pm = _mask(c, masked)
    rc, out, lse = _attention_forward(c, qkv, bias_hm, mask, scale)
    check(rc)
    kw = lambda dt: dict(keep_pm=None if keep_pm is None else keep_pm.to(dt), mask_scale=scale)          # noqa: E731
    compare(f"attention_forward[d={d},mask={masked}]", out,
            both(lambda dt: G.attention(c["qkv"].to(dt), c["bias"].to(dt), c["ptr"], c["pair_ptr"], H, c["scaling"], **kw(dt))))
    scr = torch.empty(c["N"] * H, device=DEV)

    def call():
        g_qkv, acc = nan_dev(c["N"], 3 * c["E"]), c["acc0"].to(DEV)
        for _ in range(2):                                              # the bias adjoint accumulates over two calls
            check(lib().nq_g3d_attention_backward(P(qkv), P(bias_hm), P(mask), scale, P(c["d_ptr"]), P(c["d_pair_ptr"]), c["B"], c["N"], H, d, c["max_mol"], c["scaling"],
                                                  P(out), P(lse), P(g_out), P(g_qkv), P(acc), P(scr), st()))
        return g_qkv, acc

    def ref(dt):
        gq, gb = G.attention_backward(c["qkv"].to(dt), c["bias"].to(dt), c["ptr"], c["pair_ptr"], H, c["scaling"], c["g_out"].to(dt), **kw(dt))
        return gq, c["acc0"].to(dt) + 2 * G.to_heads(gb, SIZES)
    compare(f"attention_backward[d={d},mask={masked}] qkv bias", twice(call), both(ref))


# ---- force head ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d", [16, 32])
def test_force_head_forward_backward(d, masked):
    c = case(d)
    qkv, bias_hm, unit, W3, b3, g_f = dev(c, "qkv", "bias_hm", "unit", "W3", "b3", "g_f")
    mask, scale, keep_pm = _mask(c, masked)
    fh, lse, f = nan_dev(c["N"], H, 3), nan_dev(c["N"], H), nan_dev(c["N"], 3)
    check(lib().nq_g3d_force_forward(P(qkv), P(bias_hm), P(mask), scale, P(unit), P(W3), P(b3), P(c["d_ptr"]), P(c["d_pair_ptr"]), c["B"], c["N"], H, d, c["max_mol"],
                                     c["scaling"], P(fh), P(lse), P(f), st()))
    kw = lambda dt: dict(keep_pm=None if keep_pm is None else keep_pm.to(dt), mask_scale=scale)          # noqa: E731
    args = lambda dt: (c["qkv"].to(dt), c["bias"].to(dt), c["unit"].to(dt), c["W3"].to(dt))               # noqa: E731
    compare(f"force_forward[d={d},mask={masked}]", f,
            both(lambda dt: G.force_head(*args(dt), c["b3"].to(dt), c["ptr"], c["pair_ptr"], H, c["scaling"], **kw(dt))))
    assert torch.equal(bits(f[0]), bits(b3))                            # a single atom: only the self pair, whose unit vector is 0
    scr = torch.empty(int(lib().nq_g3d_force_scratch_floats(c["N"], H, d)), device=DEV)

    def call():
        g_qkv, acc, g_W3, g_b3 = nan_dev(c["N"], 3 * c["E"]), c["acc0"].to(DEV), nan_dev(3, c["E"]), nan_dev(3)
        check(lib().nq_g3d_force_backward(P(qkv), P(bias_hm), P(mask), scale, P(unit), P(W3), P(c["d_ptr"]), P(c["d_pair_ptr"]), c["B"], c["N"], H, d, c["max_mol"],
                                          c["scaling"], P(fh), P(lse), P(g_f), P(g_qkv), P(acc), P(g_W3), P(g_b3), P(scr), st()))
        return g_qkv, acc, g_W3, g_b3

    def ref(dt):
        gq, gb, gw, gb3 = G.force_head_backward(*args(dt), c["ptr"], c["pair_ptr"], H, c["scaling"], c["g_f"].to(dt), **kw(dt))
        return gq, c["acc0"].to(dt) + G.to_heads(gb, SIZES), gw, gb3
    compare(f"force_backward[d={d},mask={masked}] qkv bias W3 b3", twice(call), both(ref))


# ---- GELU, row dot ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True])
def test_gelu(with_bias):
    g = torch.Generator().manual_seed(9)
    rows, Cc = 301, 96
    x = torch.randn(rows, Cc, generator=g) * 2.5
    x[0, :8] = torch.tensor([-12.0, -8.0, -6.5, -6.0, 6.0, 6.5, 8.0, 12.0])
    x[1, :3] = torch.tensor([0.0, 1e-4, -1e-4])
    b = torch.randn(Cc, generator=g) * (1.0 if with_bias else 0.0)
    gy = torch.randn(rows, Cc, generator=g)
    dx, db, dg = x.to(DEV), (b.to(DEV) if with_bias else None), gy.to(DEV)
    y, gx = nan_dev(rows, Cc), nan_dev(rows, Cc)
    check(lib().nq_g3d_gelu_forward(P(dx), P(db), rows, Cc, P(y), st()))
    compare(f"gelu_forward[bias={with_bias}]", y, both(lambda dt: G.gelu(x.to(dt) + b.to(dt))))

    def call():
        out = nan_dev(rows, Cc)
        check(lib().nq_g3d_gelu_backward(P(dx), P(db), P(dg), rows, Cc, P(out), st()))
        return (out,)
    (gx,) = twice(call)
    compare(f"gelu_backward[bias={with_bias}]", gx, both(lambda dt: G.gelu_backward(x.to(dt) + b.to(dt), gy.to(dt))))
    big = (x + b).abs() > 6
    assert torch.equal(y.cpu()[big & (x + b > 0)], (x + b)[big & (x + b > 0)]) and float(y.cpu()[big & (x + b < 0)].abs().max()) < 1e-8


def test_rowdot():
    g = torch.Generator().manual_seed(10)
    rows, Cc = 324, 70
    x, w, b, gy = torch.randn(rows, Cc, generator=g), torch.randn(1, Cc, generator=g), torch.randn(1, generator=g), torch.randn(rows, 1, generator=g)
    dx, dw, db, dg = (t.to(DEV) for t in (x, w, b, gy))
    y = nan_dev(rows, 1)
    check(lib().nq_g3d_rowdot_forward(P(dx), P(dw), P(db), rows, Cc, P(y), st()))
    compare("rowdot_forward", y, both(lambda dt: x.to(dt) @ w.to(dt).t() + b.to(dt)))
    scr = torch.empty(int(lib().nq_g3d_rowdot_scratch_floats(rows, Cc)), device=DEV)

    def call():
        outs = nan_dev(rows, Cc), nan_dev(1, Cc), nan_dev(1)
        check(lib().nq_g3d_rowdot_backward(P(dx), P(dw), P(dg), rows, Cc, P(outs[0]), P(outs[1]), P(outs[2]), P(scr), st()))
        return outs
    compare("rowdot_backward x w b", twice(call), both(lambda dt: (gy.to(dt) @ w.to(dt), gy.to(dt).t() @ x.to(dt), gy.to(dt).sum().reshape(1))))


# ---- the molecule size limit ----------------------------------------------------------------------------------------------------------------------------------
def test_molecule_at_and_above_the_size_limit():
    from nabladft_amd import _lib
    limit = int(lib().nq_g3d_max_mol_atoms())
    assert limit >= 256
    d, E = 16, H * 16
    g = torch.Generator().manual_seed(11)
    s = dict(_structure((limit,)), d=d, E=E, scaling=0.25)
    qkv, bias = torch.randn(limit, 3 * E, generator=g), torch.randn(limit * limit, H, generator=g)
    rc, out, lse = _attention_forward(s, qkv.to(DEV), G.to_heads(bias, (limit,)).to(DEV), None, 1.0)
    check(rc)
    compare("attention_forward[limit]", out, both(lambda dt: G.attention(qkv.to(dt), bias.to(dt), s["ptr"], s["pair_ptr"], H, 0.25)))
    # one atom more: refused before any launch, outputs untouched
    over = dict(_structure((limit + 1,)), d=d, E=E, scaling=0.25)
    q2, b2 = torch.zeros(limit + 1, 3 * E, device=DEV), torch.zeros((limit + 1) ** 2 * H, device=DEV)
    rc, out, lse = _attention_forward(over, q2, b2, None, 1.0)
    assert rc == _lib.NQ_ERR_MOL_TOO_LARGE and b"exceeds the limit" in lib().nq_last_error()
    rejected(lambda: rc, out, lse)
    c = dict(over, pos=torch.zeros(limit + 1, 3), z=torch.ones(limit + 1, dtype=torch.long))
    rc, outs = _pair_forward(c, _gauss_params(c))
    assert rc == _lib.NQ_ERR_MOL_TOO_LARGE
    rejected(lambda: rc, *outs)
    import nabladft_amd as nq
    net = nq.Graphormer3D(1, 1, 32, 32, 2, 0.0, 0.0, 0.0, 0.0, 8).to(DEV)
    with pytest.raises(_lib.NablaqError) as e:
        net(nq.Batch(torch.zeros(limit + 1, 3, device=DEV), torch.ones(limit + 1, dtype=torch.long, device=DEV), torch.zeros(limit + 1, dtype=torch.long, device=DEV)))
    assert e.value.code == _lib.NQ_ERR_MOL_TOO_LARGE
