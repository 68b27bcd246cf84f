"""GPU parity tests (run with -m gpu on an MI355X): the HIP engine, called through the C ABI, against
  * the golden vectors produced by the real reference (tests/golden/*.npz), and
  * the CPU oracle (oracle/painn_ref.py, oracle/painn_sweeps.py) on the same seeded inputs,
plus size-independent properties at larger batch sizes.
Tolerances (fp32): energies/forces 1e-5 relative (north-star), gradients 5e-5 relative to the
tensor's max, integer outputs and edge geometry bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import painn_ref as R
from oracle.painn_sweeps import Sweeps, loss_and_seeds
from tests.helpers import assert_close, GOLDEN, check_grads, load_case, rel_err

pytestmark = pytest.mark.gpu

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")


def _ulp_close(got, ref, max_ulp, min_exact_frac=0.97):
    """Float geometry check.  The reference's CPU edge_dist comes from torch's vectorised sqrt (SLEEF, <= 0.5001 ulp),
    which is not correctly rounded in ~0.5 % of cases, while the kernel uses IEEE sqrt/div: require agreement within
    `max_ulp` units in the last place everywhere and bit-equality for the overwhelming majority."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape
    if got.size == 0:
        return True
    ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    small = np.abs(ref) < 1e-30
    return bool((ulp[~small] <= max_ulp).all() and (np.abs(got[small]) < 1e-30).all() and (ulp == 0).mean() >= min_exact_frac)


def _ieee_geometry(pos, edge_index):
    """edge_dist / edge_vector of the reference formulas (painn.py:418-420, 319-321) evaluated in IEEE float32 by numpy:
    one correctly rounded operation at a time, ((dx^2+dy^2)+dz^2), sqrt, division.  The kernel must match this bit for bit;
    torch's CPU sqrt is only faithful (<=1 ulp) and differs between machines, so it is compared with a 1-ulp tolerance."""
    p = np.asarray(pos, np.float32)
    j, i = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    w = (p[i] - p[j]).astype(np.float32)
    d2 = ((w[:, 0] * w[:, 0]).astype(np.float32) + (w[:, 1] * w[:, 1]).astype(np.float32)).astype(np.float32)
    d2 = (d2 + (w[:, 2] * w[:, 2]).astype(np.float32)).astype(np.float32)
    d = np.sqrt(d2).astype(np.float32)
    den = (d + np.where(d <= 1e-6, np.float32(1e-6), np.float32(0))).astype(np.float32)
    v = ((p[j] - p[i]).astype(np.float32) / den[:, None]).astype(np.float32)
    return d, v


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _model(cfg, params, dev):
    import nabladft_amd as nq
    m = nq.PaiNN(cfg.hidden_channels, cfg.num_layers, cfg.num_rbf, cfg.cutoff, cfg.max_neighbors, {"name": cfg.rbf},
                 {"name": "polynomial", "exponent": cfg.envelope_exponent} if cfg.envelope_exponent > 0 else {"name": "exponential"},
                 True, cfg.direct_forces, False, True, cfg.num_elements)
    missing, unexpected = m.load_state_dict(params, strict=False)
    assert list(missing) == (["radial_basis.rbf.offset"] if cfg.rbf == "gaussian" else []) and not unexpected
    return m.to(dev)


def _batch(fx, dev):
    from nabladft_amd import Batch
    return Batch(torch.tensor(fx["pos"]), torch.tensor(fx["z"]), torch.tensor(fx["batch"]), torch.tensor(fx["y"]),
                 torch.tensor(fx["f_target"])).to(dev)


# ------------------------------------------------------------------------------------------------
def test_library_is_loaded_native():
    from nabladft_amd import _lib
    lib = _lib.load()
    assert lib.nq_abi_version() == _lib.ABI_VERSION
    with open("/proc/self/maps") as f:
        assert "libnablaq.so" in f.read()


@pytest.mark.parametrize("M,N,K", [(300, 384, 100), (1000, 128, 128), (257, 64, 128), (129, 384, 20), (4096, 256, 128), (77, 128, 256),
                                   (500, 1, 64), (501, 2, 64), (333, 64, 64), (1000, 3, 128),
                                   (40000, 256, 128), (33100, 128, 100), (16500, 384, 128),       # >= 256 tiles of 128x128: the large-tile kernels
                                   (5000, 32, 5376), (3000, 8320, 128), (17000, 128, 2048)])       # long contractions, few tiles: split-K forward / input gradient
def test_gemm_forward_and_grads(M, N, K):
    from nabladft_amd import _lib
    lib, dev = _lib.load(), _dev()
    tol = 2e-6 if max(K, N) <= 512 else 6e-6          # f32 accumulation error grows with the contraction length (5376 / 8320 terms here)
    g = torch.Generator().manual_seed(M * 7 + N)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    G = torch.randn(M, N, generator=g)
    Ad, Wd, bd, Gd = A.to(dev), W.to(dev), b.to(dev), G.to(dev)
    Cd, Sd = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    st = _lib.stream_ptr()
    _lib.check(lib.nq_linear_forward(_lib.ptr(Ad), _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(Cd), _lib.ptr(Sd), M, N, K, st))
    ref = (A.double() @ W.double().T + b.double())
    assert rel_err(Cd.cpu().numpy(), ref.numpy()) < tol
    assert rel_err(Sd.cpu().numpy(), torch.nn.functional.silu(ref).numpy()) < tol
    # transpose-detecting: asymmetric operands above; no-bias / no-silu variant
    _lib.check(lib.nq_linear_forward(_lib.ptr(Ad), _lib.ptr(Wd), None, _lib.ptr(Cd), None, M, N, K, st))
    assert rel_err(Cd.cpu().numpy(), (A.double() @ W.double().T).numpy()) < tol
    # input gradient, with and without accumulation
    Xd = torch.full((M, K), 0.5, device=dev)
    _lib.check(lib.nq_linear_input_grad(_lib.ptr(Gd), _lib.ptr(Wd), _lib.ptr(Xd), M, N, K, 1, st))
    refx = G.double() @ W.double() + 0.5
    assert rel_err(Xd.cpu().numpy(), refx.numpy()) < tol
    _lib.check(lib.nq_linear_input_grad(_lib.ptr(Gd), _lib.ptr(Wd), _lib.ptr(Xd), M, N, K, 0, st))
    assert rel_err(Xd.cpu().numpy(), (G.double() @ W.double()).numpy()) < tol
    # weight gradient (split-K over rows)
    scr = torch.empty(lib.nq_weight_grad_scratch_floats(M, N, K), device=dev)
    gW = torch.empty(N, K, device=dev)
    _lib.check(lib.nq_linear_weight_grad(_lib.ptr(Gd), _lib.ptr(Ad), _lib.ptr(gW), M, N, K, _lib.ptr(scr), st))
    assert rel_err(gW.cpu().numpy(), (G.double().T @ A.double()).numpy()) < 1.5 * tol


@pytest.mark.parametrize("M,N,K", [(1000, 128, 128), (130, 68, 36), (70000, 256, 128), (5000, 512, 256), (257, 3, 64)])
def test_gemm_fused_epilogues(M, N, K):
    """Dense + ScaledSiLU + residual (forward) and the two adjoint epilogues of the input-gradient product, ragged and multi-tile shapes
    (70000 x 256: every persistent workgroup walks several tiles; N = 3: the generic kernel)."""
    from nabladft_amd import _lib
    lib, dev = _lib.load(), _dev()
    g = torch.Generator().manual_seed(M + 3 * N + K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1
    R, G = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    aux = torch.randn(M, K, generator=g)
    Ad, Wd, Rd, Gd, auxd = A.to(dev), W.to(dev), R.to(dev), G.to(dev), aux.to(dev)
    pre, act = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    st = _lib.stream_ptr()
    ref = A.double() @ W.double().T
    for resid in (Rd, None):
        _lib.check(lib.nq_linear_forward_act(_lib.ptr(Ad), _lib.ptr(Wd), _lib.ptr(pre), _lib.ptr(act), None if resid is None else _lib.ptr(resid), 0.75, 1.25, M, N, K, st))
        want = 1.25 * torch.nn.functional.silu(ref) + (0.75 * R.double() if resid is not None else 0.0)
        assert rel_err(pre.cpu().numpy(), ref.numpy()) < 2e-6
        assert rel_err(act.cpu().numpy(), want.numpy()) < 2e-6
    gx = torch.empty(M, K, device=dev)
    refx = G.double() @ W.double()
    _lib.check(lib.nq_linear_input_grad_epi(_lib.ptr(Gd), _lib.ptr(Wd), _lib.ptr(gx), M, N, K, _lib.ptr(auxd), 0.0, 0.6, 1, st))
    z = aux.double()
    sg = torch.sigmoid(z)
    assert rel_err(gx.cpu().numpy(), (0.6 * refx * (sg * (1 + z * (1 - sg)))).numpy()) < 3e-6
    _lib.check(lib.nq_linear_input_grad_epi(_lib.ptr(Gd), _lib.ptr(Wd), _lib.ptr(gx), M, N, K, _lib.ptr(auxd), 0.7, 0.0, 2, st))
    assert rel_err(gx.cpu().numpy(), (0.7 * z + refx).numpy()) < 2e-6


def test_gemm_rows_do_not_depend_on_the_batch():
    """A row's result is the same whatever else is in the batch as long as the same engine runs (fixed k order, no split over K on the forward layouts):
    the exact-f32 engine picks 64x64 or 128x128 tiles from the problem size, both must produce identical bits; the split-bf16 engine (large problems only)
    is identical between two large batches; across the two engines the rows agree to f32 rounding."""
    from nabladft_amd import _lib
    lib, dev = _lib.load(), _dev()
    g = torch.Generator().manual_seed(5)
    A, W = torch.randn(50000, 128, generator=g).to(dev), (torch.randn(256, 128, generator=g) * 0.1).to(dev)
    st = _lib.stream_ptr()

    def run(rows):
        out = torch.empty(rows, 256, device=dev)
        _lib.check(lib.nq_linear_forward(_lib.ptr(A), _lib.ptr(W), None, _lib.ptr(out), None, rows, 256, 128, st))
        return out
    big, mid, small = run(50000), run(30000), run(700)            # split-bf16, split-bf16, exact-f32 (64x64 tiles)
    assert torch.equal(big[:30000], mid)
    ref = A[:700].double() @ W.double().T
    e_split, e_f32 = float((big[:700].double() - ref).abs().max()), float((small.double() - ref).abs().max())
    assert e_split <= 1.5 * e_f32 + 1e-7 and e_f32 < 5e-6 * float(ref.abs().max()), (e_split, e_f32)
    lib.nq_set_gemm_variant(1 | 32)                                  # every product on v_mfma_f32_32x32x2_f32
    try:
        big32 = run(50000)
    finally:
        lib.nq_set_gemm_variant(1)
    assert torch.equal(big32[:700], small)


def test_split_bf16_engine_matches_float64_like_the_exact_engine():
    """gemm_split.h: f32 values split exactly into three bf16 pieces, six piece products per product on the bf16 matrix pipe.  Against float64 on every layout
    (forward with bias + SiLU, input gradient with accumulate, weight gradient with the bias gradient) the error must not exceed the exact-f32 engine's;
    ragged sizes (tile tails in M, N and K), wide dynamic range in the operands."""
    from nabladft_amd import _lib
    lib, dev = _lib.load(), _dev()
    g = torch.Generator().manual_seed(11)
    M, N, K = 40000 + 37, 380, 132
    scale = torch.exp(4.0 * torch.randn(M, 1, generator=g))         # rows over ~7 decades
    A = (torch.randn(M, K, generator=g) * scale).to(dev)
    W, b = (torch.randn(N, K, generator=g) * 0.2).to(dev), torch.randn(N, generator=g).to(dev)
    G = (torch.randn(M, N, generator=g) * scale).to(dev)
    st = _lib.stream_ptr()

    def all_products():
        pre, act = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        _lib.check(lib.nq_linear_forward(_lib.ptr(A), _lib.ptr(W), _lib.ptr(b), _lib.ptr(pre), _lib.ptr(act), M, N, K, st))
        gx = torch.ones(M, K, device=dev)
        _lib.check(lib.nq_linear_input_grad(_lib.ptr(G), _lib.ptr(W), _lib.ptr(gx), M, N, K, 1, st))
        scr = torch.empty(lib.nq_weight_grad_scratch_floats(M, N, K) + 64, device=dev)
        gW = torch.empty(N, K, device=dev)
        _lib.check(lib.nq_linear_weight_grad(_lib.ptr(G), _lib.ptr(A), _lib.ptr(gW), M, N, K, _lib.ptr(scr), st))
        return pre, act, gx, gW
    split = all_products()
    lib.nq_set_gemm_variant(1 | 32)
    try:
        exact = all_products()
    finally:
        lib.nq_set_gemm_variant(1)
    Ad, Wd, Gd = A.double(), W.double(), G.double()
    pre = Ad @ Wd.T + b.double()
    refs = (pre, torch.nn.functional.silu(pre), 1.0 + Gd @ Wd, Gd.T @ Ad)
    for name, s_, e_, r in zip(("forward", "silu", "input gradient", "weight gradient"), split, exact, refs):
        rowmax = r.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
        es, ee = float(((s_.double() - r).abs() / rowmax).max()), float(((e_.double() - r).abs() / rowmax).max())
        assert not torch.equal(s_, e_), name                         # the two engines really are different code paths
        assert es <= 1.25 * ee + 1e-7 and es < 2e-5, (name, es, ee)


def test_weight_grad_many_rows_deterministic():
    from nabladft_amd import _lib
    lib, dev = _lib.load(), _dev()
    rows, N, K = 70001, 384, 100
    g = torch.Generator().manual_seed(1)
    G, X = torch.randn(rows, N, generator=g).to(dev), torch.randn(rows, K, generator=g).to(dev)
    scr = torch.empty(lib.nq_weight_grad_scratch_floats(rows, N, K), device=dev)
    o1, o2 = torch.empty(N, K, device=dev), torch.empty(N, K, device=dev)
    st = _lib.stream_ptr()
    _lib.check(lib.nq_linear_weight_grad(_lib.ptr(G), _lib.ptr(X), _lib.ptr(o1), rows, N, K, _lib.ptr(scr), st))
    _lib.check(lib.nq_linear_weight_grad(_lib.ptr(G), _lib.ptr(X), _lib.ptr(o2), rows, N, K, _lib.ptr(scr), st))
    assert torch.equal(o1, o2)
    ref = (G.double().T @ X.double()).cpu()
    assert rel_err(o1.cpu().numpy(), ref.numpy()) < 5e-6


# ------------------------------------------------------------------------------------------------
def test_graph_cases_bit_exact():
    import nabladft_amd as nq
    dev = _dev()
    gx = np.load(GOLDEN + "/graph_cases.npz")
    for c in range(int(gx["n_cases"])):
        pre = f"c{c}_"
        pos, batch = torch.tensor(gx[pre + "pos"]).to(dev), torch.tensor(gx[pre + "batch"]).to(dev)
        nl = nq.build_neighbor_list(pos, batch, None, float(gx[pre + "cutoff"]), int(gx[pre + "K"]), canonical=True)
        assert np.array_equal(nl.edge_index.cpu().numpy(), gx[pre + "edge_index"]), f"case {c} edge_index"
        assert np.array_equal(nl.neighbors.cpu().numpy(), gx[pre + "neighbors"]), f"case {c} neighbors"
        assert np.array_equal(nl.id_swap.cpu().numpy(), gx[pre + "id_swap"]), f"case {c} id_swap"
        assert _ulp_close(nl.edge_dist.cpu().numpy(), gx[pre + "edge_dist"], 1), f"case {c} edge_dist"
        assert _ulp_close(nl.edge_vector.cpu().numpy(), gx[pre + "edge_vector"], 2), f"case {c} edge_vector"
        d_ieee, v_ieee = _ieee_geometry(gx[pre + "pos"], gx[pre + "edge_index"])
        assert np.array_equal(nl.edge_dist.cpu().numpy(), d_ieee) and np.array_equal(nl.edge_vector.cpu().numpy(), v_ieee), f"case {c} IEEE"
        # CSR invariants: sorted sources per row, rev is an involution that flips (col, dst)
        col, dst, rev, rp = (nl.t[k].cpu().long() for k in ("col", "dst", "rev", "row_ptr"))
        assert torch.equal(rev[rev], torch.arange(nl.E))
        assert torch.equal(col[rev], dst) and torch.equal(dst[rev], col)
        assert torch.equal(torch.repeat_interleave(torch.arange(nl.N), rp[1:] - rp[:-1]), dst)
        same_row = dst[1:] == dst[:-1]
        assert bool((col[1:][same_row] > col[:-1][same_row]).all())
        s2c = nl.t["slot2canon"].cpu().long()
        assert torch.equal(torch.tensor(gx[pre + "edge_index"])[0][s2c], col)
        assert torch.equal(torch.tensor(gx[pre + "edge_index"])[1][s2c], dst)


def test_graph_errors():
    import nabladft_amd as nq
    from nabladft_amd._lib import NablaqError
    dev = _dev()
    pos = torch.rand(600, 3, device=dev) * 30
    with pytest.raises(NablaqError):  # molecule larger than NQ_MAX_MOL_ATOMS
        nq.build_neighbor_list(pos, torch.zeros(600, dtype=torch.long, device=dev), None, 5.0, 100)
    m = nq.PaiNN(64, 1, 8, 0.5, 10, {"name": "gaussian"}, {"name": "polynomial", "exponent": 5}, True, False, False, True, 10).to(dev)
    far = nq.Batch(torch.tensor([[0.0, 0, 0], [9.0, 0, 0]], device=dev), torch.tensor([1, 1], device=dev), torch.tensor([0, 0], device=dev))
    with pytest.raises(IndexError):  # the reference raises IndexError in repeat_blocks when no edge exists
        m(far)


# ------------------------------------------------------------------------------------------------
def _trace_report(name, model, sw, s2c, tag, lines):
    """Compares every named engine buffer with the CPU sweeps; returns worst relative error."""
    L, worst = model.num_layers, 0.0
    node_bufs = ["x_in", "vec_in", "z1", "h", "xh", "x_msg", "vec_msg", "u", "s", "cat", "zq", "q", "y"]
    for tangent in ([False, True] if tag == "bwd" else [False]):
        pre = "t_" if tangent else ""
        for l in range(L):
            for b in node_bufs:
                key = f"{pre}{b}{l}" if b in ("x_in", "vec_in", "x_msg", "vec_msg") else f"{pre}{b}_{l}"
                if key not in sw.ws:
                    continue
                ref = sw.ws[key].reshape(-1).numpy()
                got = model.workspace_view(b, l, tangent).cpu().numpy()
                e = rel_err(got, ref)
                worst = max(worst, e)
                lines.append(f"{name} {tag} {key:14s} rel_err {e:.3e}")
            if not tangent and os.environ.get("NQ_NO_FUSED_FILTER") == "1":
                for b in ("phi", "psi"):
                    ref = sw.ws[f"{b}_{l}"][s2c].reshape(-1).numpy()
                    got = model.workspace_view(b, l).cpu().numpy()
                    e = rel_err(got, ref)
                    worst = max(worst, e)
                    lines.append(f"{name} {tag} {b}_{l:<10d} rel_err {e:.3e}")
    if os.environ.get("NQ_NO_FUSED_FILTER") == "1":
        for b, key in (("rho", "rho"), ("rho", "drho")):
            ref = sw.ws[key][s2c].reshape(-1).numpy()
            got = model.workspace_view("rho", 0, key == "drho").cpu().numpy()
            e = rel_err(got, ref)
            worst = max(worst, e)
            lines.append(f"{name} {tag} {key:14s} rel_err {e:.3e}")
    elif os.environ.get("NQ_NO_MOLGW") != "1" and tag == "fwd":
        _check_pair_schedule(model, int(os.environ.get("NQ_MOLGW_CAP", "0")) or None)
    elif os.environ.get("NQ_NO_MOLGW") == "1":
        # k0-sorted order of the LOWER CSR slots (col < dst: one gphi / gpsi row per pair): every lower slot once, keys non-decreasing, stable
        nl = model._last_nl
        lower = torch.nonzero(nl.t["col"].cpu() < nl.t["dst"].cpu()).view(-1)
        assert lower.numel() * 2 == nl.E
        order = model.workspace_view("order").cpu().view(torch.int32).long()[:lower.numel()]
        k0s = model.workspace_view("rw").cpu().view(-1, 32)[:, 13].contiguous().view(torch.int32).long()
        assert torch.equal(torch.sort(order).values, lower)
        assert bool((k0s[order][1:] >= k0s[order][:-1]).all())
        same = k0s[order][1:] == k0s[order][:-1]
        assert bool((order[1:][same] > order[:-1][same]).all()), "sort must be stable"
    if os.environ.get("NQ_NO_FUSED_FILTER") != "1":
        # fused filter: per-edge 13-tap window record {rho[13], k0, ., ., drho[13]} must reproduce the full basis row
        rw = model.workspace_view("rw").cpu().view(-1, 32)
        k0 = rw[:, 13].contiguous().view(torch.int32).long()
        R_ = sw.ws["rho"].shape[1]
        nwin = min(13, R_)
        for key, off in (("rho", 0), ("drho", 16)):
            full = torch.zeros(rw.shape[0], R_ + 13)
            idx = k0[:, None] + torch.arange(13)[None, :]
            full.scatter_(1, idx, rw[:, off:off + 13])
            ref = sw.ws[key][s2c]
            e = rel_err(full[:, :R_].numpy(), ref.numpy())
            worst = max(worst, e)
            lines.append(f"{name} {tag} window {key:8s} rel_err {e:.3e} (dropped tail included)")
    if tag == "bwd":
        for b in ("t_d", "t_r"):
            ref = sw.ws[b][s2c].reshape(-1).numpy()
            got = model.workspace_view(b).cpu().numpy()
            e = rel_err(got, ref)
            worst = max(worst, e)
            lines.append(f"{name} {tag} {b:14s} rel_err {e:.3e}")
    return worst


def _lds_cap():
    """nq_painn_molecule_lds_atoms(): the largest molecule the per-molecule rbf_proj gradient kernel stages in LDS."""
    from nabladft_amd import _lib
    return int(_lib.load().nq_painn_molecule_lds_atoms())


def _check_pair_schedule(model, cap=None):
    """Pair lists of the molecule-per-workgroup rbf_proj gradient (csrc/molpair.hip): every lower CSR slot (col < dst) of a molecule of <= cap atoms exactly
    once, inside its molecule's batches; entries sorted by window start k0, slot-ascending among equal k0; the wavefront segments tile the molecule's list,
    every segment starts on a batch boundary (8 pair slots) of the padded list and its last batch is padded with -1; every pair sits inside the accumulator
    rows of its wavefront (0 <= k0 - wlo[w] < 19 = the stored row offset) and no segment is longer than ceil(pairs / wavefronts) unless the next wavefront's
    rows cannot hold the surplus; the local atom indices are the slot's (dst, col) relative to the molecule's first atom.  Larger molecules: empty segments.
    The list the workgroups deal molecules from is a permutation ordered by descending pair count."""
    cap = _lds_cap() if cap is None else cap
    nl = model._last_nl
    col, dst = nl.t["col"].cpu().long(), nl.t["dst"].cpu().long()
    lowptr, mol_ptr = nl.t["lowptr"].cpu().long(), nl.t["mol_ptr"].cpu().long()
    WMAX, BATCH = 19, 8
    sched = model.workspace_view("pair_sched").cpu().view(torch.int32).view(-1, 2).long()
    meta = model.workspace_view("pair_sched_meta").cpu().view(torch.int32).long()
    NW = (meta.numel() - 145 - 2 * nl.B) // (3 * nl.B + 1)     # wavefronts per workgroup of k_gwr_mol (csrc/molpair.hip: GM_NW)
    assert NW in (8, 12)
    assert sched.shape[0] == BATCH * ((nl.E // 2) // BATCH + NW * nl.B + NW)
    assert meta.numel() == 2 * nl.B * NW + nl.B * (NW + 1) + 128 + NW + 1 + nl.B + 16
    seg = meta[:2 * nl.B * NW].view(nl.B, NW, 2)
    sp = meta[2 * nl.B * NW:][:nl.B * (NW + 1)].view(nl.B, NW + 1)
    rest = meta[2 * nl.B * NW + nl.B * (NW + 1):]
    hist, wlo = rest[:128], rest[128:][:NW + 1]
    # the deal of molecules to workgroups: a permutation by descending pair count (molecules above the LDS limit count 0), ties by ascending index
    order = rest[128 + NW + 1:][:nl.B]
    natoms_m = mol_ptr[1:] - mol_ptr[:-1]
    npairs = torch.where(natoms_m <= cap, lowptr[mol_ptr[1:]] - lowptr[mol_ptr[:-1]], torch.zeros_like(natoms_m))
    assert torch.equal(torch.sort(order).values, torch.arange(nl.B))
    key = npairs[order] * (nl.B + 1) + (nl.B - order)
    assert bool((key[1:] < key[:-1]).all()), "molecules must be ordered by descending pair count, equal counts by ascending index"
    k0s = model.workspace_view("rw").cpu().view(-1, 32)[:, 13].contiguous().view(torch.int32).long()
    lower = torch.nonzero(col < dst).view(-1)
    assert lower.numel() * 2 == nl.E
    assert torch.equal(torch.bincount(k0s[lower], minlength=128)[:128], hist)
    assert bool((wlo[1:NW] >= wlo[:NW - 1]).all()) and bool((wlo[1:NW] <= wlo[:NW - 1] + WMAX).all())
    assert int(wlo[0]) <= int(k0s[lower].min()) and int(wlo[NW - 1]) + WMAX > int(k0s[lower].max())
    seen = []
    for m in range(nl.B):
        a0, a1 = int(mol_ptr[m]), int(mol_ptr[m + 1])
        pb, pe = int(lowptr[a0]), int(lowptr[a1])
        b0 = (pb >> 3) + NW * m
        if a1 - a0 > cap:
            assert bool((seg[m, :, 1] == 0).all()) and bool((sp[m] == 0).all())
            continue
        assert int(sp[m, 0]) == 0 and int(sp[m, NW]) == pe - pb and bool((sp[m, 1:] >= sp[m, :-1]).all())
        target = -(-(pe - pb) // NW)
        nb_run, sl_all, word_all = 0, [], []
        for w in range(NW):
            fb, ln = int(seg[m, w, 0]), int(seg[m, w, 1])
            assert fb == b0 + nb_run and ln == int(sp[m, w + 1] - sp[m, w])
            nb = -(-ln // BATCH)
            ent = sched[BATCH * fb:BATCH * (fb + nb)]
            assert bool((ent[ln:, 0] == -1).all()), "the last batch of a segment is padded with -1"
            slot, word = ent[:ln, 0], ent[:ln, 1] & 0xFFFFFFFF
            off = word >> 26
            assert torch.equal(off, k0s[slot] - wlo[w]) and bool((off >= 0).all()) and bool((off < WMAX).all())
            if ln > target and w < NW - 1:   # surplus only when forced: those pairs lie below the next wavefront's first row
                assert bool((k0s[slot][target:] < wlo[w + 1]).all())
            sl_all.append(slot); word_all.append(word)
            nb_run += nb
        if m + 1 < nl.B:
            assert b0 + nb_run <= (int(lowptr[mol_ptr[m + 1]]) >> 3) + NW * (m + 1), "a molecule's batches must end before the next molecule's first batch"
        sl, word = torch.cat(sl_all), torch.cat(word_all)
        k = k0s[sl]
        assert bool((dst[sl] >= a0).all()) and bool((dst[sl] < a1).all())
        assert bool((k[1:] >= k[:-1]).all()) and bool((sl[1:][k[1:] == k[:-1]] > sl[:-1][k[1:] == k[:-1]]).all())
        assert torch.equal((word >> 13) & 0x1FFF, dst[sl] - a0) and torch.equal(word & 0x1FFF, col[sl] - a0)
        seen.append(sl)
    seen = torch.sort(torch.cat(seen)).values if seen else torch.zeros(0, dtype=torch.long)
    natoms = (mol_ptr[1:] - mol_ptr[:-1])
    small_atom = (natoms <= cap)[nl.t["atom_mol"].cpu().long()]
    assert torch.equal(seen, lower[small_atom[dst[lower]]])


@pytest.mark.parametrize("fused", ["fused", "fused_mixed", "fused_pair_rows", "materialised"])
@pytest.mark.parametrize("name", ["painn_small_ragged.npz", "painn_full_real4.npz", "painn_small_expenv.npz"])
def test_engine_matches_reference_golden(name, fused, monkeypatch):
    """fused: radial filter evaluated inside the message kernels (WrT in LDS, 13-Gaussian window), rbf_proj gradient from node rows staged per molecule in
    LDS (csrc/molpair.hip); fused_mixed: the same batch with the LDS limit lowered to the batch's median molecule size, so that about half of the molecules take
    the per-molecule kernel and the others the pair rows INSIDE one step (the dispatch of molecules above the LDS limit); fused_pair_rows: gphi / gpsi pair rows
    through HBM for every molecule; materialised: fallback path (phi/psi through the GEMM) used when WrT does not fit the LDS."""
    if fused == "materialised":
        monkeypatch.setenv("NQ_NO_FUSED_FILTER", "1")
    else:
        monkeypatch.delenv("NQ_NO_FUSED_FILTER", raising=False)
    monkeypatch.delenv("NQ_MOLGW_CAP", raising=False)
    if fused == "fused_mixed":
        fx0 = load_case(name)[0]
        counts = np.bincount(fx0["batch"])
        cap = int(np.sort(counts)[(len(counts) - 1) // 2])
        if cap >= counts.max():
            pytest.skip("all molecules of this fixture have one size")
        monkeypatch.setenv("NQ_MOLGW_CAP", str(cap))
    if fused == "fused_pair_rows":
        monkeypatch.setenv("NQ_NO_MOLGW", "1")
        monkeypatch.delenv("NQ_MOLGW", raising=False)
    else:
        monkeypatch.delenv("NQ_NO_MOLGW", raising=False)
        monkeypatch.setenv("NQ_MOLGW", "1")   # the golden batches are small: force the per-molecule path (default from 4096 atoms per step)
    name_tag = f"{name}.{fused}"
    dev = _dev()
    fx, cfg, params = load_case(name)
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    lines = []
    # graph: bit-exact against the reference
    ei, nb, ed, ev, sw_ = model.generate_graph_values(batch)
    assert np.array_equal(ei.cpu().numpy(), fx["edge_index"])
    assert np.array_equal(nb.cpu().numpy(), fx["neighbors"])
    assert np.array_equal(sw_.cpu().numpy(), fx["id_swap"])
    assert _ulp_close(ed.cpu().numpy(), fx["edge_dist"], 1)
    assert _ulp_close(ev.cpu().numpy(), fx["edge_vector"], 2)
    # forward + forces through the autograd boundary
    model.train()
    energy, forces = model(batch)
    s2c = model._last_nl.t["slot2canon"].cpu().long()
    # CPU sweeps on the same inputs (buffer-by-buffer localisation)
    sw = Sweeps(params, cfg, torch.tensor(fx["pos"]), torch.tensor(fx["z"]), torch.tensor(fx["batch"]), torch.tensor(fx["edge_index"]))
    e_cpu, f_cpu = sw.energy_forces()
    worst_f = _trace_report(name, model, sw, s2c, "fwd", lines)
    e_err, f_err = rel_err(energy.detach().cpu().numpy(), fx["energy"]), rel_err(forces.detach().cpu().numpy(), fx["forces"])
    lines.append(f"{name} energy rel_err {e_err:.3e}  forces rel_err {f_err:.3e}  worst fwd buffer {worst_f:.3e}")
    # loss + backward exactly as PaiNNLightning.step / Lightning do it
    from nabladft_amd import L2Loss
    loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
    loss.backward()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    loss_cpu, gE, gF = loss_and_seeds(e_cpu, f_cpu, torch.tensor(fx["y"]), torch.tensor(fx["f_target"]))
    G = sw.backward(gE, gF)
    worst_b = _trace_report(name, model, sw, s2c, "bwd", lines)
    g_worst = max(rel_err(grads[k], G[k].numpy()) for k in G)
    lines.append(f"{name} loss {float(loss):.7f} (golden {float(fx['loss']):.7f})  worst bwd buffer {worst_b:.3e}  worst grad vs sweeps {g_worst:.3e}")
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"trace_{name_tag}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert e_err < 1e-5 and f_err < 1e-5, lines[-2]
    assert_close(f"painn golden {name} E", energy.detach().cpu().numpy(), fx["energy"], 1e-5)        # array-level and element-wise (|a-b| <= 1e-5 max(|b|, rms b))
    assert_close(f"painn golden {name} F", forces.detach().cpu().numpy(), fx["forces"], 1e-5)
    assert abs(float(loss) - float(fx["loss"])) < 1e-5 * abs(float(fx["loss"]))
    assert rel_err(model.workspace_view("x_msg", 0).cpu().numpy(), fx["x_msg0"].reshape(-1)) < 1e-5
    Lm = cfg.num_layers
    assert rel_err(model.workspace_view("x_in", Lm).cpu().numpy(), fx[f"x_upd{Lm - 1}"].reshape(-1)) < 1e-5
    assert rel_err(model.workspace_view("vec_in", Lm).cpu().numpy(), fx[f"vec_upd{Lm - 1}"].reshape(-1)) < 1e-5
    worst = check_grads(fx, grads, 5e-5, name)
    with open(os.path.join(OUT, f"trace_{name_tag}.txt"), "a") as f:
        f.write(f"worst grad vs golden: {worst}\n")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["painn_full_real4.npz", "painn_small_ragged.npz"])
def test_second_order_sweep_with_stored_tangent_adjoints_equals_the_full_dual_sweep(name, monkeypatch):
    """csrc/engine.hip (round 6): the tangent adjoints of the second-order sweep obey the force sweep's recursion with the same seeds, so the force sweep stores
    its per-layer adjoints and the second-order sweep reads them (input-gradient products, SiLU reverse and the GT* stores run over / touch the primal-adjoint
    half only).  NQ_NO_LITE=1 keeps the full stacked sweep of rounds 1-5.  Both must give the reference's gradients (golden vectors, the bounds of
    test_engine_matches_reference_golden) and agree with each other to f32 rounding; energies and forces are bitwise equal (the force sweep computes the same
    values, only into other buffers)."""
    import nabladft_amd as nq
    from nabladft_amd import L2Loss
    dev = _dev()
    fx, cfg, params = load_case(name)
    res = {}
    for mode in ("stored", "full"):
        if mode == "full":
            monkeypatch.setenv("NQ_NO_LITE", "1")
        else:
            monkeypatch.delenv("NQ_NO_LITE", raising=False)
        model = _model(cfg, params, dev)
        batch = _batch(fx, dev)
        model.train()
        energy, forces = model(batch)
        loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
        loss.backward()
        grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
        check_grads(fx, grads, 5e-5, f"second-order sweep ({mode} tangent adjoints)")
        res[mode] = (energy.detach().cpu(), forces.detach().cpu(), grads)
    assert torch.equal(res["stored"][0], res["full"][0]) and torch.equal(res["stored"][1], res["full"][1])
    for k in res["full"][2]:
        a, b = res["stored"][2][k], res["full"][2][k]
        assert float(np.abs(a - b).max()) <= 2e-5 * max(float(np.abs(b).max()), 1e-30), k


@pytest.mark.parametrize("mode", ["unfused", "fused_forward"])
def test_update_block_flavours_agree_with_the_reference(mode, monkeypatch):
    """csrc/updfuse.hip: the update block of a layer's forward sweep as ONE kernel (hidden_channels = 128) against the five launches it replaces and against
    the reference golden vectors of the full configuration: energies, forces, loss and every parameter gradient within the bounds of
    test_engine_matches_reference_golden, for the default (fused forward sweep) and the unfused path; the fused kernel is seen by the profiler when and only
    when it is selected."""
    import nabladft_amd as nq
    from nabladft_amd import L2Loss
    monkeypatch.delenv("NQ_NO_FUSED_UPDATE", raising=False)
    if mode == "unfused":
        monkeypatch.setenv("NQ_NO_FUSED_UPDATE", "1")
    dev = _dev()
    fx, cfg, params = load_case("painn_full_real4.npz")
    assert cfg.hidden_channels == 128
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    model.train()
    out = {}

    def run():
        for p in model.parameters():
            p.grad = None
        energy, forces = model(batch)
        loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
        loss.backward()
        out["e"], out["f"], out["loss"] = energy.detach(), forces.detach(), float(loss.detach())
    names = _kernel_names_of(run)
    assert ("upd_fused" in names) == (mode != "unfused"), names
    assert "upd_a" in names, names                                                  # the tangent sweep runs the five launches either way
    assert_close(f"update block {mode} E", out["e"].cpu().numpy(), fx["energy"], 1e-5)
    assert_close(f"update block {mode} F", out["f"].cpu().numpy(), fx["forces"], 1e-5)
    assert abs(out["loss"] - float(fx["loss"])) < 1e-5 * abs(float(fx["loss"]))
    check_grads(fx, {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}, 5e-5, f"update block {mode}")
    e1, f1 = out["e"].clone(), out["f"].clone()
    run()
    assert torch.equal(e1, out["e"]) and torch.equal(f1, out["f"])                  # deterministic


def test_backward_follows_the_plan_of_its_forward_call(monkeypatch):
    """Every path choice of a training step is made by nq_painn_forward and recorded for the workspace: switches changed between the forward and the backward
    call leave the gradients bitwise unchanged, and a backward call with the graph of another batch is refused (NQ_ERR_ARG) before any device work."""
    import nabladft_amd as nq
    from nabladft_amd import L2Loss, _lib
    lib = _lib.load()
    dev = _dev()
    fx, cfg, params = load_case("painn_full_real4.npz")
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    keep = fx["batch"] < fx["batch"].max()                     # another batch: the same conformers but the last
    other = nq.Batch(torch.tensor(fx["pos"][keep]), torch.tensor(fx["z"][keep]), torch.tensor(fx["batch"][keep])).to(dev)
    model.train()
    switches = ("NQ_NO_FUSED_FILTER", "NQ_NO_MOLGW", "NQ_MOLGW", "NQ_MOLGW_CAP", "NQ_NO_LITE")

    def step(forward_env, backward_env):
        for k in switches:
            monkeypatch.delenv(k, raising=False)
        for k, v in forward_env.items():
            monkeypatch.setenv(k, v)
        for p in model.parameters():
            p.grad = None
        energy, forces = model(batch)
        loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
        for k in switches:
            monkeypatch.delenv(k, raising=False)
        for k, v in backward_env.items():
            monkeypatch.setenv(k, v)
        loss.backward()
        return {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    flipped = {"NQ_NO_FUSED_FILTER": "1", "NQ_NO_MOLGW": "1", "NQ_MOLGW_CAP": "4", "NQ_NO_LITE": "1"}
    refs = []
    for forward_env, backward_env in (({}, {**flipped, "NQ_MOLGW": "1"}),                          # pair rows, stored adjoints
                                      ({"NQ_MOLGW": "1"}, flipped),                                # per-molecule rbf_proj gradient
                                      ({"NQ_MOLGW": "1", "NQ_MOLGW_CAP": "4"}, flipped)):          # mixed batch
        ref = step(forward_env, forward_env)
        got = step(forward_env, backward_env)
        refs.append(ref)
        for k in ref:
            assert torch.equal(ref[k], got[k]), (forward_env, k)
    check_grads(fx, {k: g.cpu().numpy() for k, g in got.items()}, 5e-5, "plan of the forward call")
    for k in switches:
        monkeypatch.delenv(k, raising=False)

    with torch.no_grad():
        model(other)
    nl_other = model._last_nl
    g_other = nl_other.c
    energy, forces = model(batch)                              # the same cached workspace, now prepared for `batch`
    ws, nl = model._last_ws, model._last_nl
    assert (g_other.N, g_other.E, g_other.B) != (nl.c.N, nl.c.E, nl.c.B)
    grad = torch.empty_like(model._flat)
    rc = lib.nq_painn_backward(C.byref(model._cfg), _lib.ptr(model._flat), _lib.ptr(model.radial_basis.engine_buffer()), C.byref(g_other), _lib.ptr(ws),
                               ws.numel(), None, None, _lib.ptr(grad), _lib.stream_ptr())
    assert rc == 2 and b"different model or batch" in lib.nq_last_error()
    loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
    for p in model.parameters():
        p.grad = None
    loss.backward()                                            # the refused call left the step intact
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, refs[0][k]), k


def test_fused_step_matches_golden_and_is_deterministic():
    """C-ABI-only path (HIP loss kernel, no autograd): same gradients, bitwise reproducible."""
    import nabladft_amd as nq
    dev = _dev()
    fx, cfg, params = load_case("painn_full_real4.npz")
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    step = nq.FusedTrainStep(model, max_grad_norm=0.0)
    l1 = float(step(batch, update=False))
    g1, e1, f1 = step.grad.clone(), step.energy.clone(), step.forces.clone()
    l2 = float(step(batch, update=False))
    assert l1 == l2 and torch.equal(g1, step.grad) and torch.equal(e1, step.energy) and torch.equal(f1, step.forces)
    assert abs(l1 - float(fx["loss"])) < 1e-5 * abs(float(fx["loss"]))
    grads = {k: g1[o:o + n].view(s).cpu().numpy() for (k, _), (o, n, s) in zip(model.named_parameters(), model._param_slices)}
    check_grads(fx, grads, 5e-5, "fused")


def test_loss_kernel_and_adamw_match_torch():
    from nabladft_amd import _lib
    lib, dev = _lib.load(), _dev()
    g = torch.Generator().manual_seed(3)
    B, N = 37, 1500
    E, y = torch.randn(B, generator=g), torch.randn(B, generator=g)
    F_, Ft = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    loss_ref, gE_ref, gF_ref = loss_and_seeds(E, F_, y, Ft, 0.7, 1.3)
    out, gE, gF = torch.zeros(1, device=dev), torch.empty(B, device=dev), torch.empty(N, 3, device=dev)
    st = _lib.stream_ptr()
    Ed, yd, Fd, Ftd = E.to(dev), y.to(dev), F_.to(dev), Ft.to(dev)  # keep the device copies alive across the launch
    _lib.check(lib.nq_loss_l1_l2(_lib.ptr(Ed), _lib.ptr(yd), B, _lib.ptr(Fd), _lib.ptr(Ftd), N, 0.7, 1.3,
                                 _lib.ptr(out), _lib.ptr(gE), _lib.ptr(gF), st))
    assert abs(float(out) - float(loss_ref)) < 1e-5 * abs(float(loss_ref))
    assert rel_err(gE.cpu().numpy(), gE_ref.numpy()) < 1e-6 and rel_err(gF.cpu().numpy(), gF_ref.numpy()) < 1e-5
    # clip + AdamW, three steps, against torch
    P = 100003
    p0, grads = torch.randn(P, generator=g), [torch.randn(P, generator=g) * 0.05 for _ in range(3)]
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=5e-4, weight_decay=0.01)
    pd, m, v = p0.clone().to(dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    scr = torch.empty(512, device=dev)
    for t, gr in enumerate(grads, 1):
        pt.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_([pt], 5.0)
        opt.step()
        grd = gr.to(dev)
        _lib.check(lib.nq_adamw_step(_lib.ptr(pd), _lib.ptr(grd), _lib.ptr(m), _lib.ptr(v), P, 5.0, 5e-4, 0.9, 0.999, 1e-8, 0.01, t,
                                     _lib.ptr(scr), st))
        torch.cuda.synchronize()
    assert rel_err(pd.cpu().numpy(), pt.detach().numpy()) < 1e-6


# ------------------------------------------------------------------------------------------------
def _rand_rotation(seed):
    q, _ = np.linalg.qr(np.random.Generator(np.random.PCG64(seed)).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return torch.tensor(q.astype(np.float32))


def test_properties_full_size_batch():
    """Size-independent properties at a BASELINE-sized batch (64 drug-like conformers, full config):
    batching invariance, E(3) invariance/equivariance, zero net force, determinism, oracle agreement."""
    import nabladft_amd as nq
    dev = _dev()
    cfg = R.PaiNNConfig()
    params = R.make_params(cfg, seed=23)
    model = _model(cfg, params, dev).eval()
    pos, z, batch, y, ft = R.gen_conformers(1, 64)
    full = nq.Batch(pos, z, batch, y, ft).to(dev)
    with torch.no_grad():
        e, f = model(full)
        e2, f2 = model(full)
    assert torch.equal(e, e2) and torch.equal(f, f2)
    # oracle on a slice (first 6 molecules) at full config
    sel = batch < 6
    e_ref, f_ref = R.energy_forces(params, cfg, pos[sel], z[sel], batch[sel])
    assert rel_err(e[:6].cpu().numpy(), e_ref.numpy()) < 1e-5
    assert rel_err(f[sel.to(dev)].cpu().numpy(), f_ref.numpy()) < 1e-5
    # batching invariance: every molecule evaluated alone gives the same energy/forces
    for mol in (0, 17, 63):
        s = batch == mol
        one = nq.Batch(pos[s], z[s], torch.zeros(int(s.sum()), dtype=torch.long)).to(dev)
        with torch.no_grad():
            e1, f1 = model(one)
        assert rel_err(e1.cpu().numpy(), e[mol:mol + 1].cpu().numpy()) < 2e-6
        assert rel_err(f1.cpu().numpy(), f[s.to(dev)].cpu().numpy()) < 1e-5
    # net force per molecule vanishes (translation invariance)
    net = torch.zeros(64, 3, device=dev).index_add_(0, full.batch, f)
    assert float(net.abs().max()) < 2e-4 * float(f.abs().max())
    # rotation + translation: E invariant, F rotates
    Rm = _rand_rotation(5)
    rot = nq.Batch(pos @ Rm.T + torch.tensor([1.5, -2.0, 0.7]), z, batch).to(dev)
    with torch.no_grad():
        er, fr = model(rot)
    assert rel_err(er.cpu().numpy(), e.cpu().numpy()) < 2e-5
    assert rel_err(fr.cpu().numpy(), (f.cpu() @ Rm.T).numpy()) < 5e-5


def test_training_reduces_loss():
    """A few fused steps on a fixed batch must lower the loss (end-to-end sanity of grads + optimizer)."""
    import nabladft_amd as nq
    dev = _dev()
    cfg = R.PaiNNConfig(hidden_channels=64, num_layers=3, num_rbf=20)
    model = _model(cfg, R.make_params(cfg, seed=2), dev)
    pos, z, batch, y, ft = R.gen_conformers(4, 8)
    b = nq.Batch(pos, z, batch, y, ft).to(dev)
    step = nq.FusedTrainStep(model, lr=2e-3)
    losses = [float(step(b)) for _ in range(30)]
    assert losses[-1] < 0.7 * losses[0], losses


@pytest.mark.parametrize("fused", ["fused", "materialised"])
def test_dense_molecules_long_rows(fused, monkeypatch):
    """Rows longer than one wavefront (degree up to 99 > 64 -> chunked row loop), K binding (max_neighbors=40 < degree),
    a 300-atom molecule (5 adjacency words per row) next to a 2-atom one; full train step vs the CPU oracle."""
    import nabladft_amd as nq
    if fused == "materialised":
        monkeypatch.setenv("NQ_NO_FUSED_FILTER", "1")
    else:
        monkeypatch.delenv("NQ_NO_FUSED_FILTER", raising=False)
    dev = _dev()
    rng = np.random.Generator(np.random.PCG64(77))
    sizes = [100, 2, 300, 70]
    pos = np.concatenate([rng.uniform(0, (n ** (1 / 3)) * 1.9 + 1.0, size=(n, 3)) for n in sizes]).astype(np.float32)
    batch = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)]).astype(np.int64)
    z = rng.choice([1, 6, 7, 8], size=len(pos)).astype(np.int64)
    y = rng.normal(size=len(sizes)).astype(np.float32)
    ft = rng.normal(0, 0.05, size=pos.shape).astype(np.float32)
    for K in (100, 40):
        cfg = R.PaiNNConfig(hidden_channels=64, num_layers=2, num_rbf=24, cutoff=6.0, max_neighbors=K)
        params = R.make_params(cfg, seed=4)
        for k in params:  # keep activations O(1) at degree ~60
            if "rbf_proj" in k or "x_proj.2" in k:
                params[k] = params[k] * 0.3
        tp, tz, tb = torch.tensor(pos), torch.tensor(z), torch.tensor(batch)
        ei, nb, sw = R.build_graph(tp, tb, cfg.cutoff, cfg.max_neighbors)
        deg = torch.bincount(ei[1], minlength=len(pos))
        assert int(deg.max()) > 64 if K == 100 else True
        model = _model(cfg, params, dev)
        b = nq.Batch(tp, tz, tb, torch.tensor(y), torch.tensor(ft)).to(dev)
        gi = model.generate_graph_values(b)
        assert np.array_equal(gi[0].cpu().numpy(), ei.numpy()) and np.array_equal(gi[1].cpu().numpy(), nb.numpy())
        e_ref, f_ref, loss_ref, g_ref = R.train_step(params, cfg, tp, tz, tb, torch.tensor(y), torch.tensor(ft), ei)
        step = nq.FusedTrainStep(model, max_grad_norm=0.0)
        loss = float(step(b, update=False))
        assert rel_err(step.energy.cpu().numpy(), e_ref.numpy()) < 1e-5, (K, fused)
        assert rel_err(step.forces.cpu().numpy(), f_ref.numpy()) < 2e-5, (K, fused)
        assert abs(loss - float(loss_ref)) < 1e-5 * abs(float(loss_ref))
        for (k, _), (o, n, s) in zip(model.named_parameters(), model._param_slices):
            assert rel_err(step.grad[o:o + n].view(s).cpu().numpy(), g_ref[k].numpy()) < 1e-4, (K, fused, k)


def test_graph_large_molecule_matches_oracle():
    """Neighbour list of molecules close to the 512-atom LDS limit (8 adjacency words per row) vs the oracle, bit-exact indices."""
    import nabladft_amd as nq
    dev = _dev()
    rng = np.random.Generator(np.random.PCG64(5))
    sizes = [512, 1, 449, 64, 65]
    pos = torch.tensor(np.concatenate([rng.uniform(0, 14.0, size=(n, 3)) for n in sizes]).astype(np.float32))
    batch = torch.tensor(np.concatenate([np.full(n, i) for i, n in enumerate(sizes)]).astype(np.int64))
    for cutoff, K in ((3.0, 100), (4.5, 7)):
        ei, nb, sw = R.build_graph(pos, batch, cutoff, K)
        nl = nq.build_neighbor_list(pos.to(dev), batch.to(dev), None, cutoff, K, canonical=True)
        assert np.array_equal(nl.edge_index.cpu().numpy(), ei.numpy())
        assert np.array_equal(nl.neighbors.cpu().numpy(), nb.numpy())
        assert np.array_equal(nl.id_swap.cpu().numpy(), sw.numpy())
        d, v = _ieee_geometry(pos.numpy(), ei.numpy())
        assert np.array_equal(nl.edge_dist.cpu().numpy(), d) and np.array_equal(nl.edge_vector.cpu().numpy(), v)   # bit-exact IEEE
        dt, vt = R.edge_geometry(pos, ei)                                                                            # torch CPU: faithful
        assert _ulp_close(nl.edge_dist.cpu().numpy(), dt.numpy(), 1, 0.5) and _ulp_close(nl.edge_vector.cpu().numpy(), vt.numpy(), 2, 0.5)


@pytest.mark.parametrize("name", ["painn_small_bessel.npz", "painn_small_bernstein.npz"])
def test_engine_learnable_bases_match_reference(name):
    """SphericalBesselBasis / BernsteinBasis (layers.py:51-126, row a4b): non-compact, learnable bases run on the materialised-filter
    path; golden vectors from the real reference incl. the gradients of the basis parameters (frequencies [R] / pregamma)."""
    from nabladft_amd import L2Loss
    dev = _dev()
    fx, cfg, params = load_case(name)
    model = _model(cfg, params, dev)
    batch = _batch(fx, dev)
    model.train()
    energy, forces = model(batch)
    e_err, f_err = rel_err(energy.detach().cpu().numpy(), fx["energy"]), rel_err(forces.detach().cpu().numpy(), fx["forces"])
    assert e_err < 2e-6 and f_err < 2e-5, (e_err, f_err)
    loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
    loss.backward()
    assert abs(float(loss) - float(fx["loss"])) < 1e-5 * abs(float(fx["loss"]))
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    basis = [k for k in grads if k.startswith("radial_basis.rbf.")]
    assert len(basis) == 1 and "grad:" + basis[0] in fx
    worst = check_grads(fx, grads, 1e-4, name)
    print(f"{name}: energy {e_err:.2e} forces {f_err:.2e} worst grad {worst[0]:.2e} ({worst[1]}); d{basis[0]}: "
          f"{rel_err(grads[basis[0]], fx['grad:' + basis[0]]):.2e}")


def test_engine_direct_forces_match_reference():
    """direct_forces=True (row a10): forces from the PaiNNOutput head (two gated equivariant blocks, painn.py:551-620) on the engine's final
    node state, first-order backward seeded with the head's adjoints; golden vectors from the real reference."""
    from nabladft_amd import L2Loss
    dev = _dev()
    fx, cfg, params = load_case("painn_small_direct.npz")
    assert cfg.direct_forces
    model = _model(cfg, params, dev)
    assert [n for n, _ in model.named_parameters()] == [k for k, _ in R.param_shapes(cfg)]
    batch = _batch(fx, dev)
    model.train()
    energy, forces = model(batch)
    assert forces.shape == (batch.pos.shape[0], 3)
    e_err, f_err = rel_err(energy.detach().cpu().numpy(), fx["energy"]), rel_err(forces.detach().cpu().numpy(), fx["forces"])
    assert e_err < 2e-6 and f_err < 2e-5, (e_err, f_err)
    loss = torch.nn.L1Loss()(energy, batch.y) + L2Loss()(forces, batch.forces)
    loss.backward()
    assert abs(float(loss) - float(fx["loss"])) < 1e-5 * abs(float(fx["loss"]))
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    worst = check_grads(fx, grads, 1e-4, "direct")
    print(f"direct forces: energy {e_err:.2e} forces {f_err:.2e} worst grad {worst[0]:.2e} ({worst[1]})")
    model.eval()                                   # inference: same outputs, no graph
    with torch.no_grad():
        e2, f2 = model(batch)
    assert torch.equal(e2, energy.detach()) and torch.equal(f2, forces.detach())


@pytest.mark.parametrize("n_conf", [1, 2, 3, 5, 9, 17, 40, 300])   # 300: > 4096 atoms -> rows claimed from counters
def test_every_row_is_processed_at_any_grid_size(n_conf):
    """Row claiming (edge.hip FUSED_ROWS): whatever the number of workgroups per XCD, every atom row is computed exactly once --
    energies, forces and all parameter gradients of small batches against the CPU oracle."""
    import nabladft_amd as nq
    dev = torch.device("cuda:0")
    cfg = R.PaiNNConfig(num_layers=2)
    params = R.make_params(cfg, seed=5)
    m = nq.PaiNN(cfg.hidden_channels, 2, cfg.num_rbf, cfg.cutoff, cfg.max_neighbors, {"name": "gaussian"}, {"name": "polynomial", "exponent": 5},
                 True, False, False, True, cfg.num_elements)
    m.load_state_dict(params, strict=False)
    m.to(dev)
    pos, z, batch, y, ft = R.gen_conformers(100 + n_conf, n_conf, size=(5, 30))
    e, f = m(nq.Batch(pos, z, batch).to(dev))
    loss = (e - y.to(dev)).abs().mean() + (f - ft.to(dev)).pow(2).sum(-1).sqrt().mean()
    loss.backward()
    e_ref, f_ref, loss_ref, g_ref = R.train_step(params, cfg, pos, z, batch, y, ft)
    assert rel_err(e.detach().cpu().numpy(), e_ref.numpy()) < 1e-5 and rel_err(f.detach().cpu().numpy(), f_ref.numpy()) < 1e-5
    assert abs(float(loss) - float(loss_ref)) < 1e-5 * abs(float(loss_ref))
    for k, p in m.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), g_ref[k].numpy()) < 5e-5, k


def test_one_large_molecule_in_a_300_conformer_batch_takes_the_pair_rows_alone(monkeypatch):
    """one molecule above the LDS limit of k_gwr_mol (62 atoms) used to send the WHOLE step back to the pair-row path.  300 conformers
    (> 4096 atoms: the default per-molecule path) with ONE 70-atom molecule in the middle: against the CPU oracle, against the pair rows forced for every
    molecule, and the schedule shows the 299 others on the per-molecule kernel (non-empty segments) and the large one with none."""
    import nabladft_amd as nq
    dev = torch.device("cuda:0")
    monkeypatch.delenv("NQ_MOLGW", raising=False); monkeypatch.delenv("NQ_NO_MOLGW", raising=False); monkeypatch.delenv("NQ_MOLGW_CAP", raising=False)
    cfg = R.PaiNNConfig(num_layers=2)
    params = R.make_params(cfg, seed=8)
    m = _model(cfg, params, dev)
    pos, z, batch, y, ft = R.gen_conformers(77, 300, size=(8, 30))
    rng = np.random.Generator(np.random.PCG64(70))
    big = 150
    keep_lo, keep_hi = batch < big, batch >= big
    pos_b = torch.tensor(rng.uniform(0, 8.0, size=(70, 3)).astype(np.float32))
    z_b = torch.tensor(rng.choice([1, 6, 7, 8], size=70).astype(np.int64))
    pos = torch.cat([pos[keep_lo], pos_b, pos[keep_hi]]); z = torch.cat([z[keep_lo], z_b, z[keep_hi]])
    batch = torch.cat([batch[keep_lo], torch.full((70,), big), batch[keep_hi] + 1])
    ft = torch.cat([ft[keep_lo], torch.tensor(rng.normal(0, 0.05, size=(70, 3)).astype(np.float32)), ft[keep_hi]])
    y = torch.cat([y[:big], torch.tensor([0.3]), y[big:]])
    assert int(batch.max()) == 300 and pos.shape[0] > 4096

    def run():
        for p in m.parameters():
            p.grad = None
        e, f = m(nq.Batch(pos, z, batch).to(dev))
        loss = (e - y.to(dev)).abs().mean() + (f - ft.to(dev)).pow(2).sum(-1).sqrt().mean()
        loss.backward()
        return e.detach(), f.detach(), float(loss), {k: p.grad.clone() for k, p in m.named_parameters()}
    names = _kernel_names_of(lambda: run())
    assert {"gwr_mol", "gwr_sorted", "msgf_rev_dual", "msgf_rev_dual_ng"} <= names, names
    e, f, loss, g = run()
    _check_pair_schedule(m)
    meta = m.workspace_view("pair_sched_meta").cpu().view(torch.int32).long()
    NW = (meta.numel() - 145 - 301) // (3 * 301 + 1)
    seg = meta[:2 * 301 * NW].view(301, NW, 2)
    npairs = seg[:, :, 1].sum(1)
    assert int(npairs[big]) == 0 and int((npairs > 0).sum()) == 300
    e_ref, f_ref, loss_ref, g_ref = R.train_step(params, cfg, pos, z, batch, y, ft)
    assert rel_err(e.cpu().numpy(), e_ref.numpy()) < 1e-5 and rel_err(f.cpu().numpy(), f_ref.numpy()) < 1e-5
    assert abs(loss - float(loss_ref)) < 1e-5 * abs(float(loss_ref))
    for k in g:
        assert rel_err(g[k].cpu().numpy(), g_ref[k].numpy()) < 5e-5, k
    monkeypatch.setenv("NQ_NO_MOLGW", "1")
    e2, f2, loss2, g2 = run()
    assert torch.equal(e, e2) and torch.equal(f, f2) and loss == loss2
    for k in g:
        d = float((g[k].double() - g2[k].double()).abs().max() / g2[k].double().abs().max().clamp_min(1e-30))
        assert d < 5e-6, (k, d)
        if "rbf_proj" not in k:
            assert torch.equal(g[k], g2[k]), k


def test_bench_sized_batch_linearity_and_determinism():
    """At the bench.py workload size (2048 conformers, ~86 k atoms, 1.6 M edges, full config) the oracle is out of reach; size-independent
    properties instead: (1) the parameter gradient of a LINEAR functional of energies and forces over the whole batch equals the sum of the
    gradients of eight 256-conformer chunks (molecules do not couple) -- this runs the tangent / dual sweeps, the full-width message rows and the
    per-molecule rbf_proj gradient (k_gwr_mol, the default from 4096 atoms per step) at full size; (2) two runs are bitwise identical; (3) net force
    per molecule vanishes.
    Yardstick for (1): on the exact-f32 engine a row's result does not depend on the batch, so chunks and full batch differ only by the partition of the
    weight-gradient sums: 5e-5 of the tensor's largest entry (measured 2e-6).  With the split-bf16 engine the chunk products partly run on the other
    engine, i.e. intermediate rows differ in the last f32 bit -- and this random-weight model turns last-bit differences of the intermediates into up to
    1e-4 of some weight gradients (measured: two exact-f32 kernels that differ only in the summation order over k are 8e-5 apart on
    update_layers.5.vec_proj.weight, scripts/debug_split_linearity.py).  So the split engine is held to twice that measured f32 reordering
    sensitivity, tensor by tensor, not to an absolute number."""
    import nabladft_amd as nq
    from nabladft_amd import _lib
    dev = _dev()
    cfg = R.PaiNNConfig()
    params = R.make_params(cfg, seed=23)
    model = _model(cfg, params, dev)
    B, C = 2048, 8
    pos, z, batch, _, _ = R.gen_conformers(7, B)
    g = torch.Generator().manual_seed(3)
    w_e, w_f = torch.randn(B, generator=g), torch.randn(pos.shape[0], 3, generator=g)
    names = [k for k, _ in model.named_parameters()]
    sizes = [p.numel() for p in model.parameters()]

    def grads(sel_mol):
        s = (batch >= sel_mol[0]) & (batch < sel_mol[1])
        b = nq.Batch(pos[s], z[s], batch[s] - sel_mol[0]).to(dev)
        for p in model.parameters():
            p.grad = None
        e, f = model(b)
        ((e * w_e[sel_mol[0]:sel_mol[1]].to(dev)).sum() + (f * w_f[s].to(dev)).sum()).backward()
        return torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone(), e.detach(), f.detach(), b

    def per_tensor(a, b_, scale):
        """max |a - b| per parameter tensor, relative to the tensor's largest entry (floored at 1e-3 of the largest gradient entry overall)."""
        out, o = [], 0
        for n in sizes:
            x, y = a[o:o + n].double(), b_[o:o + n].double()
            out.append(float((x - y).abs().max()) / max(float(y.abs().max()), 1e-3 * scale))
            o += n
        return out

    def chunks_vs_full():
        g_full, e, f, full = grads((0, B))
        g_again, e2, f2, _ = grads((0, B))
        assert torch.equal(g_full, g_again) and torch.equal(e, e2) and torch.equal(f, f2)
        acc = torch.zeros_like(g_full, dtype=torch.float64)
        step = B // C
        for c in range(C):
            gc, ec, _, _ = grads((c * step, (c + 1) * step))
            acc += gc.double()
            assert rel_err(ec.cpu().numpy(), e[c * step:(c + 1) * step].cpu().numpy()) < 2e-6
        return g_full, acc, e, f, full

    lib = _lib.load()
    try:
        lib.nq_set_gemm_variant(1 | 32)                      # exact-f32 engine: batch-independent rows
        gx_full, gx_acc, _, _, _ = chunks_vs_full()
        scale = float(gx_full.abs().max())
        assert float((gx_acc - gx_full.double()).abs().max()) < 2e-5 * scale
        for k, d in zip(names, per_tensor(gx_acc, gx_full, scale)):
            assert d <= 5e-5, (k, d)                         # small tensors must not hide behind the largest one
        lib.nq_set_gemm_variant(1 | 16)                      # the generic exact-f32 kernels: same arithmetic, another summation order over k
        gg_full = grads((0, B))[0]
    finally:
        lib.nq_set_gemm_variant(1)
    reorder = per_tensor(gg_full, gx_full, scale)           # what a pure f32 reordering does to each tensor
    g_full, acc, e, f, full = chunks_vs_full()              # default: split-bf16 engine for the large products
    assert float((acc - g_full.double()).abs().max()) < 2e-5 * scale
    # Yardstick per tensor: THREE harmless perturbations of the same step exist here -- another summation order over k on the exact engine (reorder), the
    # split-bf16 engine instead of the exact one (d_engine; since round 6 it includes the fused update block, which only exists on the bf16 matrix pipe and steps
    # aside when the exact engine is requested), and chunks instead of the full batch (d).  Each is one sample of the tensor's sensitivity to last-bit changes of
    # the intermediates; a single sample of it varies 2-3x between runs (measured: reorder of update_layers.5.vec_proj.weight 2.5e-5 / 4.6e-5 / 8e-5), so a sample
    # is held to twice the LARGER of the other two (and the engine difference to four times the reorder sample), not to twice one of them.
    for k, d, d_engine, r in zip(names, per_tensor(acc, g_full, scale), per_tensor(g_full, gx_full, scale), reorder):
        assert d <= max(5e-5, 2.0 * max(r, d_engine)) and d_engine <= max(5e-5, 4.0 * r), (k, d, d_engine, r)
    net = torch.zeros(B, 3, device=dev).index_add_(0, full.batch, f)
    assert float(net.abs().max()) < 5e-4 * float(f.abs().max())


def _kernel_names_of(fn):
    """Names of the engine launches recorded by the C-ABI profiler (nq_profile_enable / nq_profile_read) while fn() runs."""
    import ctypes as C
    from nabladft_amd import _lib
    lib = _lib.load()
    cap = 256
    names = C.create_string_buffer(cap * 64)
    ms = (C.c_double * cap)()
    cnt = (C.c_int64 * cap)()
    lib.nq_profile_read(names, 64, ms, cnt, cap)            # drop what earlier tests left behind
    lib.nq_profile_enable(1)
    try:
        fn()
        n = lib.nq_profile_read(names, 64, ms, cnt, cap)
    finally:
        lib.nq_profile_enable(0)
    return {names.raw[i * 64:(i + 1) * 64].split(b"\0")[0].decode() for i in range(min(n, cap)) if cnt[i] > 0}


@pytest.mark.parametrize("F,NR,sizes", [(64, 20, [1, 2, -1, 9, 30, 44]), (128, 100, [-1, 3, 1, 25, 40, 12, 57]), (256, 50, [5, 31, 2, -2])])   # -1: the LDS limit, -2: one below
def test_per_molecule_weight_gradient_equals_the_pair_row_path(F, NR, sizes, monkeypatch):
    """csrc/molpair.hip against the pair-row path it replaces, same step, same inputs: molecules of 1 and 2 atoms (no pair / one pair: empty wavefront
    segments, batches of padding only), the largest molecule the LDS takes (nq_painn_molecule_lds_atoms(): 62), 2 / 4 / 8 channel slices, 8 / 38 / 88 window starts.  Every gradient
    must agree to the accuracy of the split-bf16 contraction (hi hi' + hi lo' + lo hi', <= 3 x 2^-18 per product; the pair-row path is exact f32), energies and
    forces bit for bit (they do not depend on the path); a molecule one atom above the limit goes through the pair-row kernels while the REST of its batch stays on the
    per-molecule kernel (schedule checked, both kernel families seen by the profiler), same result as forcing the pair rows for everything."""
    import nabladft_amd as nq
    dev = _dev()
    cfg = R.PaiNNConfig(hidden_channels=F, num_layers=2, num_rbf=NR)
    params = R.make_params(cfg, seed=F + NR)
    model = _model(cfg, params, dev)
    rng = np.random.Generator(np.random.PCG64(F))

    def batch_of(sz):
        pos = np.concatenate([rng.uniform(0, (n ** (1 / 3)) * 1.7 + 1.0, size=(n, 3)) for n in sz]).astype(np.float32)
        bt = np.concatenate([np.full(n, i) for i, n in enumerate(sz)]).astype(np.int64)
        z = rng.choice([1, 6, 7, 8], size=len(pos)).astype(np.int64)
        return nq.Batch(torch.tensor(pos), torch.tensor(z), torch.tensor(bt), torch.tensor(rng.normal(size=len(sz)).astype(np.float32)),
                        torch.tensor(rng.normal(0, 0.05, size=pos.shape).astype(np.float32))).to(dev)

    cap = _lds_cap()
    sizes = [cap + 1 + n if n < 0 else n for n in sizes]
    b = batch_of(sizes)
    step = nq.FusedTrainStep(model, max_grad_norm=0.0)
    out = {}
    for path in ("pair_rows", "per_molecule"):
        if path == "per_molecule":
            monkeypatch.setenv("NQ_MOLGW", "1"); monkeypatch.delenv("NQ_NO_MOLGW", raising=False)
        else:
            monkeypatch.setenv("NQ_NO_MOLGW", "1"); monkeypatch.delenv("NQ_MOLGW", raising=False)
        loss = float(step(b, update=False))
        out[path] = (loss, step.energy.clone(), step.forces.clone(), step.grad.clone())
    assert out["pair_rows"][0] == out["per_molecule"][0]
    assert torch.equal(out["pair_rows"][1], out["per_molecule"][1]) and torch.equal(out["pair_rows"][2], out["per_molecule"][2])
    ga, gb = out["pair_rows"][3], out["per_molecule"][3]
    worst = 0.0
    for (k, _), (o, n, s) in zip(model.named_parameters(), model._param_slices):
        a_, b_ = ga[o:o + n].double(), gb[o:o + n].double()
        e = float((a_ - b_).abs().max() / a_.abs().max().clamp_min(1e-30))
        worst = max(worst, e)
        if "rbf_proj" not in k:
            assert torch.equal(ga[o:o + n], gb[o:o + n]), k          # only the rbf_proj gradient is computed differently
        assert e < 5e-6, (k, e)
    # deterministic: the per-molecule path twice
    loss2 = float(step(b, update=False))
    assert loss2 == out["per_molecule"][0] and torch.equal(step.grad, gb)
    # one atom more: does not fit the LDS of one workgroup -> THAT molecule takes the pair rows, the others stay on the per-molecule kernel
    b65 = batch_of([cap + 1, 4, 30, 41])
    monkeypatch.setenv("NQ_MOLGW", "1"); monkeypatch.delenv("NQ_NO_MOLGW", raising=False)
    names = _kernel_names_of(lambda: step(b65, update=False))
    g_auto, e_auto, f_auto = step.grad.clone(), step.energy.clone(), step.forces.clone()
    assert {"gwr_mol", "gwr_sorted", "msgf_rev_dual", "msgf_rev_dual_ng"} <= names, names
    _check_pair_schedule(model)                              # the large molecule: empty segments; the three others: scheduled
    step(b65, update=False)
    assert torch.equal(g_auto, step.grad)                    # deterministic
    monkeypatch.setenv("NQ_NO_MOLGW", "1"); monkeypatch.delenv("NQ_MOLGW", raising=False)
    names = _kernel_names_of(lambda: step(b65, update=False))
    assert "gwr_mol" not in names and "gwr_sorted" in names, names
    assert torch.equal(e_auto, step.energy) and torch.equal(f_auto, step.forces)
    for (k, _), (o, n, s_) in zip(model.named_parameters(), model._param_slices):
        a_, b_ = step.grad[o:o + n].double(), g_auto[o:o + n].double()
        e = float((a_ - b_).abs().max() / a_.abs().max().clamp_min(1e-30))
        worst = max(worst, e)
        assert e < 5e-6, (k, e)
    print(f"molgw vs pair rows F={F} R={NR}: worst relative gradient difference {worst:.2e}")
