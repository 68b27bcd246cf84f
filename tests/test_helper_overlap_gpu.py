"""Helper launches beside the sweeps (csrc/engine.hip: SideStream in both calls; plan_step's side_fwd / side_geom / side_reduce), the lane-group k_geom_rev
(csrc/edge.hip) and the batched loads of k_embed_grad_partial (csrc/node.hip).

None of these changes an operation or the order of a sum, so every comparison here is bit for bit:
  * the whole step with the side stream on (NQ_SIDE_STREAM=1) and off (=0), three runs with it on (a missing event wait shows as run-to-run differences);
  * forces of the lane-group k_geom_rev against the one-thread-per-atom flavour (NQ_GEOM_REV_SERIAL=1);
  * the embedding gradient against float32 additions in the kernel's order on the CPU.
The one exception is stated where it is made (test_mixed_path: the rbf_proj gradient of the pair-row kernels against that of the per-molecule kernel)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import painn_ref as R
from tests.test_engine_gpu import _dev, _model

pytestmark = pytest.mark.gpu

SWITCHES = ("NQ_SIDE_STREAM", "NQ_MOLGW", "NQ_NO_MOLGW", "NQ_MOLGW_CAP", "NQ_NO_FUSED_FILTER", "NQ_NO_LITE", "NQ_NO_LAYER0", "NQ_NO_TOPLAYER", "NQ_NO_FUSED_UPDATE",
            "NQ_NO_SIDE_FWD", "NQ_NO_SIDE_GEOM", "NQ_NO_SIDE_REDUCE", "NQ_GEOM_REV_SERIAL")


@contextmanager
def _env(**kw):
    """The engine reads its switches with getenv at every call: exactly `kw` of them set while the block runs, the caller's values afterwards."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in kw.items()})
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _step_arrays(step, batch, **env):
    with _env(**env):
        loss = float(step(batch, update=False))
        torch.cuda.synchronize()
    return {"loss": np.float32(loss), "energy": step.energy.cpu().numpy().copy(), "forces": step.forces.cpu().numpy().copy(), "grad": step.grad.cpu().numpy().copy()}


def _assert_same(a, b, what):
    for k in ("loss", "energy", "forces", "grad"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs ({int(np.sum(np.asarray(a[k]) != np.asarray(b[k])))} elements)"


# ---- the whole step, full configuration, 12 synthetic conformers --------------------------------------------------------------------------------------
_FULL = {}


def _full():
    """Model, batch and step of the full F = 128 / L = 6 configuration, and the per-molecule path's result with the side stream off (computed once)."""
    if not _FULL:
        import nabladft_amd as nq
        from nabladft_amd.synth import gen_conformers
        dev = _dev()
        cfg = R.PaiNNConfig()
        assert (cfg.hidden_channels, cfg.num_layers) == (128, 6)
        model = _model(cfg, R.make_params(cfg, seed=7), dev)
        pos, z, bt, y, ft = gen_conformers(2024, 12)
        sizes = torch.bincount(bt)
        _FULL.update(model=model, batch=nq.Batch(pos, z, bt, y, ft).to(dev), step=nq.FusedTrainStep(model, max_grad_norm=0.0), largest=int(sizes.max()),
                     smallest=int(sizes.min()))
        _FULL["molgw_off"] = _step_arrays(_FULL["step"], _FULL["batch"], NQ_MOLGW=1, NQ_SIDE_STREAM=0)
    return _FULL


def _on_off_three_times(extra, what):
    c = _full()
    off = _step_arrays(c["step"], c["batch"], NQ_SIDE_STREAM=0, **extra)
    runs = [_step_arrays(c["step"], c["batch"], NQ_SIDE_STREAM=1, **extra) for _ in range(3)]
    for i, r in enumerate(runs):
        _assert_same(off, r, f"{what}: side stream off vs on (run {i})")
    return off


def test_side_stream_on_and_off():
    """NQ_MOLGW=1: the pair schedule, the pair geometry records and k_gwr_mol_reduce run (and move to the side stream with everything else)."""
    off = _on_off_three_times({"NQ_MOLGW": 1}, "per-molecule path")
    _assert_same(_full()["molgw_off"], off, "per-molecule path, side stream off, repeated")
    # each group of moved launches alone on the main stream: the same bits
    c = _full()
    for sw in ("NQ_NO_SIDE_FWD", "NQ_NO_SIDE_GEOM", "NQ_NO_SIDE_REDUCE"):
        _assert_same(off, _step_arrays(c["step"], c["batch"], NQ_MOLGW=1, NQ_SIDE_STREAM=1, **{sw: 1}), sw)


def test_mixed_path():
    """NQ_MOLGW_CAP below the largest molecule: the mixed dispatch, which keeps every launch on the main stream.  Side stream on / off / three runs: bit for bit.
    Against the per-molecule path of test_side_stream_on_and_off: loss, energies, forces and every gradient but rbf_proj's bit for bit (they do not depend on the
    dispatch); the rbf_proj gradient of the molecules above the cap comes from the exact-f32 pair-row contraction instead of the split-bf16 one (hi hi' + hi lo' +
    lo hi', <= 3 x 2^-18 per product), so it agrees to 5e-6 of its largest entry, the bound tests/test_engine_gpu.py sets for the same pair of paths."""
    c = _full()
    cap = (c["largest"] + c["smallest"]) // 2
    assert c["smallest"] <= cap < c["largest"]
    mixed = _on_off_three_times({"NQ_MOLGW": 1, "NQ_MOLGW_CAP": cap}, "mixed path")
    ref = c["molgw_off"]
    for k in ("loss", "energy", "forces"):
        assert np.array_equal(mixed[k], ref[k]), k
    for (name, _), (o, n, _s) in zip(c["model"].named_parameters(), c["model"]._param_slices):
        a, b = mixed["grad"][o:o + n], ref["grad"][o:o + n]
        if "rbf_proj" in name:
            e = float(np.abs(a.astype(np.float64) - b).max() / max(float(np.abs(b).max()), 1e-30))
            print(f"mixed vs per-molecule {name}: {e:.2e}")
            assert e < 5e-6, (name, e)
        else:
            assert np.array_equal(a, b), name


def test_small_batch_path():
    """Without NQ_MOLGW (about 500 atoms: pair rows): the forward fork carries the transposes, the pre-splits and the zero fills only, the backward fork the
    tangent zero fills, whose first readers are the general dual kernels of layer 0."""
    _on_off_three_times({}, "pair-row path")
    _on_off_three_times({"NQ_NO_LITE": 1}, "pair-row path, full dual sweep")


# ---- k_geom_rev ---------------------------------------------------------------------------------------------------------------------------------------
def _four_molecules():
    """One atom (an empty row), a pair, 17 atoms (a lane group not filled), a compact 70-atom cluster with every pair inside the cutoff (rows of 69 slots:
    more than two 32-lane chunks, more than one 64-lane chunk).  90 atoms: no multiple of the 8 lane groups of a workgroup."""
    rng = np.random.Generator(np.random.PCG64(70))
    one = np.zeros((1, 3))
    pair = np.array([[0.0, 0.0, 0.0], [1.1, 0.2, -0.3]])
    chain = np.stack([np.arange(17) * 1.3, np.sin(np.arange(17)) * 0.8, np.cos(np.arange(17) * 1.7) * 0.8], 1)
    grid = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3)[:70] * 0.78   # extent 3.12 x 3.12 x 1.56: diagonal 4.68
    cluster = grid + rng.uniform(-0.05, 0.05, size=grid.shape)
    sizes = [1, 2, 17, 70]
    pos = np.concatenate([one, pair, chain, cluster]).astype(np.float32)
    bt = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)]).astype(np.int64)
    z = rng.choice([1, 6, 7, 8], size=len(pos)).astype(np.int64)
    y = rng.normal(size=len(sizes)).astype(np.float32)
    ft = rng.normal(0, 0.05, size=pos.shape).astype(np.float32)
    return tuple(torch.tensor(a) for a in (pos, z, bt, y, ft))


@pytest.mark.parametrize("F", [64, 128])   # one GEDGE plane; two (below 2048 atoms a 128-channel row runs as two slices)
def test_geom_rev_lane_groups_equal_the_serial_kernel(F):
    import nabladft_amd as nq
    dev = _dev()
    pos, z, bt, y, ft = _four_molecules()
    cfg = R.PaiNNConfig(hidden_channels=F, num_layers=2, num_rbf=32)
    ei, _, _ = R.build_graph(pos, bt, cfg.cutoff, cfg.max_neighbors)
    deg = torch.bincount(ei[1], minlength=len(pos)).numpy()
    assert len(pos) == 90 and len(pos) % 8 != 0
    assert deg[0] == 0 and (deg[1:3] == 1).all() and 0 < deg[3:20].max() < 32 and (deg[20:] == 69).all(), deg
    model = _model(cfg, R.make_params(cfg, seed=F), dev)
    batch = nq.Batch(pos, z, bt, y, ft).to(dev)
    assert np.array_equal(model.generate_graph_values(batch)[0].cpu().numpy(), ei.numpy())
    step = nq.FusedTrainStep(model, max_grad_norm=0.0)
    serial = _step_arrays(step, batch, NQ_GEOM_REV_SERIAL=1)
    groups = _step_arrays(step, batch)
    assert np.abs(serial["forces"]).max() > 0 and np.all(serial["forces"].reshape(-1, 3)[0] == 0)   # the lone atom: no edge, no force
    _assert_same(serial, groups, f"F={F}: serial vs lane-group k_geom_rev")


# ---- k_embed_grad_partial -----------------------------------------------------------------------------------------------------------------------------
EMB_CHUNK_SMALL = 32   # csrc/node.hip emb_chunk(): max(32, min(512, ceil(N / 256))) atoms per workgroup


@pytest.mark.parametrize("N", [2 * EMB_CHUNK_SMALL - 1, 2 * EMB_CHUNK_SMALL, 2 * EMB_CHUNK_SMALL + 1])
def test_embedding_gradient_in_the_kernels_order(N):
    """Chunks of 32 atoms: 32 + 31 (three batches of eight loads and a tail of seven), 32 + 32, 32 + 32 + 1 (a chunk that is all tail).  Per chunk and element
    type one float32 accumulator takes the atoms' rows in ascending order (index_add_ on the CPU adds in index order); the two or three per-chunk slabs are then
    summed by k_reduce_partials, which for fewer than four slabs is (p0 + p1) + p2.  Additions only: nothing to contract.  Element types 1, 6, 7, 8 of 100:
    the other rows of the gradient are exact zeros."""
    import nabladft_amd as nq
    dev = _dev()
    rng = np.random.Generator(np.random.PCG64(N))
    sizes = [N - 40, 23, 17]
    pos = np.concatenate([rng.uniform(0, (n ** (1 / 3)) * 1.7 + 1.0, size=(n, 3)) for n in sizes]).astype(np.float32)
    bt = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)]).astype(np.int64)
    z = rng.choice([1, 6, 7, 8], size=N).astype(np.int64)
    cfg = R.PaiNNConfig(hidden_channels=128, num_layers=2, num_rbf=32)
    model = _model(cfg, R.make_params(cfg, seed=N), dev)
    batch = nq.Batch(torch.tensor(pos), torch.tensor(z), torch.tensor(bt), torch.tensor(rng.normal(size=3).astype(np.float32)),
                     torch.tensor(rng.normal(0, 0.05, size=pos.shape).astype(np.float32))).to(dev)
    step = nq.FusedTrainStep(model, max_grad_norm=0.0)
    with _env():
        step(batch, update=False)
        torch.cuda.synchronize()
        gx = model.workspace_view("gx", 0).reshape(N, cfg.hidden_channels).cpu()
    T, F = cfg.num_elements, cfg.hidden_channels
    slabs = []
    for n0 in range(0, N, EMB_CHUNK_SMALL):
        n1 = min(N, n0 + EMB_CHUNK_SMALL)
        slabs.append(torch.zeros(T, F).index_add_(0, torch.tensor(z[n0:n1] - 1), gx[n0:n1]))
    assert len(slabs) in (2, 3)
    ref = slabs[0] + slabs[1]
    if len(slabs) == 3:
        ref = ref + slabs[2]
    names = [k for k, _ in model.named_parameters()]
    o, n, _s = model._param_slices[names.index("atom_emb.embeddings.weight")]
    got = step.grad[o:o + n].reshape(T, F).cpu()
    assert float(gx.abs().max()) > 0
    untouched = np.setdiff1d(np.arange(T), np.unique(z) - 1)
    assert len(untouched) >= T - 4 and bool((got[untouched] == 0).all())
    assert np.array_equal(got.numpy(), ref.numpy()), f"N={N}: {int((got != ref).sum())} of {T * F} entries differ, max {float((got - ref).abs().max()):.3e}"
