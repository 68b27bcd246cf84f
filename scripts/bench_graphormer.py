"""Graphormer3D (config/model/graphormer3d-small.yaml: 4 blocks x 6 shared layers, embed 512, ffn 512, 32 heads of 16, 128 Gaussian kernels; Adam lr 3e-4,
L1 losses with coefficients 1 / 1 in the reference's padded-mean form, gradient clip 5.0; config/graphormer3d.yaml: batch_size 32) training-step timing on one
MI355X in fp32: pair structure -> forward (train mode, with its dropouts) -> losses -> backward -> clip -> Adam, on synthetic ~42-atom conformers already
resident in HBM.  Timed with HIP events over the steps after the warm-up.

    python scripts/bench_graphormer.py [--batches 32 128 512] [--steps 20] [--warmup 3] [--kernels] [--cpu-baseline] [--out profiles/graphormer_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(blocks=4, layers=6, embed_dim=512, ffn_embed_dim=512, attention_heads=32, input_dropout=0.1, dropout=0.1, attention_dropout=0.0,
           activation_dropout=0.1, num_kernel=128)                   # config/model/graphormer3d-small.yaml:5-15
CLIP = 5.0


def synthetic_batch(molecules, seed, device):
    import nabladft_amd as nq
    from nabladft_amd.synth import gen_conformers
    pos, z, batch, y, f = gen_conformers(seed, molecules)
    return nq.Batch(pos, z, batch, y=y, forces=f).to(device)


def build(device, seed=23):
    import torch
    import nabladft_amd as nq
    torch.manual_seed(seed)
    net = nq.Graphormer3D(**CFG).to(device)
    return nq.Graphormer3DLightning("Graphormer3D-small", net, lambda params: torch.optim.Adam(params, lr=3e-4), None, torch.nn.L1Loss(), None, 0, 1.0, 1.0)


def run(molecules=32, steps=20, warmup=3, kernels=True, seed=1):
    import torch
    from nabladft_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    task = build(dev)
    task.train()
    params = list(task.parameters())
    opt = task.configure_optimizers()["optimizer"]
    batches = [synthetic_batch(molecules, seed * 100 + k, dev) for k in range(4)]
    for b in batches:
        b.prepared = task.net.prepare(b)                     # once per composition (the data loader's job)

    def step(i):
        opt.zero_grad(set_to_none=True)
        loss = task.step(batches[i % len(batches)])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()
        return loss

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(steps):
        loss = step(i)
    stop.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop) / steps
    plan = batches[0].prepared
    out = {"molecules_per_step": molecules, "ms_per_step": ms, "value": molecules / ms * 1e3, "unit": "conformer-steps/s", "atoms": plan.N, "pairs": plan.P,
           "peak_memory_MiB": torch.cuda.max_memory_allocated() / 2 ** 20, "final_loss": float(loss.detach()), "steps": steps, "dtype": "f32", "data": "synthetic"}
    if kernels:
        _lib.profile_enable(True)
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        _lib.profile_enable(False)
        ks = sorted(((k, v[0] / steps, v[1] // steps) for k, v in prof.items()), key=lambda x: -x[1])
        dense = sum(v[0] for v in prof.values() if v[2] > 0) / steps
        new = sum(v[0] for k, v in prof.items() if k.startswith("g3d_")) / steps
        total = sum(v[0] for v in prof.values()) / steps
        out.update(device_ms_per_step_nq_kernels=total, dense_products_ms_per_step=dense, graphormer_kernels_ms_per_step=new, other_nq_kernels_ms_per_step=total - dense - new,
                   dense_TFLOPs=sum(v[2] for v in prof.values()) / steps / max(dense, 1e-9) / 1e9,
                   kernel_ms_per_step={k: [round(t, 4), int(n)] for k, t, n in ks[:24]})
    return out


def cpu_baseline(conformers=2, budget=40.0):
    """The float64 restatement (tests/graphormer_ref.py) run in float32 on at most 16 threads: forward + loss + backward, eval mode, no optimizer step."""
    import torch
    from nabladft_amd.synth import gen_conformers
    from tests import graphormer_ref as G
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    pos, z, batch, y, f = gen_conformers(101, conformers)
    sizes = tuple(torch.bincount(batch).tolist())
    cfg = {k: CFG[k] for k in ("blocks", "layers", "embed_dim", "ffn_embed_dim", "attention_heads", "num_kernel")}
    params = {k: v.float() for k, v in G.make_params(cfg, 0).items()}
    b = dict(z=z, pos=pos.float(), y=y.float(), forces=f.float(), sizes=sizes)
    times, t_start = [], time.perf_counter()
    while True:
        t0 = time.perf_counter()
        G.loss_and_grads(params, cfg, b)
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - t_start > budget or len(times) >= 6:
            break
    timed = times[1:] if len(times) > 1 else times
    dt = sorted(timed)[len(timed) // 2] / conformers
    return {"value": 1.0 / dt, "unit": "conformer-steps/s", "cores": cores, "kind": "restatement",
            "sample": f"{conformers} synthetic conformers ({pos.shape[0]} atoms), yaml configuration, forward + loss + backward of tests/graphormer_ref.py in float32, "
                      f"median of {len(timed)} steps after one warm-up step, torch {torch.__version__} CPU, no optimizer step"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 128, 512])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"workload": "Graphormer3D (config/model/graphormer3d-small.yaml) train step: forward, L1(E) + L1(F, padded mean), backward, clip 5.0, Adam; synthetic "
                       "~42-atom conformers; HIP events over the timed steps", "runs": [run(m, a.steps, a.warmup, a.kernels) for m in a.batches]}
    if a.cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
