"""DimeNet++ (config/model/dimenetplusplus.yaml: hidden 256, 6 blocks, int_emb 64, basis_emb 8, out_emb 256, 7 spherical x 6 radial, 32 neighbours, cutoff 5 A)
timing on one MI355X in fp32, on synthetic ~42-atom conformers already resident in HBM, with HIP events over the steps after the warm-up:
  * the energy + force call (what the test / predict / optimize jobs run): graph, forward, one backward to the positions;
  * the energy-loss training step: graph, forward, the force backward, L1(E), backward to the parameters, Adam;
  * with --force-loss, the force-loss training step of DimeNetPlusPlusForceLightning (the yaml's coefficients 1 and 1): graph, forward, the force backward with
    its graph kept, L1(E) + L1(F), the second sweep to the parameters, Adam; the table gives the share of the two tangent triplet kernels.

    python scripts/bench_dimenet.py [--batches 32 128 512] [--steps 10] [--warmup 2] [--kernels] [--cpu-baseline] [--out profiles/dimenet_bench.json]
    python scripts/bench_dimenet.py --kernels --force-loss --out profiles/dimenet_force_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(node_latent_dim=50, dimenet_hidden_channels=256, dimenet_num_blocks=6, dimenet_int_emb_size=64, dimenet_basis_emb_size=8, dimenet_out_emb_channels=256,
           dimenet_num_spherical=7, dimenet_num_radial=6, dimenet_max_num_neighbors=32, cutoff=5.0)
TANGENT = ("dn_triplet_tan_fwd", "dn_triplet_tan_bwd")
TRIPLET = ("dn_triplet_fwd", "dn_triplet_bwd") + TANGENT


def synthetic_batch(molecules, seed, device):
    import nabladft_amd as nq
    from nabladft_amd.synth import gen_conformers
    pos, z, batch, y, f = gen_conformers(seed, molecules)
    return nq.Batch(pos, z, batch, y=y, forces=f).to(device)


def build(device, seed=23, force_loss=False):
    import torch
    import nabladft_amd as nq
    from tests import dimenet_ref as D
    torch.manual_seed(seed)
    net = nq.DimeNetPlusPlusPotential(**CFG)
    net.load_state_dict({k: v.float() for k, v in D.make_params(CFG, 0).items()})      # the default initialisation has a zero output layer: no force signal
    cls, cf = (nq.DimeNetPlusPlusForceLightning, 1.0) if force_loss else (nq.DimeNetPlusPlusLightning, 0.0)
    return cls(net=net.to(device), loss=torch.nn.L1Loss(), metric=None, energy_loss_coef=1.0, forces_loss_coef=cf, optimizer=lambda p: torch.optim.Adam(p, lr=1e-4))


def timed(fn, steps, warmup):
    import torch
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(steps):
        fn(i)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps, torch.cuda.max_memory_allocated() / 2 ** 20


def kernel_table(fn, steps):
    import torch
    from nabladft_amd import _lib
    _lib.profile_enable(True)
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    total = sum(v[0] for v in prof.values()) / steps
    dense = sum(v[0] for v in prof.values() if v[2] > 0) / steps
    trip = sum(v[0] for k, v in prof.items() if k in TRIPLET) / steps
    tan = sum(v[0] for k, v in prof.items() if k in TANGENT) / steps
    other_dn = sum(v[0] for k, v in prof.items() if k.startswith("dn_") and k not in TRIPLET) / steps
    ks = sorted(((k, v[0] / steps, v[1] // steps) for k, v in prof.items()), key=lambda x: -x[1])
    return dict(device_ms_nq_kernels=total, dense_products_ms=dense, triplet_kernels_ms=trip, triplet_share=trip / max(total, 1e-9), tangent_triplet_kernels_ms=tan,
                tangent_triplet_share=tan / max(total, 1e-9), other_dimenet_kernels_ms=other_dn,
                dense_TFLOPs=sum(v[2] for v in prof.values()) / steps / max(dense, 1e-9) / 1e9, kernel_ms={k: [round(t, 4), int(n)] for k, t, n in ks[:20]})


def run(molecules=32, steps=10, warmup=2, kernels=True, seed=1, force_loss=False):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    task = build(dev)
    opt = task.configure_optimizers()["optimizer"]
    batches = [synthetic_batch(molecules, seed * 100 + k, dev) for k in range(2)]

    def infer(i):
        with torch.no_grad():
            return task(batches[i % len(batches)])

    def train(i):
        opt.zero_grad(set_to_none=True)
        loss = task.training_step(batches[i % len(batches)], i)
        loss.backward()
        opt.step()
        return loss

    task.eval()
    ms_ef, mem_ef = timed(infer, steps, warmup)
    plan = task.net.last_plan
    out = {"molecules": molecules, "atoms": plan.N, "edges": plan.E, "dtype": "f32", "data": "synthetic", "steps": steps,
           "energy_forces": {"ms": ms_ef, "value": molecules / ms_ef * 1e3, "unit": "conformers/s", "peak_memory_MiB": mem_ef}}
    if kernels:
        out["energy_forces"].update(kernel_table(infer, steps))
    task.train()
    ms_tr, mem_tr = timed(train, steps, warmup)
    out["energy_loss_train_step"] = {"ms": ms_tr, "value": molecules / ms_tr * 1e3, "unit": "conformer-steps/s", "peak_memory_MiB": mem_tr}
    if kernels:
        out["energy_loss_train_step"].update(kernel_table(train, steps))
    if force_loss:
        del task, opt
        torch.cuda.empty_cache()
        task = build(dev, force_loss=True).train()
        opt = task.configure_optimizers()["optimizer"]
        ms_f, mem_f = timed(train, steps, warmup)
        out["force_loss_train_step"] = {"ms": ms_f, "value": molecules / ms_f * 1e3, "unit": "conformer-steps/s", "peak_memory_MiB": mem_f,
                                        "ms_over_energy_loss_step": ms_f / ms_tr}
        if kernels:
            out["force_loss_train_step"].update(kernel_table(train, steps))
    return out


def cpu_baseline(conformers=2, budget=60.0):
    """The restatement (tests/dimenet_ref.py) in float32 on at most 16 threads: E + F, and E + F + loss + backward to the parameters; no optimizer step."""
    import torch
    from nabladft_amd.synth import gen_conformers
    from tests import dimenet_ref as D
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    pos, z, batch, y, f = gen_conformers(101, conformers)
    params = D.make_params(CFG, 0)
    model = D.build(CFG, params, torch.float32)
    res = {}
    for kind in ("energy_forces", "energy_loss_train_step"):
        times, t_start = [], time.perf_counter()
        while True:
            t0 = time.perf_counter()
            E, F, _ = model(z, pos.float(), batch)
            if kind != "energy_forces":
                torch.autograd.grad((E - y.float()).abs().mean(), list(model.parameters()), allow_unused=True)
            times.append(time.perf_counter() - t0)
            if time.perf_counter() - t_start > budget / 2 or len(times) >= 4:
                break
        use = times[1:] if len(times) > 1 else times
        res[kind] = {"value": conformers / sorted(use)[len(use) // 2], "unit": "conformers/s"}
    res.update(cores=cores, kind="restatement", sample=f"{conformers} synthetic conformers ({pos.shape[0]} atoms), yaml sizes, tests/dimenet_ref.py in float32 (index lists "
               f"and a [T, 42] basis, host-side graph construction included), median after one warm-up, torch {torch.__version__} CPU")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 128, 512])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--force-loss", action="store_true", help="add the force-loss training step (coefficients 1, 1)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"workload": "DimeNet++ (config/model/dimenetplusplus.yaml sizes): energy + force call, and energy-loss train step (forward, force backward, L1(E), "
                       "backward, Adam)" + (", and force-loss train step (L1(E) + L1(F), second sweep through the tangent kernels)" if a.force_loss else "") +
                       "; synthetic ~42-atom conformers; HIP events over the timed steps; graph construction inside every step",
           "runs": []}
    import torch
    for m in a.batches:
        try:
            out["runs"].append(run(m, a.steps, a.warmup, a.kernels, force_loss=a.force_loss))
        except torch.OutOfMemoryError as e:                       # the machine is shared: a run that does not fit is recorded, not fatal
            out["runs"].append({"molecules": m, "error": "out of device memory: " + str(e).splitlines()[0]})
            torch.cuda.empty_cache()
    if a.cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
