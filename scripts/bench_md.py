"""Batched MD on one MI355X: what an MD step costs next to the model call it follows (nabladft_amd/md.py, csrc/md.hip), and next to doing the same step on
the host.

PaiNN-OC at the yaml configuration (config/model/painn-oc.yaml: F=128, 6 layers, 100 rbf, 5 A cutoff) with seeded random weights on synthetic drug-like
conformers (nabladft_amd.synth), at 32 and 2048 conformers.  The loop is the job's own: model call (energies + forces) -> one ``nq_md_step`` launch -> model
call ...  The time step is 0.01 fs from 300 K velocities, so that the 60 steps on a random-weight surface (whose forces are far larger than a trained
model's) stay near the start geometry (max_displacement_A in the record; the cost of a step does not depend on the values).  After a warm-up, over ``--steps`` steps (>= 50), for NVE and for Langevin (generator on the device):
  model_ms   HIP events around the model call, mean per call
  step_ms    HIP events around the step launch, mean per step (log ring on, every step sampled)
  loop_ms    HIP events around the whole timed loop (no host synchronisation inside it)
and, in the same process on the same batch, the host-side alternative the reference's per-molecule ase loop amounts to at best: forces device -> host, the
float64 numpy restatement of the step (tests/md_ref.py, vectorised over the batch; Langevin draws its normals with numpy), positions host -> device as
float32.  host_step_ms is the host clock around that synchronised triple, the model call excluded.  Nothing is promised: the record states plainly whether
the kernel is faster than the host leg at each size.

    python scripts/bench_md.py [--steps 50] [--batches 32,2048] [--out profiles/md_step.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, L, R, CUTOFF, KNBR, DT, T0, FRICTION, WARMUP = 128, 6, 100, 5.0, 100, 0.01, 300.0, 0.01, 10


def setup(B, dev, seed=1):
    import torch
    import nabladft_amd as nq
    from nabladft_amd.synth import gen_conformers
    torch.manual_seed(23)
    model = nq.PaiNN(F, L, R, CUTOFF, KNBR, {"name": "gaussian"}, {"name": "polynomial", "exponent": 5}, True, False, False, True, 100).to(dev).eval()
    pos, z, batch, _, _ = gen_conformers(seed, B)
    return model, nq.Batch(pos, z, batch).to(dev)


def device_loop(B, steps, dev, mode):
    import torch
    import nabladft_amd as nq
    from nabladft_amd.md import KB, MDState, masses_for
    from nabladft_amd.optimization import PyGBatchwiseCalculator
    model, batch = setup(B, dev)
    calc = PyGBatchwiseCalculator(model, dev, energy_unit="Hartree", position_unit="Ang")
    st = MDState(batch.ptr.cpu().numpy(), batch.pos, masses_for(batch.z), log_capacity=WARMUP + steps + 1)
    st.init_velocities(T0, seed=5)
    work = nq.Batch(st.pos32, batch.z, batch.batch, ptr=batch.ptr)
    args = (mode, DT, KB * T0 if mode else 0.0, FRICTION if mode else 0.0, 1, 5)
    start = st.r.clone()
    calc.calculate(work)
    for _ in range(WARMUP):
        st.step(calc.forces, calc.energy, *args)
        calc.calculate(work)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for a, b, c in ev:
        a.record()
        st.step(calc.forces, calc.energy, *args)
        b.record()
        calc.calculate(work)
        c.record()
    t1.record()
    torch.cuda.synchronize()
    st.step(calc.forces, calc.energy, *args, finish_only=True)
    h = st.header()
    assert h["step"] == WARMUP + steps and h["log_rows"] == WARMUP + steps + 1 and not h["overflow"] and bool(torch.isfinite(st.r).all())
    step_ms = sum(a.elapsed_time(b) for a, b, _ in ev) / steps
    model_ms = sum(b.elapsed_time(c) for _, b, c in ev) / steps
    loop_ms = t0.elapsed_time(t1) / steps
    return {"batch": B, "atoms": st.N, "mode": "langevin" if mode else "nve", "state_MB": round(st.buf.numel() / 1e6, 2), "model_ms": round(model_ms, 4),
            "step_ms": round(step_ms, 4), "loop_ms_per_step": round(loop_ms, 4), "steps_per_s": round(1e3 / loop_ms, 2),
            "conformer_steps_per_s": round(B * 1e3 / loop_ms, 1), "step_over_model": round(step_ms / model_ms, 5),
            "max_displacement_A": round(float((st.r - start).abs().max()), 4), "timed_steps": steps}


def host_loop(B, steps, dev, mode):
    """The numpy restatement driving the same model: forces device->host, step on the host, positions host->device, every step."""
    import numpy as np
    import torch
    import nabladft_amd as nq
    from md_ref import KB, MDNumpy
    from nabladft_amd.md import MDState, masses_for
    model, batch = setup(B, dev)
    ptr, masses = batch.ptr.cpu().numpy(), masses_for(batch.z)
    st = MDState(ptr, batch.pos, masses)                        # only for the same initial velocities as the device leg
    st.init_velocities(T0, seed=5)
    md = MDNumpy(ptr, masses, batch.pos.double().cpu().numpy(), st.v.cpu().numpy())
    rng = np.random.Generator(np.random.PCG64(5))
    t_step = t_all = 0.0
    pos32 = batch.pos.float().contiguous()

    def one(timed):
        nonlocal t_step, t_all, pos32
        torch.cuda.synchronize()
        a = time.perf_counter()
        with torch.no_grad():
            _, f = model(nq.Batch(pos32, batch.z, batch.batch, ptr=batch.ptr))
        torch.cuda.synchronize()
        b = time.perf_counter()
        fh = f.cpu().numpy()
        xi = eta = None
        if mode:
            xi, eta = rng.standard_normal(fh.shape), rng.standard_normal(fh.shape)
        md.launch(fh, mode, DT, KB * T0, FRICTION, xi, eta)
        pos32 = torch.from_numpy(md.x.astype(np.float32)).to(dev)
        torch.cuda.synchronize()
        c = time.perf_counter()
        if timed:
            t_step += c - b
            t_all += c - a

    for _ in range(WARMUP):
        one(False)
    for _ in range(steps):
        one(True)
    return {"batch": B, "mode": "langevin" if mode else "nve", "host_step_ms": round(1e3 * t_step / steps, 4), "loop_ms_per_step": round(1e3 * t_all / steps, 4),
            "steps_per_s": round(steps / t_all, 2), "timed_steps": steps}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batches", default="32,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_md.py measures on an MI355X; no device is visible (nothing is measured on a CPU)")
    if args.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    runs = [device_loop(b, args.steps, dev, mode) for b in batches for mode in (0, 1)]
    host = [host_loop(b, args.steps, dev, mode) for b in batches for mode in (0, 1)]
    verdict = {f"{d['batch']}_{d['mode']}": {"step_ms": d["step_ms"], "host_step_ms": h["host_step_ms"], "kernel_faster_than_host_leg": d["step_ms"] < h["host_step_ms"],
                                             "host_over_kernel": round(h["host_step_ms"] / d["step_ms"], 1)} for d, h in zip(runs, host)}
    rec = {"bench": "md_step", "model": f"PaiNN-OC F={F} L={L} R={R} cutoff={CUTOFF} (random weights, seed 23), inference call: energies + forces",
           "device": torch.cuda.get_device_name(0), "time_step_fs": DT, "device_resident": runs,
           "host_alternative": {"what": "float64 numpy restatement of the step on the host + D2H forces / H2D float32 positions per step (host clock, model call excluded)",
                                "runs": host},
           "kernel_vs_host_leg": verdict, "note": "both legs ran in this one process on this one device; HIP events for the device leg, host clock for the host leg"}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
