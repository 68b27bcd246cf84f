"""The ``optimize`` job on one MI355X: what an L-BFGS step costs next to the model call it follows (nabladft_amd/optimization.py, csrc/lbfgs.hip).

PaiNN-OC at the yaml configuration (config/model/painn-oc.yaml: F=128, 6 layers, 100 rbf, 5 A cutoff) with seeded random weights on synthetic drug-like
conformers (nabladft_amd.synth), at 32 and 2048 conformers, history depth 100 as in config/optimizer/batchwise_lbfgs.yaml.  The loop is the job's own:
model call (energies + forces) -> one ``nq_lbfgs_step`` launch -> model call ...  fmax is set below anything the forces reach, so every molecule does the
full two-loop recursion in every step, and maxstep is 0.02 A so that 150+ steps on a random-weight surface stay near the start geometry (the cost of a step
does not depend on the values).  After the history has filled, over ``--steps`` steps (>= 50):
  model_ms      HIP events around the model call, mean per call
  optimizer_ms  HIP events around the step launch, mean per step
  steps_per_s   from HIP events around the whole timed loop (no host synchronisation inside it), conformer_steps_per_s = batch x that
For context, at 32 conformers: the host-side alternative, the float64 numpy restatement of the reference's step (tests/lbfgs_helpers.py) driving the same
model with a device->host copy of the forces and a host->device copy of the positions every step (host clock around synchronised work).
Acceptance is relative: optimizer_ms < model_ms at both batch sizes, measured in the same run; the script exits non-zero otherwise.

    python scripts/bench_optimize.py [--steps 50] [--batches 32,2048] [--out profiles/optimize_lbfgs.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, L, R, CUTOFF, KNBR, MEMORY, FMAX, MAXSTEP = 128, 6, 100, 5.0, 100, 100, 1e-9, 0.02


def setup(B, dev, seed=1):
    import torch
    import nabladft_amd as nq
    from nabladft_amd.synth import gen_conformers
    torch.manual_seed(23)
    model = nq.PaiNN(F, L, R, CUTOFF, KNBR, {"name": "gaussian"}, {"name": "polynomial", "exponent": 5}, True, False, False, True, 100).to(dev).eval()
    pos, z, batch, _, _ = gen_conformers(seed, B)
    return model, nq.Batch(pos, z, batch).to(dev)


def device_loop(B, steps, dev):
    import torch
    import nabladft_amd as nq
    from nabladft_amd.optimization import LBFGSState, PyGBatchwiseCalculator
    model, batch = setup(B, dev)
    calc = PyGBatchwiseCalculator(model, dev, energy_unit="Hartree", position_unit="Ang")
    st = LBFGSState(batch.ptr.cpu().numpy(), batch.pos, MEMORY)
    work = nq.Batch(st.pos32, batch.z, batch.batch, ptr=batch.ptr)
    calc.calculate(work)
    e_start = calc.energy.double().cpu()
    for _ in range(MEMORY + 5):                                  # fills the ring; warms up every shape the timed loop uses
        st.step(calc.forces, FMAX, MAXSTEP, 1.0, 1.0)
        calc.calculate(work)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for a, b, c in ev:
        a.record()
        calc.calculate(work)
        b.record()
        st.step(calc.forces, FMAX, MAXSTEP, 1.0, 1.0)
        c.record()
    t1.record()
    torch.cuda.synchronize()
    model_ms = sum(a.elapsed_time(b) for a, b, _ in ev) / steps
    opt_ms = sum(b.elapsed_time(c) for _, b, c in ev) / steps
    loop_ms = t0.elapsed_time(t1) / steps
    calc.calculate(work)
    h = st.header()
    assert h["iteration"] == MEMORY + 5 + steps and h["unconverged"] == B and bool(torch.isfinite(st.r).all())
    return {"batch": B, "atoms": st.N, "history_depth": MEMORY, "state_MB": round(st.buf.numel() / 1e6, 1), "model_ms": round(model_ms, 4),
            "optimizer_ms": round(opt_ms, 4), "loop_ms_per_step": round(loop_ms, 4), "steps_per_s": round(1e3 / loop_ms, 2),
            "conformer_steps_per_s": round(B * 1e3 / loop_ms, 1), "optimizer_over_model": round(opt_ms / model_ms, 4),
            "energy_drop_mean": round(float((e_start - calc.energy.double().cpu()).mean()), 4), "timed_steps": steps}


def host_loop(B, steps, dev):
    """The numpy restatement of the reference's step driving the same model: forces device->host, positions host->device, every step."""
    import torch
    import nabladft_amd as nq
    from lbfgs_helpers import LbfgsNumpy
    model, batch = setup(B, dev)
    opt = LbfgsNumpy(batch.ptr.cpu().numpy(), memory=MEMORY, maxstep=MAXSTEP)
    r = batch.pos.double().cpu().numpy()
    t_opt = t_all = 0.0

    def one(timed):
        nonlocal r, t_opt, t_all
        torch.cuda.synchronize()
        a = time.perf_counter()
        with torch.no_grad():
            _, f = model(nq.Batch(torch.from_numpy(r).float().to(dev), batch.z, batch.batch, ptr=batch.ptr))
        f = f.cpu().numpy()
        b = time.perf_counter()
        r = opt.step(r, f, FMAX)
        c = time.perf_counter()
        if timed:
            t_opt += c - b
            t_all += c - a

    for _ in range(MEMORY + 5):
        one(False)
    for _ in range(steps):
        one(True)
    return {"batch": B, "what": "float64 numpy restatement of the reference step on the host + D2H forces / H2D positions per step (host clock)",
            "host_optimizer_ms": round(1e3 * t_opt / steps, 4), "loop_ms_per_step": round(1e3 * t_all / steps, 4), "steps_per_s": round(steps / t_all, 2),
            "conformer_steps_per_s": round(B * steps / t_all, 1), "timed_steps": steps}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batches", default="32,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimize_lbfgs.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimize.py measures on an MI355X; no device is visible (nothing is measured on a CPU)")
    if args.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    runs = [device_loop(int(b), args.steps, dev) for b in args.batches.split(",")]
    rec = {"bench": "optimize_lbfgs", "model": f"PaiNN-OC F={F} L={L} R={R} cutoff={CUTOFF} (random weights, seed 23), inference call: energies + forces",
           "device": torch.cuda.get_device_name(0), "device_resident": runs, "host_alternative": host_loop(32, args.steps, dev),
           "criterion": "optimizer_ms < model_ms at every batch size", "criterion_met": all(r["optimizer_ms"] < r["model_ms"] for r in runs)}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sys.exit(0 if rec["criterion_met"] else 1)
