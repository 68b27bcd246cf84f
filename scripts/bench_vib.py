"""Batched normal modes on one MI355X: where the time of ``BatchedVibrations.run`` goes (nabladft_amd/vibrations.py, csrc/vib.hip), and the same job with
the host in the loop.

PaiNN-OC at the yaml configuration (config/model/painn-oc.yaml: F=128, 6 layers, 100 rbf, 5 A cutoff) with seeded random weights on synthetic drug-like
conformers (nabladft_amd.synth), at 32 and 2048 molecules (about 42 atoms each: 6 n images per molecule).  After one untimed warm-up chunk, HIP events give
  model_ms       all model calls on the images
  fd_ms          all displace + accumulate launches (and the device-side building of the image batches' z / batch / ptr)
  eig_ms         finish + the Jacobi eigensolver
  total_ms       the whole run (no host synchronisation inside it)
and, in the same process on the same batch, the host-in-the-loop alternative: per call the float32 images are built with numpy and copied to the device, the
forces are copied back, the rows are assembled with numpy (tests/vib_ref.py arithmetic, vectorised), then ``np.linalg.eigh`` per molecule; host clock,
``host_model_ms`` being the synchronised model calls inside it.  ``torch.linalg.eigh`` on the device runs on the same mass-weighted matrices when this torch
build has it.  ``--images`` lists the values of ``images_per_call`` to compare (the class default is chosen from this record).  The time at the cap: the
eigensolver alone on one random symmetric matrix of 576 (global-memory path), and on 256 of them (one per compute unit).  Nothing is promised: the record
states plainly where the Jacobi kernel loses to torch's eigh.

    python scripts/bench_vib.py [--batches 32,2048] [--images 512,1024,2048,4096] [--out profiles/vib_step.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, L, R, CUTOFF, KNBR = 128, 6, 100, 5.0, 100


def setup(B, dev, seed=1):
    import torch
    import nabladft_amd as nq
    from nabladft_amd.synth import gen_conformers
    torch.manual_seed(23)
    model = nq.PaiNN(F, L, R, CUTOFF, KNBR, {"name": "gaussian"}, {"name": "polynomial", "exponent": 5}, True, False, False, True, 100).to(dev).eval()
    pos, z, batch, _, _ = gen_conformers(seed, B)
    return model, nq.Batch(pos, z, batch).to(dev)


def device_run(B, images_per_call, dev):
    import torch
    from nabladft_amd import _lib
    from nabladft_amd.optimization import PyGBatchwiseCalculator
    from nabladft_amd.vibrations import BatchedVibrations
    model, batch = setup(B, dev)
    calc = PyGBatchwiseCalculator(model, dev, energy_unit="Hartree", position_unit="Ang")
    vib = BatchedVibrations(calc, images_per_call=images_per_call)
    st = vib.prepare(batch)
    c0, c1 = vib.todo[0]                                    # warm-up: one chunk, untimed
    im = vib.image_batch(c0, c1)
    st.displace(c0, c1, vib.delta, im.pos)
    calc.calculate(im)
    torch.cuda.synchronize()
    E = lambda: torch.cuda.Event(enable_timing=True)
    ev = [[E() for _ in range(4)] for _ in vib.todo]
    t0, t1, t2 = E(), E(), E()
    t0.record()
    for (c0, c1), (a, b, c, d) in zip(vib.todo, ev):
        a.record()
        im = vib.image_batch(c0, c1)
        st.displace(c0, c1, vib.delta, im.pos)
        b.record()
        calc.calculate(im)
        c.record()
        st.accumulate(c0, c1, calc.forces)
        d.record()
    t1.record()
    _lib.profile_read()
    _lib.profile_enable(True)                              # per-kernel events of the library's own launchers: finish, Jacobi in LDS, Jacobi in global memory
    st.finish()
    st.eigh(True)
    _lib.profile_enable(False)
    t2.record()
    torch.cuda.synchronize()
    kernels = {k: round(v[0], 2) for k, v in _lib.profile_read().items() if k.startswith("vib_")}
    assert st.header()["status"] == 0 and not st.status.any()
    model_ms = sum(b.elapsed_time(c) for _, b, c, _ in ev)
    fd_ms = sum(a.elapsed_time(b) + c.elapsed_time(d) for a, b, c, d in ev)
    rec = {"batch": B, "atoms": st.N, "displacements": st.D, "images": 2 * st.D, "images_per_call": images_per_call, "model_calls": len(vib.todo),
           "state_MB": round(st.buf.numel() / 1e6, 1), "model_ms": round(model_ms, 2), "fd_ms": round(fd_ms, 2), "eig_ms": round(t1.elapsed_time(t2), 2),
           "total_ms": round(t0.elapsed_time(t2), 2), "sweeps_max": int(st.sweeps.max()), "largest_m": st.max_m, "molecules_in_lds": st.n_lds,
           "eig_kernels_ms": kernels, "molecules_in_global_memory": st.B - st.n_lds, "asymmetry_max": float(st.asymmetry.max())}
    rec["shares"] = {k: round(rec[k + "_ms"] / rec["total_ms"], 4) for k in ("model", "fd", "eig")}
    rec["images_per_s"] = round(2 * st.D / rec["total_ms"] * 1e3, 1)
    rec["peak_memory_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 1)
    calc.model = None                                       # the engine's workspace goes with the model
    return rec, vib


def release():
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def host_run(B, images_per_call, dev):
    """The host in the loop: numpy images -> device, model, forces -> host, numpy rows; then numpy eigh per molecule."""
    import numpy as np
    import torch
    import nabladft_amd as nq
    from nabladft_amd.md import masses_for
    from nabladft_amd.vibrations import chunks, plan
    model, batch = setup(B, dev)
    ptr = batch.ptr.cpu().numpy()
    pl = plan(ptr)
    x0 = batch.pos.double().cpu().numpy()
    x32 = x0.astype(np.float32)
    z = batch.z.cpu().numpy()
    im_all = np.repeat(1.0 / np.sqrt(masses_for(z)), 3)
    n, start = pl["n"], ptr[:-1]
    G = np.zeros(pl["P"])
    t_model = 0.0
    todo = chunks(pl, images_per_call)
    t_begin = 0.0
    for it, (c0, c1) in enumerate(todo[:1] + todo):         # the first chunk once more in front, untimed: the engine allocates its workspace in its first call
        if it == 1:
            torch.cuda.synchronize()
            t_model, t_begin = 0.0, time.perf_counter()
        mol = np.repeat(pl["disp_mol"][c0:c1], 2)
        sizes = n[mol]
        iptr = np.concatenate([[0], np.cumsum(sizes)])
        ibatch = np.repeat(np.arange(len(mol)), sizes)
        orig = start[mol][ibatch] + np.arange(iptr[-1]) - iptr[ibatch]
        img = x32[orig]
        j = np.arange(c0, c1)
        atom, axis = pl["free_atom"][j // 3], j % 3
        row_m, row_p = iptr[:-1][0::2] + atom - start[pl["disp_mol"][j]], iptr[:-1][1::2] + atom - start[pl["disp_mol"][j]]
        img[row_m, axis] = (x0[atom, axis] - 0.01).astype(np.float32)
        img[row_p, axis] = (x0[atom, axis] + 0.01).astype(np.float32)
        h = img[row_p, axis].astype(np.float64) - img[row_m, axis].astype(np.float64)
        a = time.perf_counter()
        with torch.no_grad():
            _, f = model(nq.Batch(torch.from_numpy(img).to(dev), torch.from_numpy(z[orig]).to(dev), torch.from_numpy(ibatch).to(dev), ptr=torch.from_numpy(iptr).to(dev)))
        torch.cuda.synchronize()
        t_model += time.perf_counter() - a
        f = f.cpu().numpy().astype(np.float64)
        for i, jj in enumerate(j):                       # every molecule's atoms are free here: a row is the molecule's whole force difference
            b = pl["disp_mol"][jj]
            m = pl["m"][b]
            fm, fp = f[iptr[2 * i]:iptr[2 * i + 1]].ravel(), f[iptr[2 * i + 1]:iptr[2 * i + 2]].ravel()
            o = pl["hess_ptr"][b] + (jj - pl["dof_ptr"][b]) * m
            G[o:o + m] = (fm - fp) / h[i]
    t_fd = time.perf_counter()
    w = np.zeros(pl["D"])
    for b in range(pl["B"]):
        m = pl["m"][b]
        g = G[pl["hess_ptr"][b]:pl["hess_ptr"][b + 1]].reshape(m, m)
        im = im_all[pl["dof_ptr"][b]:pl["dof_ptr"][b + 1]]
        w[pl["dof_ptr"][b]:pl["dof_ptr"][b + 1]] = np.linalg.eigh(im[:, None] * (0.5 * (g + g.T)) * im)[0]
    t_end = time.perf_counter()
    return {"batch": B, "images_per_call": images_per_call, "host_total_ms": round(1e3 * (t_end - t_begin), 2), "host_model_ms": round(1e3 * t_model, 2),
            "host_fd_ms": round(1e3 * (t_fd - t_begin - t_model), 2), "host_eig_ms": round(1e3 * (t_end - t_fd), 2)}, w


def torch_eigh(vib, dev):
    """torch.linalg.eigh on the device for the same mass-weighted matrices (equal sizes are batched), or the reason it did not run."""
    import torch
    st = vib.state
    try:
        im, H = st.im, st.hessian
        groups = {}
        for b, m in enumerate(st.plan["m"]):
            groups.setdefault(int(m), []).append(b)
        mats = []
        for m, bs in groups.items():
            idx = torch.tensor([st.plan["hess_ptr"][b] for b in bs], device=dev)[:, None] + torch.arange(m * m, device=dev)[None]
            d = torch.tensor([st.plan["dof_ptr"][b] for b in bs], device=dev)[:, None] + torch.arange(m, device=dev)[None]
            mats.append(im[d][:, :, None] * H[idx].reshape(len(bs), m, m) * im[d][:, None, :])
        torch.linalg.eigh(mats[0][:1])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for A in mats:
            torch.linalg.eigh(A)
        b.record()
        torch.cuda.synchronize()
        return {"torch_eigh_ms": round(a.elapsed_time(b), 2), "distinct_sizes": len(mats)}
    except Exception as e:                                    # this torch build may not link a device eigensolver
        return {"torch_eigh_ms": None, "reason": f"{type(e).__name__}: {str(e)[:200]}"}


def at_the_cap(dev, copies):
    import numpy as np
    import torch
    from nabladft_amd.vibrations import MAX_DOF, VibState
    n = MAX_DOF // 3
    ptr = np.arange(copies + 1) * n
    st = VibState(ptr, torch.zeros(copies * n, 3, dtype=torch.float64, device=dev), np.ones(copies * n))
    M = torch.randn(copies, MAX_DOF, MAX_DOF, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(5))
    A = (M + M.transpose(1, 2)).contiguous()
    st.work.copy_(A.reshape(-1))
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st.eigh(False)
    b.record()
    torch.cuda.synchronize()
    rec = {"m": MAX_DOF, "matrices": copies, "jacobi_ms": round(a.elapsed_time(b), 1), "sweeps": int(st.sweeps.max()), "status": int(st.status.max())}
    try:
        torch.linalg.eigh(A[:1])
        torch.cuda.synchronize()
        a.record()
        torch.linalg.eigh(A)
        b.record()
        torch.cuda.synchronize()
        rec["torch_eigh_ms"] = round(a.elapsed_time(b), 1)
    except Exception as e:
        rec["torch_eigh_ms"], rec["reason"] = None, f"{type(e).__name__}: {str(e)[:200]}"
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,2048")
    ap.add_argument("--images", default="512,1024,2048,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vib_step.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vib.py measures on an MI355X; no device is visible (nothing is measured on a CPU)")
    dev = torch.device("cuda:0")
    from nabladft_amd.vibrations import BatchedVibrations
    import inspect
    default_ipc = inspect.signature(BatchedVibrations.__init__).parameters["images_per_call"].default
    runs, hosts, eighs, sweep = [], [], [], []
    for B in [int(b) for b in args.batches.split(",")]:
        for ipc in [int(i) for i in args.images.split(",")]:
            if ipc != default_ipc:
                release()
                try:
                    sweep.append(device_run(B, ipc, dev)[0])
                except torch.OutOfMemoryError as e:          # the engine's workspace grows with the images of a call
                    sweep.append({"batch": B, "images_per_call": ipc, "out_of_memory": str(e)[:120]})
                print(json.dumps(sweep[-1]), flush=True)
        release()
        rec, vib = device_run(B, default_ipc, dev)
        print(json.dumps(rec), flush=True)
        release()
        host, w_host = host_run(B, default_ipc, dev)
        print(json.dumps(host), flush=True)
        w_dev = vib.omega2.cpu().numpy()
        host["omega2_max_deviation_from_device"] = float(np.abs(w_dev - w_host).max())
        host["omega2_largest"] = float(np.abs(w_host).max())
        te = torch_eigh(vib, dev)
        te["batch"], te["jacobi_finish_ms"] = B, rec["eig_ms"]
        te["jacobi_faster"] = None if te["torch_eigh_ms"] is None else bool(rec["eig_ms"] < te["torch_eigh_ms"])
        print(json.dumps(te), flush=True)
        runs.append(rec), hosts.append(host), eighs.append(te)
    del vib
    release()
    cap = [at_the_cap(dev, 1), at_the_cap(dev, 256)]
    print(json.dumps(cap), flush=True)
    out = {"bench": "vib_step", "model": f"PaiNN-OC F={F} L={L} R={R} cutoff={CUTOFF} (random weights, seed 23), inference call: energies + forces",
           "device": torch.cuda.get_device_name(0), "delta_A": 0.01, "default_images_per_call": default_ipc, "device_resident": runs,
           "images_per_call_sweep": sweep, "host_in_the_loop": hosts, "eigensolver_vs_torch": eighs, "at_the_cap": cap,
           "note": "all legs ran in this one process on this one device; HIP events for the device legs, host clock for the host leg"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
