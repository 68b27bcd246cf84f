"""Batched orbital energies (nabladft_amd/orbitals.py) against the alternatives, one process, HIP events, warm-up first:

  (a) the device solver: one launch of nq_orb_solve for the whole batch;
  (b) the host route: D2H of the packed matrices, per molecule np.linalg.cholesky + two triangular solves + np.linalg.eigh + back substitution, H2D;
  (c) torch.linalg on the device: cholesky / solve_triangular / eigh / solve_triangular, the molecules grouped by size into batched calls;
  (d) at 32 molecules only: the Jacobi kernel of csrc/vib.hip on the reduced matrices L^-1 H L^-T (computed on the host, padded with a decoupled diagonal
      to a multiple of three, which is what a VibState can carry), m <= 576 -- the only eigensolver this project had.
  Also: one matrix at the cap m = 1024, and the QHNet forward (config/qhnet.yaml sizes) on 16 conformers, the model call such a solve follows.

Conformers: nabladft_amd/synth.py sizes with the QHNet yaml's orbital table (H 5, C/N/O/F 14, S/Cl 18 orbitals: a 42-atom conformer has about 412);
matrices: tests/orbitals_ref.case at those sizes (conditioned overlap, Fock-like H) -- the solver's cost depends on the size, not on the chemistry.
No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 900 python scripts/bench_orbitals.py --molecules 32 --out profiles/orbitals_step.json && \\
    timeout -k 10 900 python scripts/bench_orbitals.py --molecules 512 --skip-cap --skip-model --append --out profiles/orbitals_step.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scripts.bench_qhnet import ORBITALS  # noqa: E402


def sizes_of(molecules, seed=7):
    import torch
    from nabladft_amd.synth import gen_conformers
    _, z, batch, _, _ = gen_conformers(seed, molecules)
    per_atom = torch.tensor([sum(2 * l + 1 for l in ORBITALS[int(a)]) for a in z.tolist()])
    return torch.zeros(molecules, dtype=torch.long).index_add_(0, batch, per_atom).tolist()


def problems(ms, seed=100):
    import orbitals_ref as R
    cache, out = {}, []
    for b, m in enumerate(ms):                       # one generated problem per distinct size, shifted per molecule: the QR of case() is the slow part
        if m not in cache:
            cache[m] = R.case(m, 1e2, seed + m)
        H, S = cache[m]
        out.append((H + 0.01 * (b % 17) * S, S))     # H + c S shifts every eigenvalue by c: another problem of the same cost
    return out


def event_ms(fn, warmup, repeat):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [float(t) for t in times]


def leg_device(probs, warmup, repeat):
    import torch
    from nabladft_amd.orbitals import BatchedOrbitals
    op = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in probs])])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    orb = BatchedOrbitals(op, "cuda")
    ms, all_ms = event_ms(lambda: orb.solve(H, S), warmup, repeat)
    orb.check()
    return dict(ms=ms, runs=all_ms, ql_sweeps=int(orb.iters.sum()), launches=1), H, S, op


def leg_host(H_dev, S_dev, op, repeat):
    import torch
    pp = np.concatenate([[0], np.cumsum(np.diff(op) ** 2)])
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        H, S = H_dev.cpu().numpy(), S_dev.cpu().numpy()
        eps, coeff = [], []
        for b in range(len(op) - 1):
            m = int(op[b + 1] - op[b])
            Hb, Sb = H[pp[b]:pp[b + 1]].reshape(m, m), S[pp[b]:pp[b + 1]].reshape(m, m)
            L = np.linalg.cholesky(Sb)
            X = np.linalg.solve(L, Hb)               # numpy has no triangular solver: the general one, on a triangular matrix
            A = np.linalg.solve(L, X.T).T
            w, Y = np.linalg.eigh(0.5 * (A + A.T))
            eps.append(w), coeff.append(np.linalg.solve(L.T, Y).T.ravel())
        out = (torch.from_numpy(np.concatenate(eps)).cuda(), torch.from_numpy(np.concatenate(coeff)).cuda())
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    del out
    return dict(ms=float(np.median(times)), runs=times, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count())


def leg_torch(H_dev, S_dev, op, warmup, repeat):
    import torch
    pp = np.concatenate([[0], np.cumsum(np.diff(op) ** 2)])
    groups = {}
    for b in range(len(op) - 1):
        groups.setdefault(int(op[b + 1] - op[b]), []).append(b)
    stacks = [(torch.stack([H_dev[pp[b]:pp[b + 1]].view(m, m) for b in bs]), torch.stack([S_dev[pp[b]:pp[b + 1]].view(m, m) for b in bs])) for m, bs in groups.items()]

    def run():
        for Hs, Ss in stacks:
            L = torch.linalg.cholesky(Ss)
            X = torch.linalg.solve_triangular(L, Hs, upper=False)
            A = torch.linalg.solve_triangular(L, X.transpose(1, 2), upper=False).transpose(1, 2)
            w, Y = torch.linalg.eigh(0.5 * (A + A.transpose(1, 2)))
            torch.linalg.solve_triangular(L.transpose(1, 2), Y, upper=True)
    ms, all_ms = event_ms(run, warmup, repeat)
    return dict(ms=ms, runs=all_ms, groups=len(stacks))


def leg_jacobi(probs, repeat):
    import torch
    import orbitals_ref as R
    from nabladft_amd.vibrations import MAX_DOF, VibState
    mats = []
    for H, S in probs:
        m = H.shape[0]
        if m > MAX_DOF - 2:
            continue
        L = np.linalg.cholesky(S)
        A = R.lower_solve(L, R.lower_solve(L, H).T).T
        A = 0.5 * (A + A.T)
        mp = 3 * ((m + 2) // 3)
        P = np.diag(np.full(mp, 1e3))
        P[:m, :m] = A
        mats.append(P)
    if not mats:
        return dict(ms=None, molecules=0)
    ptr = np.concatenate([[0], np.cumsum([a.shape[0] // 3 for a in mats])])
    st = VibState(ptr, torch.zeros(int(ptr[-1]), 3, dtype=torch.float64, device="cuda"), np.ones(int(ptr[-1])))
    flat = torch.from_numpy(np.concatenate([a.ravel() for a in mats])).cuda()

    def run():
        st.work.copy_(flat)
        st.eigh(scale_modes=False)
    ms, all_ms = event_ms(run, 0, repeat)
    return dict(ms=ms, runs=all_ms, molecules=len(mats), sweeps=int(st.sweeps.max()), status=int(st.status.max()))


def leg_model(molecules, warmup, repeat):
    import torch
    from scripts.bench_qhnet import build, synthetic_batch
    net = build("cuda")
    b = synthetic_batch(molecules, 7, "cuda")

    def run():
        with torch.no_grad():
            net(b, packed=True)
    ms, all_ms = event_ms(run, warmup, repeat)
    return dict(ms=ms, runs=all_ms, molecules=molecules)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-cap", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbitals_step.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_orbitals.py needs the MI355X"
    ms = sizes_of(args.molecules)
    probs = problems(ms)
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), device=torch.cuda.get_device_name(0))
    rec["device_solve"], H, S, op = leg_device(probs, args.warmup, args.repeat)
    print(json.dumps(dict(leg="a", **rec["device_solve"])), flush=True)
    rec["host_numpy"] = leg_host(H, S, op, 1 if args.molecules > 64 else args.repeat)
    print(json.dumps(dict(leg="b", **rec["host_numpy"])), flush=True)
    if not args.skip_torch:
        rec["torch_linalg"] = leg_torch(H, S, op, args.warmup, args.repeat)
        print(json.dumps(dict(leg="c", **rec["torch_linalg"])), flush=True)
    if args.molecules <= 32:
        rec["vib_jacobi"] = leg_jacobi(probs, 1)
        print(json.dumps(dict(leg="d", **rec["vib_jacobi"])), flush=True)
    if not args.skip_cap:
        rec["cap_m1024"] = leg_device(problems([1024]), args.warmup, args.repeat)[0]
        print(json.dumps(dict(leg="cap", **rec["cap_m1024"])), flush=True)
    if not args.skip_model:
        rec["qhnet_forward"] = leg_model(16, args.warmup, args.repeat)
        print(json.dumps(dict(leg="model", **rec["qhnet_forward"])), flush=True)
    records = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as fh:
            records = json.load(fh)
    records.append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(records, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
