"""The eigensolver-free square roots (``BatchedMatrixRoot``, csrc/orbsqrt.hip) and the SCF target without a solve (``scf_target_iterative``) leg by leg,
against the decomposition route and ``torch.linalg.eigh`` IN THE SAME RUN, one process, HIP events, warm-up first, on the synthetic conformers of
scripts/bench_orbital_loss.py with the overlaps of scripts/bench_orbital_purify.py:

  (a) init: c, Y_0 = S / c, Z_0 = I (one workgroup per molecule);
  (b) one iteration, split per launch: iteration 0 on S (both launches do their products) and iteration 0 on S = I (delta_0 = 0: the first launch forms Z Y in
      full, the second decides to stop and forms nothing); launch 1 is the second figure, launch 2 the difference;
  (c) the loop: nq_orb_sqrt_init + nq_orb_sqrt_run with max_iter = 100 (two launches per iteration, finished molecules exit at once), the init of (a)
      subtracted, with the iteration counts and the useful Tflop/s counting 5 m^3 per iteration and molecule;
  (d) finish: the two scaled, mirrored outputs;
  (e) the decomposition route on the same batch: ``LowdinBasis.of(S, method="eigh")`` (one latency-bound solve, weights, one wgram launch);
  (f) S^(1/2) and S^(-1/2) through ``torch.linalg.eigh`` on dense blocks grouped by size, the regrouping by prebuilt index gather / scatter;
  (g) ``scf_target`` and ``scf_target_iterative``.

  With --model: the QHNet training step (config/qhnet.yaml sizes, 16 conformers) with the residual term and an UNCACHED target, by both methods, set up as in
  scripts/bench_orbital_commutator.py.

No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_sqrt.py --molecules 32 --model --out profiles/orbital_sqrt_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_sqrt.py --molecules 512 --append --out profiles/orbital_sqrt_step.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scripts.bench_orbital_loss import closed_shell_counts, conformers  # noqa: E402
from scripts.bench_orbital_purify import gapped_problems  # noqa: E402
from scripts.bench_orbitals import event_ms  # noqa: E402


def leg_eigh(st, S, warmup, repeat):
    """S^(1/2) and S^(-1/2) through ``torch.linalg.eigh`` per size group -> (record, half [P], inv_half [P])."""
    import torch
    dev = S.device
    groups = {}
    for b, m in enumerate(st.m.tolist()):
        groups.setdefault(int(m), []).append(b)
    pp = st.pack_ptr_host
    index = [(m, len(bs), torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev)) for m, bs in groups.items()]

    def step():
        half, inv = torch.empty_like(S), torch.empty_like(S)
        for m, nb, blk in index:
            s, U = torch.linalg.eigh(S[blk].view(nb, m, m))
            a = s.sqrt()
            half[blk] = torch.bmm(U * a[:, None, :], U.mT).reshape(nb, m * m)
            inv[blk] = torch.bmm(U / a[:, None, :], U.mT).reshape(nb, m * m)
        return half, inv
    t, runs = event_ms(step, warmup, repeat)
    return (dict(ms=t, runs=runs, groups=len(groups), what="torch.linalg.eigh per size group, two bmm", regrouping="index gather / scatter, indices prebuilt"),) + step()


def leg_model(warmup, repeat, molecules=16):
    """The QHNet training step with the residual term against an UNCACHED target, by both methods; the set-up of scripts/bench_orbital_commutator.py."""
    import torch
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from scripts.bench_qhnet import build, synthetic_batch
    net = build("cuda")
    b = synthetic_batch(molecules, 7, "cuda")
    with torch.no_grad():
        pred = net(b, packed=True)
    op = net.last_plan.mol_orb_ptr.cpu().numpy()
    ms = np.diff(op).tolist()
    target = (pred + 0.05 * torch.randn(pred.shape, generator=torch.Generator().manual_seed(1)).cuda()).detach()
    ne = torch.zeros(molecules, dtype=torch.long).index_add_(0, b.batch.cpu(), b.z.cpu().long()).tolist()
    n_occ = closed_shell_counts(ms, ne)
    probs = gapped_problems(ms, n_occ)
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    H_gap = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    c = 0.05 / (float(pred.abs().max()) * max(ms))
    H_t = (H_gap + c * target.double()).detach()
    opt = torch.optim.AdamW(net.parameters(), lr=5e-4, betas=(0.9, 0.95), amsgrad=True)
    l_h, l_r = HamiltonianLoss(), nq.ScfResidualLoss("mse")
    cached = nq.scf_target(H_t, S, op, n_occ)

    def step(route):
        opt.zero_grad(set_to_none=True)
        p = net(b, packed=True)
        loss = l_h(p, target)
        if route != "plain":
            tgt = cached if route == "residual_cached" else (nq.scf_target_iterative if route == "iterative" else nq.scf_target)(H_t, S, op, n_occ)
            loss = loss + 0.1 * l_r(nq.scf_residual_to_target(H_gap + c * p.double(), tgt), None, op)
        loss.backward()
        opt.step()
    out = dict(molecules=molecules, m_mean=float(np.mean(ms)))
    for route in ("plain", "residual_cached", "solve", "iterative"):
        t, runs = event_ms(lambda: step(route), warmup, repeat)
        key = route if route in ("plain", "residual_cached") else f"residual_uncached_{route}"
        out[f"step_{key}_ms"], out[f"step_{key}_runs"] = t, runs
    out["uncached_iterative_over_solve"] = out["step_residual_uncached_iterative_ms"] / out["step_residual_uncached_solve_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--model", action="store_true", help="also time the QHNet training step at 16 conformers with an uncached target by both methods")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_sqrt_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import BatchedMatrixRoot
    assert torch.cuda.is_available(), "bench_orbital_sqrt.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    n_occ = closed_shell_counts(ms, ne)
    probs = gapped_problems(ms, n_occ)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    eye = torch.from_numpy(np.concatenate([np.eye(m).ravel() for m in ms])).cuda()
    kappa = [float(np.linalg.cond(p[1])) for p in probs[:8]]
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), device=torch.cuda.get_device_name(0),
               kappa_of_the_first_8=[min(kappa), max(kappa)])
    w, r = args.warmup, args.repeat
    cube = np.asarray(ms, dtype=np.float64) ** 3

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)
        return t

    root = BatchedMatrixRoot(op, "cuda")
    t_init = leg("init", lambda: root.prepare(S, 100), launches=1)
    root.prepare(S, 100)
    t_both = leg("iteration_both_launches", lambda: root.step(0), launches=2, useful_flops=5.0 * float(cube.sum()))
    root.prepare(eye, 100)
    t_first = leg("iteration_launch_1_T", lambda: root.step(0), launches=2, what="S = I: the second launch decides to stop and forms nothing",
                  useful_flops=float(cube.sum()))
    rec["iteration_launch_2_update"] = dict(ms=t_both - t_first, what="the difference of the two legs above: Y' = Y T and Z' = T Z", useful_flops=4.0 * float(cube.sum()))
    for name in ("iteration_both_launches", "iteration_launch_1_T", "iteration_launch_2_update"):
        rec[name]["useful_tflops"] = rec[name]["useful_flops"] / (max(rec[name]["ms"], 1e-9) * 1e-3) / 1e12

    def init_and_loop():
        root.prepare(S, 100)
        root.state.call("nq_orb_sqrt_run", 100, *root._iterates(), _lib.ptr(root.ctl), _lib.ptr(root.log))
    t_loop = leg("init_and_loop", init_and_loop, launches=201) - t_init
    leg("finish", lambda: root.finish(), launches=1)
    root.check()
    iters = root.iterations.cpu().numpy()
    rec["loop"] = dict(ms=t_loop, iterations_min=int(iters.min()), iterations_max=int(iters.max()), iterations_mean=float(iters.mean()),
                       useful_tflops=5.0 * float((cube * iters).sum()) / (t_loop * 1e-3) / 1e12, what="init_and_loop minus init; 5 m^3 per iteration and molecule")
    t_ns = leg("roots_newton_schulz", lambda: root.run(S, 100), what="init, loop and finish: BatchedMatrixRoot.run")
    t_eig = leg("roots_decomposition", lambda: nq.LowdinBasis.of(S, op), what="LowdinBasis.of(method='eigh'): one solve of S, weights, one wgram launch")
    rec["roots_newton_schulz_over_decomposition"] = t_ns / t_eig
    ref = nq.LowdinBasis.of(S, op).check()
    rec["against_decomposition"] = dict(half=float((root.half - ref.half).abs().max()), inv_half=float((root.inv_half - ref.inv_half).abs().max()),
                                        max_abs_inv_half=float(ref.inv_half.abs().max()))
    rec["torch_eigh"], th, ti = leg_eigh(root.state, S, w, r)
    rec["torch_eigh"]["max_difference_inv_half"] = float((root.inv_half - ti).abs().max())
    print(json.dumps(dict(leg="torch_eigh", **rec["torch_eigh"])), flush=True)
    rec["roots_newton_schulz_over_torch_eigh"] = t_ns / rec["torch_eigh"]["ms"]
    t_sv = leg("scf_target_solve", lambda: nq.scf_target(H, S, op, n_occ), what="one target solve, one decomposition of S, the target's congruence")
    t_it = leg("scf_target_iterative", lambda: nq.scf_target_iterative(H, S, op, n_occ), what="Newton-Schulz roots, one congruence, SP2 on the standard problem")
    rec["scf_target_iterative_over_solve"] = t_it / t_sv
    a, bb = nq.scf_target(H, S, op, n_occ).check(), nq.scf_target_iterative(H, S, op, n_occ).check()
    rec["scf_target_max_difference_DL"] = float((a.DL - bb.DL).abs().max())
    rec["scf_target_sp2_iterations_max"] = int(bb.purification.iterations.max())
    if args.model:
        rec["qhnet_step_16"] = leg_model(w, max(r, 3))
        print(json.dumps(dict(leg="qhnet_step_16", **rec["qhnet_step_16"])), flush=True)
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
