"""HOMO, LUMO and the gap without a solve (``BatchedPurification.frontier``, csrc/orbfrontier.hip) leg by leg, against the solver route and
``torch.linalg.eigvalsh`` IN THE SAME RUN, one process, HIP events, warm-up first, on the synthetic conformers of scripts/bench_orbital_loss.py with the gapped
matrices of scripts/bench_orbital_purify.py:

  (a) the purification the levels follow: orthogonaliser, then congruence + bounds + SP2 loop (``purify``);
  (b) the Lanczos launch (``nq_orb_front_lanczos``: one workgroup per molecule and side), with the steps taken per side;
  (c) the gram launch (``nq_orb_front_gram``: gH and gS);
  (d) ``BatchedOrbitals.solve`` + ``frontier`` on the same matrices;
  (e) ``torch.linalg.cholesky`` / ``solve_triangular`` / ``eigvalsh`` on dense blocks grouped by size, the regrouping by prebuilt index gather.

  With --model: the QHNet training step (config/qhnet.yaml sizes, 16 conformers) with a gap term through this route and through ``QHNetOrbitalLightning``'s
  way (``orbital_energies`` + ``OrbitalEnergyLoss("mae", "frontier")``), set up as in scripts/bench_orbital_purify.py.

No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_frontier.py --molecules 32 --model --out profiles/orbital_frontier_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_frontier.py --molecules 512 --append --out profiles/orbital_frontier_step.json
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


def leg_eigvalsh(st, H, S, n_occ, warmup, repeat):
    """HOMO and LUMO through ``torch.linalg`` per size group -> (record, homo [B], lumo [B])."""
    import torch
    dev = H.device
    groups = {}
    for b, m in enumerate(st.m.tolist()):
        groups.setdefault(int(m), []).append(b)
    pp = st.pack_ptr_host
    index = [(m, bs, torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev), torch.tensor([int(n_occ[b]) for b in bs], device=dev)) for m, bs in groups.items()]

    def step():
        homo, lumo = torch.empty(st.B, dtype=torch.float64, device=dev), torch.empty(st.B, dtype=torch.float64, device=dev)
        for m, bs, blk, no in index:
            nb = len(bs)
            L = torch.linalg.cholesky(S[blk].view(nb, m, m))
            Y = torch.linalg.solve_triangular(L, H[blk].view(nb, m, m), upper=False)
            A = torch.linalg.solve_triangular(L, Y.mT, upper=False)
            e = torch.linalg.eigvalsh(0.5 * (A + A.mT))
            homo[bs] = e.gather(1, (no - 1)[:, None])[:, 0]
            lumo[bs] = e.gather(1, no[:, None])[:, 0]
        return homo, lumo
    t, runs = event_ms(step, warmup, repeat)
    return (dict(ms=t, runs=runs, groups=len(groups), what="torch.linalg cholesky, two solve_triangular, eigvalsh per size group", regrouping="index gather, indices prebuilt"),) + step()


def leg_model(warmup, repeat, molecules=16):
    """The QHNet training step with a gap term through the purification + Lanczos route and through the solver; the set-up of scripts/bench_orbital_purify.py
    (an untrained network's prediction has no gap to speak of: both routes take their levels of ``H_gap + c p``)."""
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
    l_h, l_f, l_e, l_d = HamiltonianLoss(), nq.FrontierLoss("mae", "gap"), nq.OrbitalEnergyLoss("mae", "frontier"), nq.DensityMatrixLoss("mae")
    seen = {}

    def step(route):
        opt.zero_grad(set_to_none=True)
        p = net(b, packed=True)
        loss = l_h(p, target)
        Hp = H_gap + c * p.double()
        if route == "solver":
            eps_t = nq.BatchedOrbitals(op, "cuda").solve(H_t, S).energies
            loss = loss + 0.1 * l_e(nq.orbital_energies(Hp, S, op), eps_t, n_occ, op)
        elif route in ("frontier", "frontier_and_density"):
            pur_t = nq.BatchedPurification(op, "cuda")
            orth = pur_t.orthogonalize(S)
            lv_t = pur_t.purify(H_t, n_occ, 100, orth).frontier()
            sol = None
            if route == "frontier_and_density":
                D_p, sol = nq.purified_density_matrix(Hp, S, op, n_occ, orth, return_solution=True)
                loss = loss + 0.1 * l_d(D_p, pur_t.density(), op)
            homo, lumo, sol = nq.purified_frontier(Hp, S, op, n_occ, orth, solution=sol, return_solution=True)
            loss = loss + 0.1 * l_f(torch.stack((homo, lumo)), torch.stack((lv_t.homo, lv_t.lumo)), n_occ, op)
            seen["levels"] = (sol.levels, lv_t)
        loss.backward()
        opt.step()
    out = dict(molecules=molecules, m_mean=float(np.mean(ms)))
    for route in ("plain", "solver", "frontier", "frontier_and_density"):
        t, runs = event_ms(lambda: step(route), warmup, repeat)
        out[f"step_{route}_ms"], out[f"step_{route}_runs"] = t, runs
    lv_p, lv_t = seen["levels"]
    out["lanczos_steps_max"] = int(max(lv_p.iterations.max(), lv_t.iterations.max()))
    out["converged"] = bool((lv_p.converged == 1).all() and (lv_t.converged == 1).all())
    out["frontier_over_solver"] = out["step_frontier_ms"] / out["step_solver_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--model", action="store_true", help="also time the QHNet training step at 16 conformers with a gap term by both routes")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_frontier_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    assert torch.cuda.is_available(), "bench_orbital_frontier.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    n_occ = closed_shell_counts(ms, ne)
    probs = gapped_problems(ms, n_occ)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), n_occ_mean=float(np.mean(n_occ)), device=torch.cuda.get_device_name(0),
               k_max=256, tol="2^-44")
    w, r = args.warmup, args.repeat
    sq = np.asarray(ms, dtype=np.float64) ** 2

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)
        return t

    pur = nq.BatchedPurification(op, "cuda")
    leg("orthogonalizer", lambda: pur.orthogonalize(S), launches=1)
    orth = pur.orthogonalize(S)
    t_pur = leg("purify", lambda: pur.purify(H, n_occ, 100, orth), what="congruence, bounds and the SP2 loop")
    pur.purify(H, n_occ, 100, orth).check()
    rec["purify"]["sp2_iterations_mean"] = float(pur.iterations.float().mean())
    t_lan = leg("lanczos", lambda: pur.frontier(), launches=1, what="nq_orb_front_lanczos: both sides of every molecule")
    lv = pur.frontier()
    pur.frontier_check(lv)
    it = lv.iterations.cpu().numpy().astype(np.float64)
    rec["lanczos"].update(steps_homo_mean=float(it[:, 0].mean()), steps_homo_max=int(it[:, 0].max()), steps_lumo_mean=float(it[:, 1].mean()), steps_lumo_max=int(it[:, 1].max()),
                          matrix_bytes_read=float(3.0 * 8.0 * (sq[:, None] * it).sum()),
                          matrix_gbytes_per_s=float(3.0 * 8.0 * (sq[:, None] * it).sum() / (t_lan * 1e-3) / 1e9), what_bytes="3 m^2 doubles per step, the stored vectors not counted")
    g = torch.ones(len(ms), dtype=torch.float64, device="cuda")
    leg("gram", lambda: pur.frontier_gradients(lv, -g, g), launches=1, what="nq_orb_front_gram: gH and gS")
    leg("gram_without_overlap", lambda: pur.frontier_gradients(lv, -g, g, overlap=False), launches=1)
    rec["frontier_after_purify_over_purify"] = t_lan / t_pur
    orb = nq.BatchedOrbitals(op, "cuda")
    t_sol = leg("solve_and_frontier", lambda: orb.solve(H, S).frontier(n_occ), what="BatchedOrbitals.solve + frontier")
    sh, sl, _ = orb.solve(H, S).frontier(n_occ)
    rec["against_solver"] = dict(homo=float((lv.homo - sh).abs().max()), lumo=float((lv.lumo - sl).abs().max()))
    t_all = leg("orthogonalize_purify_frontier", lambda: pur.purify(H, n_occ, 100, pur.orthogonalize(S)).frontier(), what="the whole route from (H, S)")
    rec["route_over_solver"] = t_all / t_sol
    rec["torch_eigvalsh"], th, tl = leg_eigvalsh(pur.state, H, S, n_occ, w, r)
    rec["torch_eigvalsh"]["max_difference"] = float(max((lv.homo - th).abs().max(), (lv.lumo - tl).abs().max()))
    print(json.dumps(dict(leg="torch_eigvalsh", **rec["torch_eigvalsh"])), flush=True)
    rec["route_over_torch_eigvalsh"] = t_all / rec["torch_eigvalsh"]["ms"]
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
