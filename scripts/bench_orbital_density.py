"""The density response and the population gradients (nabladft_amd/orbital_loss.py, csrc/orbresp.hip) beside the solve they follow, one process, HIP events,
warm-up first, on the synthetic conformers of scripts/bench_orbital_loss.py:

  (a) the solve: one launch of nq_orb_solve for the whole batch;
  (b) the backward of the energies: one launch of nq_orb_wgram for gH and gS;
  (c) the density forward: ``density(n_occ)``, one nq_orb_wgram launch;
  (d) the response chain for gH and gS: nq_orb_resp_project (symmetrise + project), nq_orb_resp_mo, nq_orb_resp_back, nq_orb_syr2k, each alone and all four
      as ``density_response`` runs them (with the allocation of their scratch arrays);
  (e) ``populations(D, plan, S, H)`` forward + backward through autograd (nq_orb_population, nq_orb_population_backward);
  (f) the alternative on the device: the same loss ``sum G o D`` through ``torch.linalg`` autograd (cholesky, two triangular solves, ``eigh``, back
      substitution, masked occupied columns), grouped by size -- forward AND backward, since that route has no separate solve; the regrouping is one index
      gather / scatter per group with the index tensors built beforehand;
  With --model: the QHNet training step (config/qhnet.yaml sizes, 16 conformers) with the matrix loss alone and with a density term added the way
  ``QHNetDensityLightning`` adds it (one solve per side, ``DensityMatrixLoss``, the response chain in the backward).

No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_density.py --molecules 32 --model --out profiles/orbital_density_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_density.py --molecules 512 --append --out profiles/orbital_density_step.json
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scripts.bench_orbital_loss import closed_shell_counts, conformers  # noqa: E402
from scripts.bench_orbitals import event_ms, problems  # noqa: E402


def leg_eigh(orb, H, S, G, n_occ, warmup, repeat):
    """``sum G o D`` through torch.linalg autograd per size group -> (record, gH packed)."""
    import torch
    st = orb.state
    dev = st.coeff.device
    groups = {}
    for b, m in enumerate(st.m.tolist()):
        groups.setdefault(int(m), []).append(b)
    pp = st.pack_ptr_host
    index = []
    for m, bs in groups.items():
        blk = torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev)          # [nb, m m] packed positions
        occ = (torch.arange(m)[None, :] < torch.tensor([n_occ[b] for b in bs])[:, None]).to(dev, torch.float64)      # [nb, m]: 1 over the occupied orbitals
        index.append((m, len(bs), blk, occ))

    def run():
        Hl = H.detach().clone().requires_grad_(True)
        total = 0.0
        for m, nb, blk, occ in index:
            Hs, Ss, Gs = Hl[blk].view(nb, m, m), S[blk].view(nb, m, m), G[blk].view(nb, m, m)
            L = torch.linalg.cholesky(Ss)
            X = torch.linalg.solve_triangular(L, Hs, upper=False)
            A = torch.linalg.solve_triangular(L, X.mT, upper=False).mT
            _, Y = torch.linalg.eigh(0.5 * (A + A.mT))
            Co = torch.linalg.solve_triangular(L.mT, Y, upper=True) * occ[:, None, :]
            total = total + (Gs * (2.0 * Co @ Co.mT)).sum()
        total.backward()
        return Hl.grad
    ms_, runs = event_ms(run, warmup, repeat)
    return dict(ms=ms_, runs=runs, groups=len(groups), regrouping="index gather / scatter, indices prebuilt", what="forward and backward"), run()


def leg_model(warmup, repeat, molecules=16):
    """The QHNet training step with and without the density term, on device-resident targets and overlaps."""
    import torch
    import nabladft_amd as nq
    from nabladft_amd.hamiltonian import HamiltonianLoss
    from scripts.bench_qhnet import build, synthetic_batch
    net = build("cuda")
    b = synthetic_batch(molecules, 7, "cuda")
    with torch.no_grad():
        pred = net(b, packed=True)
    plan = net.last_plan
    op = plan.mol_orb_ptr.cpu().numpy()
    ms = np.diff(op).tolist()
    target = (pred + 0.05 * torch.randn(pred.shape, generator=torch.Generator().manual_seed(1)).cuda()).detach()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in problems(ms)]).astype(np.float32)).cuda()
    ne = torch.zeros(molecules, dtype=torch.long).index_add_(0, b.batch.cpu(), b.z.cpu().long()).tolist()
    n_occ = closed_shell_counts(ms, ne)
    opt = torch.optim.AdamW(net.parameters(), lr=5e-4, betas=(0.9, 0.95), amsgrad=True)
    l_h, l_d = HamiltonianLoss(), nq.DensityMatrixLoss("mae")

    def step(density):
        opt.zero_grad(set_to_none=True)
        p = net(b, packed=True)
        loss = l_h(p, target)
        if density:
            D_p = nq.density_matrix(p, S, op, n_occ)
            D_t = nq.BatchedOrbitals(op, "cuda").solve(target, S).density(n_occ)
            loss = loss + 0.1 * l_d(D_p, D_t, op)
        loss.backward()
        opt.step()
    plain, plain_runs = event_ms(lambda: step(False), warmup, repeat)
    both, both_runs = event_ms(lambda: step(True), warmup, repeat)
    return dict(molecules=molecules, m_mean=float(np.mean(ms)), step_ms=plain, step_runs=plain_runs, step_with_density_term_ms=both, step_with_density_term_runs=both_runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--model", action="store_true", help="also time the QHNet training step at 16 conformers with and without the density term")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_density_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals
    assert torch.cuda.is_available(), "bench_orbital_density.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    probs = problems(ms)
    n_occ = closed_shell_counts(ms, ne)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    plan = SimpleNamespace(B=len(ms), N=sum(atoms), m_total=int(op[-1]), total=int(sum(m * m for m in ms)),
                           mol_ptr=torch.tensor(np.concatenate([[0], np.cumsum(atoms)]), dtype=torch.int32).cuda(),
                           orb_ptr=torch.tensor(np.concatenate([[0], np.cumsum(per_atom)]), dtype=torch.int64).cuda())
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), n_occ_mean=float(np.mean(n_occ)),
               device=torch.cuda.get_device_name(0))
    w, r = args.warmup, args.repeat

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)

    orb = BatchedOrbitals(op, "cuda")
    leg("solve", lambda: orb.solve(H, S), launches=1)
    orb.check()
    rng = np.random.Generator(np.random.PCG64(5))
    g = torch.from_numpy(rng.normal(size=int(op[-1]))).cuda()
    G = torch.from_numpy(rng.normal(size=int(H.numel()))).cuda()
    leg("eps_backward", lambda: orb.weighted_gram(g, -(orb.energies * g)), launches=1)
    leg("density_forward", lambda: orb.density(n_occ), launches=1)
    lay = orb.occupied_layout(n_occ)
    flops = 2.0 * sum(float(n) * m * m for n, m in zip(n_occ, ms))       # one n_occ x m x m product
    T = orb.resp_project(G, lay)
    A_H, A_S = orb.resp_mo(T, lay)
    Rt_H, Rt_S = orb.resp_back(A_H, A_S, lay)
    chain = {}
    for name, fn, products in (("project", lambda: orb.resp_project(G, lay), 1), ("mo", lambda: orb.resp_mo(T, lay), 1),
                               ("back", lambda: orb.resp_back(A_H, A_S, lay), 2), ("syr2k", lambda: orb.syr2k(Rt_H, Rt_S, lay), 2)):
        t, runs = event_ms(fn, w, r)
        chain[name] = dict(ms=t, runs=runs, useful_tflops=products * flops / (t * 1e-3) / 1e12)
    t, runs = event_ms(lambda: orb.density_response(G, lay), w, r)
    chain["total"] = dict(ms=t, runs=runs, launches=5, useful_tflops=6.0 * flops / (t * 1e-3) / 1e12)
    t, runs = event_ms(lambda: orb.density_response(G, lay, False), w, r)
    chain["total_without_overlap_gradient"] = dict(ms=t, runs=runs, launches=5)
    rec["response_chain"] = chain
    print(json.dumps(dict(leg="response_chain", **chain)), flush=True)
    D = orb.density(n_occ)

    def pops():
        Dl, Sl, Hl = (x.detach().clone().requires_grad_(True) for x in (D, S, H))
        pop, nelec, eband = nq.populations(Dl, plan, Sl, Hl, orb)
        (pop.sum() + nelec.sum() + eband.sum()).backward()
        return Dl.grad
    leg("populations_forward_backward", pops, launches=2)
    rec["torch_eigh_autograd"], eH = leg_eigh(orb, H, S, G, n_occ, w, r)
    kH = orb.density_response(G, lay, False)[0]
    rec["torch_eigh_autograd"]["max_difference_gH"] = float((kH - eH).abs().max())
    rec["torch_eigh_autograd"]["max_abs_gH"] = float(kH.abs().max())
    print(json.dumps(dict(leg="torch_eigh_autograd", **rec["torch_eigh_autograd"])), flush=True)
    if args.model:
        rec["qhnet_step"] = leg_model(w, r)
        print(json.dumps(dict(leg="model", **rec["qhnet_step"])), flush=True)
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
