"""The orbital-energy loss and the density / population calls (nabladft_amd/orbital_loss.py, csrc/orbdens.hip) beside the solve they follow, one process, HIP
events, warm-up first, on the synthetic conformers of scripts/bench_orbitals.py:

  (a) the solve: one launch of nq_orb_solve for the whole batch (what the forward of ``orbital_energies`` costs);
  (b) the backward: ONE launch of nq_orb_wgram for gH and gS together (two weight vectors from the same operand loads);
  (c) ``density(n_occ, energy_weighted=True)`` + ``populations(D, plan, S, H)``: one nq_orb_wgram and one nq_orb_population launch;
  (d) the alternative to (b) for the same blocks on the device: ``torch.bmm`` on dense float64 copies grouped by size -- the regrouping (one index gather of
      the blocks of a size into a stack, one index scatter of each result back into the packed layout; the index tensors prebuilt) is part of it;
  With --model: the QHNet training step (config/qhnet.yaml sizes, 16 conformers) with the matrix loss alone and with the orbital term added the way
  ``QHNetOrbitalLightning`` adds it (predicted and target solve under a common overlap, ``OrbitalEnergyLoss``, the wgram backward).

No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_loss.py --molecules 32 --model --out profiles/orbital_loss_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_loss.py --molecules 512 --append --out profiles/orbital_loss_step.json
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

from scripts.bench_orbitals import event_ms, problems  # noqa: E402
from scripts.bench_qhnet import ORBITALS  # noqa: E402


def conformers(molecules, seed=7):
    """-> (orbitals per molecule, atoms per molecule, orbitals per atom, electrons per molecule) of the bench generator's conformers."""
    import torch
    from nabladft_amd.synth import gen_conformers
    _, z, batch, _, _ = gen_conformers(seed, molecules)
    per_atom = torch.tensor([sum(2 * l + 1 for l in ORBITALS[int(a)]) for a in z.tolist()])
    zero = torch.zeros(molecules, dtype=torch.long)
    ms = zero.clone().index_add_(0, batch, per_atom)
    ne = zero.clone().index_add_(0, batch, z.long())
    return ms.tolist(), torch.bincount(batch, minlength=molecules).tolist(), per_atom.tolist(), ne.tolist()


def closed_shell_counts(ms, ne):
    """Occupied orbitals of the synthetic conformers: half the electrons (an odd count loses one: the cost does not depend on it), within 1..m."""
    return [min(m, max(1, e // 2)) for m, e in zip(ms, ne)]


def leg_bmm(orb, g, warmup, repeat):
    """``torch.bmm`` per size group.  The regrouping is one index gather of the blocks of a size into a stack and one index scatter of each result back into
    the packed layout; the index tensors are built once per batch composition, outside the timed region (as a plan would hold them)."""
    import torch
    st = orb.state
    dev = st.coeff.device
    groups = {}
    for b, m in enumerate(st.m.tolist()):
        groups.setdefault(int(m), []).append(b)
    pp, op = st.pack_ptr_host, st.orb_ptr_host
    index = []
    for m, bs in groups.items():
        blk = torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev)          # [nb, m m] packed positions
        orbs = torch.from_numpy(np.stack([np.arange(op[b], op[b + 1]) for b in bs])).to(dev)         # [nb, m]
        index.append((m, len(bs), blk, orbs))
    w1 = -(st.eps * g)

    def run():
        gH, gS = torch.empty_like(st.coeff), torch.empty_like(st.coeff)
        for m, nb, blk, orbs in index:
            Cs = st.coeff[blk].view(nb, m, m)                                                         # [nb, m (orbital k), m]
            Ct = Cs.transpose(1, 2)
            gH[blk] = torch.bmm(Ct * g[orbs][:, None, :], Cs).view(nb, m * m)
            gS[blk] = torch.bmm(Ct * w1[orbs][:, None, :], Cs).view(nb, m * m)
        return gH, gS
    ms_, all_ms = event_ms(run, warmup, repeat)
    return dict(ms=ms_, runs=all_ms, groups=len(groups), regrouping="index gather / scatter, indices prebuilt"), run()


def leg_model(warmup, repeat, molecules=16):
    """The QHNet training step with and without the orbital term, on device-resident targets and overlaps."""
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
    l_h, l_o = HamiltonianLoss(), nq.OrbitalEnergyLoss("mae", "occupied")

    def step(orbital):
        opt.zero_grad(set_to_none=True)
        p = net(b, packed=True)
        loss = l_h(p, target)
        if orbital:
            eps_p = nq.orbital_energies(p, S, op)
            eps_t = nq.BatchedOrbitals(op, "cuda").solve(target, S).energies
            loss = loss + 0.1 * l_o(eps_p, eps_t, n_occ, op)
        loss.backward()
        opt.step()
    plain, plain_runs = event_ms(lambda: step(False), warmup, repeat)
    both, both_runs = event_ms(lambda: step(True), warmup, repeat)
    return dict(molecules=molecules, m_mean=float(np.mean(ms)), step_ms=plain, step_runs=plain_runs, step_with_orbital_term_ms=both, step_with_orbital_term_runs=both_runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--model", action="store_true", help="also time the QHNet training step at 16 conformers with and without the orbital term")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_loss_step.json"))
    args = ap.parse_args()
    import torch
    from nabladft_amd.orbitals import BatchedOrbitals
    assert torch.cuda.is_available(), "bench_orbital_loss.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    probs = problems(ms)
    n_occ = closed_shell_counts(ms, ne)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    plan = SimpleNamespace(B=len(ms), N=sum(atoms), m_total=int(op[-1]), total=int(sum(m * m for m in ms)),
                           mol_ptr=torch.tensor(np.concatenate([[0], np.cumsum(atoms)]), dtype=torch.int32).cuda(),
                           orb_ptr=torch.tensor(np.concatenate([[0], np.cumsum(per_atom)]), dtype=torch.int64).cuda())
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), device=torch.cuda.get_device_name(0))
    orb = BatchedOrbitals(op, "cuda")
    t, runs = event_ms(lambda: orb.solve(H, S), args.warmup, args.repeat)
    orb.check()
    rec["solve"] = dict(ms=t, runs=runs, launches=1)
    print(json.dumps(dict(leg="a", **rec["solve"])), flush=True)
    g = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).normal(size=int(op[-1]))).cuda()
    t, runs = event_ms(lambda: orb.weighted_gram(g, -(orb.energies * g)), args.warmup, args.repeat)
    flops = 2.0 * 2.0 * sum(float(m) ** 3 for m in ms) / 2.0          # two weight vectors, the lower triangle
    rec["wgram_backward"] = dict(ms=t, runs=runs, launches=1, useful_tflops=flops / (t * 1e-3) / 1e12)
    print(json.dumps(dict(leg="b", **rec["wgram_backward"])), flush=True)

    def dens():
        D, W = orb.density(n_occ, energy_weighted=True)
        return orb.populations(D, plan, S, H)
    t, runs = event_ms(dens, args.warmup, args.repeat)
    pop, nelec, eband = dens()
    rec["density_populations"] = dict(ms=t, runs=runs, launches=2, nelec_max_error=float((nelec - 2.0 * torch.tensor(n_occ, dtype=torch.float64).cuda()).abs().max()))
    print(json.dumps(dict(leg="c", **rec["density_populations"])), flush=True)
    rec["torch_bmm"], (bH, bS) = leg_bmm(orb, g, args.warmup, args.repeat)
    kH, kS = orb.weighted_gram(g, -(orb.energies * g))
    rec["torch_bmm"]["max_difference_gH"] = float((kH - bH).abs().max())
    rec["torch_bmm"]["max_difference_gS"] = float((kS - bS).abs().max())
    print(json.dumps(dict(leg="d", **rec["torch_bmm"])), flush=True)
    if args.model:
        rec["qhnet_step"] = leg_model(args.warmup, args.repeat)
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
