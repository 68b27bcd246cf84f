"""The SCF-residual loss (nabladft_amd/orbital_loss.py ``commutator`` / ``scf_residual``, csrc/orbcomm.hip) leg by leg and against ``torch.bmm``, one process, HIP
events, warm-up first, on the synthetic conformers of scripts/bench_orbital_loss.py:

  (a) the commutator forward (nq_orb_comm_product on two symmetric operands) and each reverse (the same kernel on an antisymmetric first operand, alpha = +1
      for dL/dX and -1 for dL/dY);
  (b) nq_orb_comm_antisymmetrize and nq_orb_comm_norms;
  (c) ``scf_residual_to_target`` forward + backward through autograd with a cached ``ScfTarget`` (two congruence products and one commutator forward; the
      antisymmetric part, one commutator and the congruence's reverse backward), and ``scf_target`` itself (one target solve, one decomposition of S);
  (d) the same loss through ``torch.bmm`` autograd on dense float64 blocks grouped by size, S^(-1/2) and the target's Löwdin density given; the regrouping is one
      index gather / scatter per group with the indices built beforehand.

  With --model: the QHNet training step (config/qhnet.yaml sizes, 16 conformers) with the residual term, cached and uncached, and IN THE SAME RUN the density
  term through ``QHNetDensityLightning``'s route (one solve per side) and through ``QHNetPurifiedDensityLightning``'s, set up as in
  scripts/bench_orbital_purify.py (whose text explains why the routes take H_gap + c p).

Useful flops: 2 m^3 per molecule and m x m x m product; a commutator is two products of which the kernel computes the lower triangle only, so it is counted
as ONE (2 m^3 per molecule: 2 products x 1/2).  No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_commutator.py --molecules 32 --model --out profiles/orbital_commutator_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_commutator.py --molecules 512 --append --out profiles/orbital_commutator_step.json
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


def leg_bmm(orb, H, Ai, DL, G, warmup, repeat):
    """Forward + backward of sum G o R + 1/2 |R|^2, R = [A^- H A^-, D^L], through ``torch.bmm`` autograd per size group -> (record, gH [P])."""
    import torch
    st = orb.state
    dev = st.coeff.device
    groups = {}
    for b, m in enumerate(st.m.tolist()):
        groups.setdefault(int(m), []).append(b)
    pp = st.pack_ptr_host
    index = [(m, len(bs), torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev)) for m, bs in groups.items()]
    P = int(pp[-1])

    def step():
        gH = torch.empty(P, dtype=torch.float64, device=dev)
        for m, nb, blk in index:
            Hm = H[blk].view(nb, m, m).clone().requires_grad_(True)
            Am, Dm, Gm = Ai[blk].view(nb, m, m), DL[blk].view(nb, m, m), G[blk].view(nb, m, m)
            HL = torch.bmm(torch.bmm(Am, 0.5 * (Hm + Hm.mT)), Am)
            R = torch.bmm(HL, Dm) - torch.bmm(Dm, HL)
            ((Gm * R).sum() + 0.5 * (R * R).sum()).backward()
            gH[blk] = (0.5 * (Hm.grad + Hm.grad.mT)).reshape(nb, m * m)
        return gH
    t, runs = event_ms(step, warmup, repeat)
    return dict(ms=t, runs=runs, groups=len(groups), what="S^(-1/2) and D^L given: congruence, commutator, autograd backward",
                regrouping="index gather / scatter, indices prebuilt"), step()


def leg_model(warmup, repeat, molecules=16):
    """The QHNet training step with the residual term (cached and uncached target) and, for comparison in the same run, with a density term through the solver
    and through purification; device-resident targets and overlaps, the set-up of scripts/bench_orbital_purify.py."""
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
    ne = torch.zeros(molecules, dtype=torch.long).index_add_(0, b.batch.cpu(), b.z.cpu().long()).tolist()
    n_occ = closed_shell_counts(ms, ne)
    probs = gapped_problems(ms, n_occ)
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    H_gap = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    c = 0.05 / (float(pred.abs().max()) * max(ms))
    H_t = (H_gap + c * target.double()).detach()
    opt = torch.optim.AdamW(net.parameters(), lr=5e-4, betas=(0.9, 0.95), amsgrad=True)
    l_h, l_d, l_r = HamiltonianLoss(), nq.DensityMatrixLoss("mae"), nq.ScfResidualLoss("mse")
    cached = nq.scf_target(H_t, S, op, n_occ)

    def step(route):
        opt.zero_grad(set_to_none=True)
        p = net(b, packed=True)
        loss = l_h(p, target)
        if route == "solver":
            D_p = nq.density_matrix(H_gap + c * p.double(), S, op, n_occ)
            D_t = nq.BatchedOrbitals(op, "cuda").solve(H_t, S).density(n_occ)
            loss = loss + 0.1 * l_d(D_p, D_t, op)
        elif route == "purify":
            pur_t = nq.BatchedPurification(op, "cuda")
            orth = pur_t.orthogonalize(S)
            D_t = pur_t.purify(H_t, n_occ, 100, orth).density()
            D_p = nq.purified_density_matrix(H_gap + c * p.double(), S, op, n_occ, orth)
            loss = loss + 0.1 * l_d(D_p, D_t, op)
        elif route.startswith("residual"):
            tgt = cached if route == "residual_cached" else nq.scf_target(H_t, S, op, n_occ)
            loss = loss + 0.1 * l_r(nq.scf_residual_to_target(H_gap + c * p.double(), tgt), None, op)
        loss.backward()
        opt.step()
    out = dict(molecules=molecules, m_mean=float(np.mean(ms)))
    for route in ("plain", "residual_cached", "residual_uncached", "solver", "purify"):
        t, runs = event_ms(lambda: step(route), warmup, repeat)
        out[f"step_{route}_ms"], out[f"step_{route}_runs"] = t, runs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--model", action="store_true", help="also time the QHNet training step at 16 conformers with the residual term and with the two density routes")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_commutator_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals
    assert torch.cuda.is_available(), "bench_orbital_commutator.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    n_occ = closed_shell_counts(ms, ne)
    probs = gapped_problems(ms, n_occ)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), device=torch.cuda.get_device_name(0))
    w, r = args.warmup, args.repeat
    flops = 2.0 * sum(float(m) ** 3 for m in ms)

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        if "products" in more:
            rec[name]["useful_tflops"] = more["products"] * flops / (t * 1e-3) / 1e12
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)

    leg("scf_target", lambda: nq.scf_target(H, S, op, n_occ), what="one target solve, one decomposition of S, weights + wgram, the target's congruence")
    target = nq.scf_target(H, S, op, n_occ)
    target.basis.check()
    orb = BatchedOrbitals(op, "cuda")                              # the layout alone: nothing is solved for the legs below
    rng = np.random.Generator(np.random.PCG64(5))
    Hp = (H + 0.02 * float(H.abs().max()) * torch.from_numpy(np.concatenate([(lambda x: 0.5 * (x + x.T))(rng.normal(size=(m, m))).ravel() for m in ms])).cuda())
    G = torch.from_numpy(np.concatenate([rng.normal(size=(m, m)).ravel() for m in ms])).cuda()
    HL = orb.sym_congruence(target.basis.inv_half, Hp)[0]
    DL = target.DL
    leg("comm_product_forward", lambda: orb.commutator(HL, DL), launches=1, products=1)
    leg("antisymmetrize", lambda: orb.antisymmetrize(G), launches=1)
    Ga = orb.antisymmetrize(G)
    leg("comm_product_reverse_dX", lambda: orb.commutator(Ga, DL, True, 1.0), launches=1, products=1)
    leg("comm_product_reverse_dY", lambda: orb.commutator(Ga, HL, True, -1.0), launches=1, products=1)
    R = orb.commutator(HL, DL)
    leg("norms", lambda: orb.commutator_norms(R), launches=1)
    leg("congruence", lambda: orb.sym_congruence(target.basis.inv_half, Hp), launches=2, products=2)

    def autograd():
        Hl = Hp.detach().clone().requires_grad_(True)
        Rl = nq.scf_residual_to_target(Hl, target)
        ((G * Rl).sum() + 0.5 * (Rl * Rl).sum()).backward()
        return Hl.grad
    leg("forward_backward_autograd_cached_target", autograd, launches=8, products=6,
        what="forward: product, symprod, commutator; backward: antisymmetrize, commutator, symmetrize, product, symprod")
    kH = autograd()
    rec["torch_bmm_autograd"], tH = leg_bmm(orb, Hp, target.basis.inv_half, DL, G, w, r)
    rec["torch_bmm_autograd"]["max_difference_gH"] = float((kH - tH).abs().max())
    rec["torch_bmm_autograd"]["max_abs_gH"] = float(kH.abs().max())
    print(json.dumps(dict(leg="torch_bmm_autograd", **rec["torch_bmm_autograd"])), flush=True)
    rec["against_torch_bmm_autograd"] = rec["forward_backward_autograd_cached_target"]["ms"] / rec["torch_bmm_autograd"]["ms"]
    sumsq, top = orb.commutator_norms(R)
    rec["residual"] = dict(rms_mean=float((sumsq.sqrt() / torch.from_numpy(np.asarray(ms, dtype=np.float64)).cuda()).mean()), diis_error_mean=float(top.mean()))
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
