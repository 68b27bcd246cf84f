"""Mayer bond orders and their reverse (nabladft_amd/orbital_loss.py ``bond_orders``, csrc/orbbond.hip) beside the solve they follow and against ``torch.bmm``,
one process, HIP events, warm-up first, on the synthetic conformers of scripts/bench_orbital_loss.py:

  (a) the solve: one launch of nq_orb_solve for the whole batch, and the density forward (one nq_orb_wgram launch);
  (b) the forward: nq_orb_bond_product (P = D S) and nq_orb_bond_reduce (table + valences), each alone and both as ``bond_orders`` runs them (with the
      allocation of their outputs);
  (c) the reverse, materialised E: nq_orb_bond_backward with and without the S half (E elementwise, then one launch for sym(E S) and sym(D E));
      the fused variant, which would form E while staging, is not built: its entry in the record says so;
  (d) ``bond_orders`` forward + backward through autograd, as a training step pays it;
  (e) the same quantities through ``torch.bmm`` on dense float64 blocks grouped by size: P = D S, the table as Ai (P o P^T) Ai^T with a 0/1 atom-indicator
      stack, P again and E = (Ai^T (Gamma + Gamma^T) Ai) o P^T, sym(E S), sym(D E); the regrouping is one index gather / scatter per group with the index tensors and the
      indicator stacks built beforehand.

Useful flops: 2 m^3 per molecule for P, and 2 m^3 for each of sym(E S) and sym(D E) (one m x m x m product each; the kernels compute the lower-triangle
tiles of two contractions, the same count).  No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_bond.py --molecules 32 --out profiles/orbital_bond_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_bond.py --molecules 512 --append --out profiles/orbital_bond_step.json
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


def leg_bmm(orb, D, S, gB, gV, atoms, per_atom, warmup, repeat):
    """The forward and the reverse through ``torch.bmm`` per size group -> (forward record, reverse record, bond [Q], gD [P], gS [P]).  The reverse forms
    ``P`` again (three products where the kernels' reverse, which is handed the stored ``P``, has two)."""
    import torch
    st = orb.state
    dev = st.coeff.device
    ms = st.m.tolist()
    aptr = np.concatenate([[0], np.cumsum(atoms)])
    bptr = np.concatenate([[0], np.cumsum(np.asarray(atoms, dtype=np.int64) ** 2)])
    groups = {}
    for b, m in enumerate(ms):
        groups.setdefault(int(m), []).append(b)
    pp = st.pack_ptr_host
    index = []
    for m, bs in groups.items():
        nmax = max(atoms[b] for b in bs)
        blk = torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev)          # [nb, m m] packed positions
        Ai = np.zeros((len(bs), nmax, m))
        gpos = np.zeros((len(bs), nmax, nmax), dtype=np.int64)       # where (A, B) of the padded table sits in the flat one (padding: entry 0, masked)
        gmask = np.zeros((len(bs), nmax, nmax))
        vpos = np.zeros((len(bs), nmax), dtype=np.int64)
        for i, b in enumerate(bs):
            o = 0
            n = atoms[b]
            for a in range(n):
                k = per_atom[aptr[b] + a]
                Ai[i, a, o:o + k] = 1.0
                o += k
            gpos[i, :n, :n] = bptr[b] + np.arange(n * n).reshape(n, n)
            gmask[i, :n, :n] = 1.0
            vpos[i, :n] = aptr[b] + np.arange(n)
        index.append((m, len(bs), nmax, blk, torch.from_numpy(Ai).to(dev), torch.from_numpy(gpos).to(dev), torch.from_numpy(gmask).to(dev),
                      torch.from_numpy(vpos).to(dev)))
    Q, P = int(bptr[-1]), int(pp[-1])

    def forward():
        bond = torch.zeros(Q, dtype=torch.float64, device=dev)
        for m, nb, nmax, blk, Ai, gpos, gmask, vpos in index:
            Pm = torch.bmm(D[blk].view(nb, m, m), S[blk].view(nb, m, m))
            Bt = torch.bmm(torch.bmm(Ai, Pm * Pm.mT), Ai.mT)
            bond[gpos[gmask > 0]] = Bt[gmask > 0]
        return bond

    def reverse():
        gD, gS = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        for m, nb, nmax, blk, Ai, gpos, gmask, vpos in index:
            Dm, Sm = D[blk].view(nb, m, m), S[blk].view(nb, m, m)
            Pm = torch.bmm(Dm, Sm)
            off = (1.0 - torch.eye(nmax, dtype=torch.float64, device=dev))[None]
            Gm = (gB[gpos] + off * gV[vpos][:, :, None]) * gmask
            E = torch.bmm(torch.bmm(Ai.mT, Gm + Gm.mT), Ai) * Pm.mT
            ES, DE = torch.bmm(E, Sm), torch.bmm(Dm, E)
            gD[blk] = (0.5 * (ES + ES.mT)).reshape(nb, m * m)
            gS[blk] = (0.5 * (DE + DE.mT)).reshape(nb, m * m)
        return gD, gS
    f_ms, f_runs = event_ms(forward, warmup, repeat)
    r_ms, r_runs = event_ms(reverse, warmup, repeat)
    common = dict(groups=len(groups), regrouping="index gather / scatter, indices and atom indicators prebuilt")
    gD, gS = reverse()
    return dict(ms=f_ms, runs=f_runs, **common), dict(ms=r_ms, runs=r_runs, what="P again, E, sym(E S), sym(D E)", **common), forward(), gD, gS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_bond_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals
    assert torch.cuda.is_available(), "bench_orbital_bond.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    probs = problems(ms)
    n_occ = closed_shell_counts(ms, ne)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    plan = SimpleNamespace(B=len(ms), N=sum(atoms), m_total=int(op[-1]), total=int(sum(m * m for m in ms)),
                           mol_ptr=torch.tensor(np.concatenate([[0], np.cumsum(atoms)]), dtype=torch.int32).cuda(),
                           orb_ptr=torch.tensor(np.concatenate([[0], np.cumsum(per_atom)]), dtype=torch.int64).cuda())
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), atoms_mean=float(np.mean(atoms)),
               orbitals_per_atom_max=int(max(per_atom)), device=torch.cuda.get_device_name(0))
    w, r = args.warmup, args.repeat
    flops = 2.0 * sum(float(m) ** 3 for m in ms)                  # one m x m x m product per molecule

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        if "products" in more:
            rec[name]["useful_tflops"] = more["products"] * flops / (t * 1e-3) / 1e12
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)

    orb = BatchedOrbitals(op, "cuda")
    leg("solve", lambda: orb.solve(H, S), launches=1)
    orb.check()
    leg("density_forward", lambda: orb.density(n_occ), launches=1)
    D = orb.density(n_occ)
    leg("product", lambda: orb.bond_product(D, S), launches=1, products=1)
    Pm = orb.bond_product(D, S)
    leg("reduce", lambda: orb.bond_reduce(Pm, plan), launches=2)
    leg("forward", lambda: orb.bond_orders(D, plan, S), launches=3, products=1)
    bond, val, _ = orb.bond_orders(D, plan, S)
    rng = np.random.Generator(np.random.PCG64(5))
    gB = torch.from_numpy(rng.normal(size=int(bond.numel()))).cuda()
    gV = torch.from_numpy(rng.normal(size=int(val.numel()))).cuda()
    leg("backward_materialised", lambda: orb.bond_orders_backward(plan, gB, gV, Pm, D, S, want_s=True), launches=2, products=2)
    leg("backward_materialised_without_overlap_gradient", lambda: orb.bond_orders_backward(plan, gB, gV, Pm, None, S), launches=2, products=1)
    rec["backward_fused"] = "not built: E is materialised by an elementwise launch"

    def autograd():
        Dl, Sl = D.detach().clone().requires_grad_(True), S.detach().clone().requires_grad_(True)
        b_, v_ = nq.bond_orders(Dl, plan, Sl, orb)
        ((b_ * gB).sum() + (v_ * gV).sum()).backward()
        return Dl.grad, Sl.grad
    leg("forward_backward_autograd", autograd, launches=5, products=3)
    kD, kS = autograd()
    rec["torch_bmm_forward"], rec["torch_bmm_backward"], tb, tD, tS = leg_bmm(orb, D, S, gB, gV, atoms, per_atom, w, r)
    for name, a, b in (("bond", bond, tb), ("gD", kD, tD), ("gS", kS, tS)):
        rec["torch_bmm_backward"]["max_difference_" + name] = float((a - b).abs().max())
        rec["torch_bmm_backward"]["max_abs_" + name] = float(a.abs().max())
    print(json.dumps(dict(leg="torch_bmm", forward=rec["torch_bmm_forward"], backward=rec["torch_bmm_backward"])), flush=True)
    rec["beside_the_solve"] = dict(forward_over_solve=rec["forward"]["ms"] / rec["solve"]["ms"],
                                   forward_backward_over_solve=rec["forward_backward_autograd"]["ms"] / rec["solve"]["ms"])
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
