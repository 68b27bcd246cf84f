"""Löwdin populations, Wiberg indices and their reverse (nabladft_amd/orbital_loss.py ``lowdin_*``, csrc/orblowdin.hip) leg by leg and against
``torch.linalg.eigh`` autograd, one process, HIP events, warm-up first, on the synthetic conformers of scripts/bench_orbital_loss.py:

  (a) the decomposition of S: one launch of nq_orb_solve (the standard problem) for the whole batch -- latency-bound, expected to dominate at 32 molecules;
  (b) the matrix functions: nq_orb_low_weights and ONE nq_orb_wgram launch for S^(1/2) and S^(-1/2);
  (c) the congruence S^(1/2) D S^(1/2): nq_orb_low_product and nq_orb_low_symprod, each alone and both;
  (d) the populations (nq_orb_population without S) and the bond table (nq_orb_bond_product without S, nq_orb_bond_reduce) of the Löwdin density;
  (e) each reverse leg: of the congruence (dL/dM: two launches, dL/dX: one) and of the matrix function (nq_orb_resp_project, nq_orb_low_mo, nq_orb_smear_back,
      nq_orb_syr2k over all orbital pairs);
  (f) forward + backward through autograd with a given ``LowdinBasis`` (what a step pays when the basis is cached with the conformer; no gradient of S) and
      including ``lowdin_basis`` (what it pays otherwise, with the gradient of S); the difference of the latter and (a) is recorded as the in-step remainder;
  (g) the same loss through ``torch.linalg.eigh`` autograd on dense float64 blocks grouped by size: eigh of S, U sqrt(s) U^T, the congruence, the populations and
      the table with a 0/1 atom-indicator stack; the regrouping is one index gather / scatter per group with the indices built beforehand; and the same with
      S^(1/2) given as a constant (no eigh, no gradient of S), which is what the cached-basis leg of (f) is compared with.

Useful flops: 2 m^3 per molecule and m x m x m product.  No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_lowdin.py --molecules 32 --out profiles/orbital_lowdin_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_lowdin.py --molecules 512 --append --out profiles/orbital_lowdin_step.json
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


def leg_eigh(orb, D, S, gq, gW, atoms, per_atom, warmup, repeat, A_given=None):
    """Forward + backward of sum gq q + sum gW W through ``torch.linalg.eigh`` autograd per size group -> (record, gD [P], gS [P]).  ``A_given``: S^(1/2) packed
    [P], taken as a constant: no eigh and no gradient of S (gS None), the torch counterpart of a step with a cached basis."""
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
        blk = torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev)
        Ai = np.zeros((len(bs), nmax, m))
        gpos = np.zeros((len(bs), nmax, nmax), dtype=np.int64)
        gmask = np.zeros((len(bs), nmax, nmax))
        vpos = np.zeros((len(bs), nmax), dtype=np.int64)
        vmask = np.zeros((len(bs), nmax))
        for i, b in enumerate(bs):
            o, n = 0, atoms[b]
            for a in range(n):
                k = per_atom[aptr[b] + a]
                Ai[i, a, o:o + k] = 1.0
                o += k
            gpos[i, :n, :n] = bptr[b] + np.arange(n * n).reshape(n, n)
            gmask[i, :n, :n] = 1.0
            vpos[i, :n] = aptr[b] + np.arange(n)
            vmask[i, :n] = 1.0
        index.append((m, len(bs), blk, torch.from_numpy(Ai).to(dev), torch.from_numpy(gpos).to(dev), torch.from_numpy(gmask).to(dev), torch.from_numpy(vpos).to(dev),
                      torch.from_numpy(vmask).to(dev)))
    P = int(pp[-1])

    def step():
        gD, gS = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        for m, nb, blk, Ai, gpos, gmask, vpos, vmask in index:
            Dm = D[blk].view(nb, m, m).clone().requires_grad_(True)
            if A_given is None:
                Sm = S[blk].view(nb, m, m).clone().requires_grad_(True)
                s, Uv = torch.linalg.eigh(0.5 * (Sm + Sm.mT))
                A = (Uv * torch.sqrt(s)[:, None, :]) @ Uv.mT
            else:
                A = A_given[blk].view(nb, m, m)
            DL = A @ Dm @ A
            q = torch.bmm(Ai, torch.diagonal(DL, dim1=1, dim2=2)[:, :, None])[:, :, 0]
            W = torch.bmm(torch.bmm(Ai, DL * DL), Ai.mT)
            ((gq[vpos] * vmask * q).sum() + (gW[gpos] * gmask * W).sum()).backward()
            gD[blk] = (0.5 * (Dm.grad + Dm.grad.mT)).reshape(nb, m * m)
            if A_given is None:
                gS[blk] = (0.5 * (Sm.grad + Sm.grad.mT)).reshape(nb, m * m)
        return gD, (gS if A_given is None else None)
    t, runs = event_ms(step, warmup, repeat)
    gD, gS = step()
    what = ("eigh of S, U sqrt(s) U^T, " if A_given is None else "S^(1/2) given, no gradient of S: ") + "congruence, populations, table, autograd backward"
    return dict(ms=t, runs=runs, groups=len(groups), what=what,
                regrouping="index gather / scatter, indices and atom indicators prebuilt"), gD, gS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_lowdin_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals, LowdinBasis
    assert torch.cuda.is_available(), "bench_orbital_lowdin.py needs the MI355X"
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
    flops = 2.0 * sum(float(m) ** 3 for m in ms)

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        if "products" in more:
            rec[name]["useful_tflops"] = more["products"] * flops / (t * 1e-3) / 1e12
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)

    sol = BatchedOrbitals(op, "cuda").solve(H, S).check()
    D = sol.density(n_occ)
    orb = BatchedOrbitals(op, "cuda")
    leg("decomposition_of_S", lambda: orb.solve(S), launches=1)
    orb.check()
    leg("weights_and_wgram", lambda: orb.overlap_functions(), launches=2, products=2)
    basis = LowdinBasis(orb, *orb.overlap_functions()).check()
    A = basis.half
    leg("congruence_product", lambda: orb.low_product(D, A), launches=1, products=1)
    Y = orb.low_product(D, A)
    leg("congruence_symprod", lambda: orb.low_symprod(Y, A, 0), launches=1, products=1)
    leg("congruence", lambda: orb.sym_congruence(A, D), launches=2, products=2)
    DL = orb.sym_congruence(A, D)[0]
    leg("populations", lambda: orb.populations(DL, plan), launches=1)
    leg("bond_orders", lambda: orb.bond_orders(DL, plan), launches=3)
    pop = orb.populations(DL, plan)[0]
    bond = orb.bond_orders(DL, plan)[0]
    rng = np.random.Generator(np.random.PCG64(5))
    gq = torch.from_numpy(rng.normal(size=int(pop.numel()))).cuda()
    gW = torch.from_numpy(rng.normal(size=int(bond.numel()))).cuda()
    G = torch.from_numpy(np.concatenate([(lambda x: 0.5 * (x + x.T))(rng.normal(size=(m, m))).ravel() for m in ms])).cuda()
    Gn = torch.from_numpy(np.concatenate([rng.normal(size=(m, m)).ravel() for m in ms])).cuda()
    leg("symmetrize", lambda: orb.low_symmetrize(Gn), launches=1)
    leg("congruence_backward_dM", lambda: orb.sym_congruence_backward(G, A, Y, True, False), launches=2, products=2)
    leg("congruence_backward_dX", lambda: orb.sym_congruence_backward(G, A, Y, False, True), launches=1, products=1)
    gX = orb.sym_congruence_backward(G, A, Y, False, True)[1]
    leg("matfun_response", lambda: orb.matfun_response(gX, 0), launches=4, products=4)

    def autograd(with_basis):
        Dl, Sl = D.detach().clone().requires_grad_(True), S.detach().clone().requires_grad_(True)
        bs = nq.lowdin_basis(Sl, op) if with_basis else basis
        q_ = nq.lowdin_populations(Dl, plan, bs)[0]
        b_ = nq.lowdin_bond_orders(Dl, plan, bs)[0]
        ((q_ * gq).sum() + (b_ * gW).sum()).backward()
        return Dl.grad, Sl.grad
    leg("forward_backward_autograd_cached_basis", lambda: autograd(False), gradient_of_S=False)
    leg("forward_backward_autograd_with_basis", lambda: autograd(True))
    kD, kS = autograd(True)
    rec["torch_eigh_autograd"], tD, tS = leg_eigh(orb, D, S, gq, gW, atoms, per_atom, w, r)
    for name, a, b in (("gD", kD, tD), ("gS", kS, tS)):
        rec["torch_eigh_autograd"]["max_difference_" + name] = float((a - b).abs().max())
        rec["torch_eigh_autograd"]["max_abs_" + name] = float(a.abs().max())
    print(json.dumps(dict(leg="torch_eigh_autograd", **rec["torch_eigh_autograd"])), flush=True)
    rec["torch_autograd_given_half"], tD2, _ = leg_eigh(orb, D, S, gq, gW, atoms, per_atom, w, r, A_given=basis.half)
    rec["torch_autograd_given_half"]["max_difference_gD"] = float((autograd(False)[0] - tD2).abs().max())
    print(json.dumps(dict(leg="torch_autograd_given_half", **rec["torch_autograd_given_half"])), flush=True)
    rec["in_step_remainder_ms"] = rec["forward_backward_autograd_with_basis"]["ms"] - rec["decomposition_of_S"]["ms"]
    rec["against_torch_eigh_autograd"] = dict(with_basis=rec["forward_backward_autograd_with_basis"]["ms"] / rec["torch_eigh_autograd"]["ms"],
                                              cached_basis_against_given_half=rec["forward_backward_autograd_cached_basis"]["ms"] / rec["torch_autograd_given_half"]["ms"],
                                              decomposition_share=rec["decomposition_of_S"]["ms"] / rec["forward_backward_autograd_with_basis"]["ms"])
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
