"""Fermi-smeared occupations and their gradient chain (nabladft_amd/orbital_loss.py ``smeared_solution``, csrc/orbsmear.hip) beside the solve they follow and
beside the closed-shell chain of ``orbital_solution`` on the same batch: one process, HIP events, warm-up first, on the synthetic conformers of
scripts/bench_orbital_loss.py (kT = 0.01, n_elec = 2 n_occ):

  (a) the solve: one launch of nq_orb_solve for the whole batch;
  (b) nq_orb_fermi: the chemical potential, occupations, their derivatives and the entropy;
  (c) the smeared density forward: ``smeared_density(occ)``, one nq_orb_wgram launch over all orbitals;
  (d) the response chain for gH and gS: nq_orb_resp_project over all orbitals, nq_orb_smear_mo, nq_orb_smear_diag, nq_orb_smear_back, nq_orb_syr2k over all
      orbitals, each alone and all five as ``smeared_response`` runs them (with the allocation of their scratch arrays);
  (e) the closed-shell chain ``density_response`` (four launches over occupied x all) on the same batch;
  (f) the alternative on the device: the loss ``sum G o D`` through ``torch.linalg`` autograd (cholesky, two triangular solves, ``eigh``, Fermi occupations at
      the device's mu with one Newton step for its implicit gradient), grouped by size -- forward AND backward.

No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_smearing.py --molecules 32 --out profiles/orbital_smearing_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_smearing.py --molecules 512 --append --out profiles/orbital_smearing_step.json
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
from scripts.bench_orbitals import event_ms, problems  # noqa: E402


def leg_eigh(orb, H, S, G, mu, kT, warmup, repeat):
    """``sum G o D`` of the smeared density through torch.linalg autograd per size group -> (record, gH packed)."""
    import torch
    st = orb.state
    dev = st.coeff.device
    groups = {}
    for b, m in enumerate(st.m.tolist()):
        groups.setdefault(int(m), []).append(b)
    pp = st.pack_ptr_host
    index = [(m, len(bs), torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev), mu[torch.tensor(bs, device=dev)][:, None])
             for m, bs in groups.items()]
    occ_of = lambda x: 2.0 * torch.exp(-torch.nn.functional.softplus(x, threshold=700.0))

    def run():
        Hl = H.detach().clone().requires_grad_(True)
        total = 0.0
        for m, nb, blk, mu0 in index:
            Hs, Ss, Gs = Hl[blk].view(nb, m, m), S[blk].view(nb, m, m), G[blk].view(nb, m, m)
            L = torch.linalg.cholesky(Ss)
            X = torch.linalg.solve_triangular(L, Hs, upper=False)
            A = torch.linalg.solve_triangular(L, X.mT, upper=False).mT
            eps, Y = torch.linalg.eigh(0.5 * (A + A.mT))
            C = torch.linalg.solve_triangular(L.mT, Y, upper=True)
            x0 = ((eps - mu0) / kT).detach()
            F0 = occ_of((eps - mu0) / kT)
            slope = (4.0 * torch.sigmoid(x0) * torch.sigmoid(-x0)).sum(1, keepdim=True) / (2.0 * kT)
            mu1 = mu0 - (F0.sum(1, keepdim=True) - F0.sum(1, keepdim=True).detach()) / slope      # the value of mu0, the implicit gradient of mu
            occ = occ_of((eps - mu1) / kT)
            total = total + (Gs * ((C * occ[:, None, :]) @ C.mT)).sum()
        total.backward()
        return Hl.grad
    ms_, runs = event_ms(run, warmup, repeat)
    return dict(ms=ms_, runs=runs, groups=len(groups), regrouping="index gather / scatter, indices prebuilt", what="forward and backward"), run()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kT", type=float, default=0.01)
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_smearing_step.json"))
    args = ap.parse_args()
    import torch
    from nabladft_amd.orbitals import BatchedOrbitals
    assert torch.cuda.is_available(), "bench_orbital_smearing.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    probs = problems(ms)
    n_occ = closed_shell_counts(ms, ne)
    n_elec = [2.0 * n for n in n_occ]
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), n_occ_mean=float(np.mean(n_occ)), kT=args.kT,
               device=torch.cuda.get_device_name(0))
    w, r = args.warmup, args.repeat

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)

    orb = BatchedOrbitals(op, "cuda")
    leg("solve", lambda: orb.solve(H, S), launches=1)
    leg("fermi", lambda: orb.fermi(n_elec, args.kT), launches=1)
    fr = orb.fermi(n_elec, args.kT)
    orb.check()
    leg("smeared_density_forward", lambda: orb.smeared_density(fr.occ), launches=1)
    G = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).normal(size=int(H.numel()))).cuda()
    full = orb.full_layout()
    flops = 2.0 * sum(float(m) ** 3 for m in ms)                       # one m x m x m product
    T = orb.resp_project(G, full)
    A_H, A_S, wdiag = orb.smear_mo(T, fr)
    orb.smear_diag(A_H, A_S, wdiag, fr)
    Rt_H, Rt_S = orb.smear_back(A_H, A_S)
    chain = {}
    for name, fn, products in (("project", lambda: orb.resp_project(G, full), 1), ("mo", lambda: orb.smear_mo(T, fr), 1),
                               ("diag", lambda: orb.smear_diag(A_H, A_S, wdiag, fr), 0), ("back", lambda: orb.smear_back(A_H, A_S), 2),
                               ("syr2k", lambda: orb.syr2k(Rt_H, Rt_S, full), 2)):
        t, runs = event_ms(fn, w, r)
        chain[name] = dict(ms=t, runs=runs, useful_tflops=products * flops / (t * 1e-3) / 1e12)
    t, runs = event_ms(lambda: orb.smeared_response(G, fr), w, r)
    chain["total"] = dict(ms=t, runs=runs, launches=6, useful_tflops=6.0 * flops / (t * 1e-3) / 1e12)
    t, runs = event_ms(lambda: orb.smeared_response(G, fr, overlap=False), w, r)
    chain["total_without_overlap_gradient"] = dict(ms=t, runs=runs, launches=6)
    rec["smeared_response_chain"] = chain
    print(json.dumps(dict(leg="smeared_response_chain", **chain)), flush=True)
    lay = orb.occupied_layout(n_occ)
    leg("closed_shell_chain", lambda: orb.density_response(G, lay), launches=5)
    leg("closed_shell_chain_without_overlap_gradient", lambda: orb.density_response(G, lay, False), launches=5)
    rec["torch_eigh_autograd"], eH = leg_eigh(orb, H, S, G, fr.mu, args.kT, w, r)
    kH = orb.smeared_response(G, fr, overlap=False)[0]
    rec["torch_eigh_autograd"]["max_difference_gH"] = float((kH - eH).abs().max())
    rec["torch_eigh_autograd"]["max_abs_gH"] = float(kH.abs().max())
    print(json.dumps(dict(leg="torch_eigh_autograd", **rec["torch_eigh_autograd"])), flush=True)
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
