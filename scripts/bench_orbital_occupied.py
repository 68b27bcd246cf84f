"""All occupied levels without a full solve (``BatchedPurification.occupied``, csrc/orbocc.hip) leg by leg, against the solver route and ``torch.linalg`` IN THE
SAME RUN, one process, HIP events, warm-up first, on the synthetic conformers of scripts/bench_orbital_loss.py with the gapped matrices of
scripts/bench_orbital_purify.py:

  (a) the purification the levels follow: orthogonaliser, then congruence + bounds + SP2 loop (``purify``);
  (b) the four stages, each alone: ``nq_orb_occ_factor``; ``nq_orb_resp_project`` + ``nq_orb_occ_reduce``; ``nq_orb_solve`` on the reduced blocks;
      ``nq_orb_occ_back``; and ``occupied()`` as a whole (which also prepares its two states);
  (c) the whole route from ``(H, S)`` for prediction and target with ``compare``, beside ``BatchedOrbitals.solve`` twice + ``compare``;
  (d) ``torch.linalg.cholesky`` / ``solve_triangular`` / ``eigh`` on dense blocks grouped by size, the regrouping by prebuilt index gather;
  (e) the backward launch (``nq_orb_wgram`` over k < n_occ: gH and gS).

  With --model: the QHNet training step (config/qhnet.yaml sizes, 16 conformers) with an occupied-energy term through this route and through
  ``QHNetOrbitalLightning``'s way (``orbital_energies`` + ``OrbitalEnergyLoss("mae", "occupied")``), set up as in scripts/bench_orbital_purify.py.

No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_occupied.py --molecules 32 --model --out profiles/orbital_occupied_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_occupied.py --molecules 512 --append --out profiles/orbital_occupied_step.json
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


def leg_eigh(st, H, S, n_occ, warmup, repeat):
    """The occupied levels through ``torch.linalg`` per size group (``eigh``: the vectors are part of the job) -> (record, eps [M] with NaN in the virtual slots)."""
    import torch
    dev = H.device
    groups = {}
    for b, m in enumerate(st.m.tolist()):
        groups.setdefault(int(m), []).append(b)
    pp, op = st.pack_ptr_host, st.orb_ptr_host
    index = [(m, torch.from_numpy(np.stack([np.arange(pp[b], pp[b + 1]) for b in bs])).to(dev), torch.from_numpy(np.stack([np.arange(op[b], op[b + 1]) for b in bs])).to(dev))
             for m, bs in groups.items()]

    def step():
        eps = torch.empty(st.M, dtype=torch.float64, device=dev)
        for m, blk, orb in index:
            nb = blk.shape[0]
            L = torch.linalg.cholesky(S[blk].view(nb, m, m))
            Y = torch.linalg.solve_triangular(L, H[blk].view(nb, m, m), upper=False)
            A = torch.linalg.solve_triangular(L, Y.mT, upper=False)
            e, V = torch.linalg.eigh(0.5 * (A + A.mT))
            C = torch.linalg.solve_triangular(L.mT, V, upper=True)      # the coefficients, as the other routes deliver them
            eps[orb] = e + 0.0 * C[:, 0, :]
        return eps
    t, runs = event_ms(step, warmup, repeat)
    return dict(ms=t, runs=runs, groups=len(groups), what="torch.linalg cholesky, two solve_triangular, eigh, back substitution per size group",
                regrouping="index gather, indices prebuilt"), step()


def leg_model(warmup, repeat, molecules=16):
    """The QHNet training step with an occupied-energy term through the purification + Cholesky-factor route and through the solver; the set-up of
    scripts/bench_orbital_purify.py (an untrained network's prediction has no gap to speak of: both routes take their levels of ``H_gap + c p``)."""
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
    l_h, l_o, l_e, l_d = HamiltonianLoss(), nq.OccupiedEnergyLoss("mae"), nq.OrbitalEnergyLoss("mae", "occupied"), nq.DensityMatrixLoss("mae")
    seen = {}

    def step(route):
        opt.zero_grad(set_to_none=True)
        p = net(b, packed=True)
        loss = l_h(p, target)
        Hp = H_gap + c * p.double()
        if route == "solver":
            eps_t = nq.BatchedOrbitals(op, "cuda").solve(H_t, S).energies
            loss = loss + 0.1 * l_e(nq.orbital_energies(Hp, S, op), eps_t, n_occ, op)
        elif route in ("occupied", "occupied_and_density"):
            pur_t = nq.BatchedPurification(op, "cuda")
            orth = pur_t.orthogonalize(S)
            occ_t = pur_t.purify(H_t, n_occ, 100, orth).occupied()
            sol = None
            if route == "occupied_and_density":
                D_p, sol = nq.purified_density_matrix(Hp, S, op, n_occ, orth, return_solution=True)
                loss = loss + 0.1 * l_d(D_p, pur_t.density(), op)
            eps, sol = nq.purified_occupied_energies(Hp, S, op, n_occ, orth, solution=sol, return_solution=True)
            loss = loss + 0.1 * l_o(eps, occ_t.energies, n_occ, op)
            seen["status"] = (sol.occupied_orbitals.status, occ_t.status)
        loss.backward()
        opt.step()
    out = dict(molecules=molecules, m_mean=float(np.mean(ms)), n_occ_mean=float(np.mean(n_occ)))
    for route in ("plain", "solver", "occupied", "occupied_and_density"):
        t, runs = event_ms(lambda: step(route), warmup, repeat)
        out[f"step_{route}_ms"], out[f"step_{route}_runs"] = t, runs
    out["all_status_zero"] = bool(all(int(s.abs().max()) == 0 for s in seen["status"]))
    out["occupied_over_solver"] = out["step_occupied_ms"] / out["step_solver_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--model", action="store_true", help="also time the QHNet training step at 16 conformers with an occupied-energy term by both routes")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_occupied_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    from nabladft_amd import _lib
    from nabladft_amd.orbitals import OrbitalState
    assert torch.cuda.is_available(), "bench_orbital_occupied.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    n_occ = closed_shell_counts(ms, ne)
    probs = gapped_problems(ms, n_occ)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    H2 = H + 1e-4 * torch.randn(H.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).cuda()      # the "prediction" of the comparison legs
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), n_occ_mean=float(np.mean(n_occ)), n_occ_max=int(np.max(n_occ)),
               device=torch.cuda.get_device_name(0))
    w, r = args.warmup, args.repeat

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **more)
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)
        return t

    pur = nq.BatchedPurification(op, "cuda")
    leg("orthogonalizer", lambda: pur.orthogonalize(S), launches=1)
    orth = pur.orthogonalize(S)
    leg("purify", lambda: pur.purify(H, n_occ, 100, orth), what="congruence, bounds and the SP2 loop")
    pur.purify(H, n_occ, 100, orth).check()
    rec["purify"]["sp2_iterations_mean"] = float(pur.iterations.float().mean())
    occ = pur.occupied().check()
    rec["factor_min_pivot_times_m"] = float((occ.min_pivot * torch.from_numpy(np.asarray(ms, dtype=np.float64)).cuda()).min())
    rec["factor_defect_max"] = float(occ.defect.max())
    # the stages alone, on the buffers of one occupied() call
    ps, st, red = pur.state, occ.state, occ.reduced
    no, optr, O = occ._layout
    f64 = torch.float64
    Q = torch.empty(ps.P, dtype=f64, device="cuda")
    piv = torch.empty(ps.M, dtype=torch.int32, device="cuda")
    minp, defect = torch.empty(ps.B, dtype=f64, device="cuda"), torch.empty(ps.B, dtype=f64, device="cuda")
    stat = torch.zeros(ps.B, dtype=torch.int32, device="cuda")
    t_fac = leg("factor", lambda: ps.call("nq_orb_occ_factor", _lib.ptr(no), _lib.ptr(Q), _lib.ptr(piv), _lib.ptr(minp), _lib.ptr(defect), _lib.ptr(stat)), launches=1,
                what="nq_orb_occ_factor: one workgroup per molecule, n_occ steps")
    st.coeff.copy_(Q)                                                # Q again: the back-transform of occupied() has overwritten it
    Gs, T = torch.empty(ps.P, dtype=f64, device="cuda"), torch.empty(O, dtype=f64, device="cuda")
    Hs = torch.empty(red.P, dtype=f64, device="cuda")

    def reduce():
        st.call("nq_orb_resp_project", _lib.ptr(no), _lib.ptr(optr), O, _lib.ptr(ps.work), _lib.ptr(Gs), _lib.ptr(T))
        st.call("nq_orb_occ_reduce", _lib.ptr(no), _lib.ptr(optr), O, _lib.ptr(T), _lib.ptr(stat), _lib.ptr(red.pack_ptr), red.P, _lib.ptr(Hs))
    t_red = leg("reduce", reduce, launches=3, what="nq_orb_resp_project (symmetrise, Ht Q^T) + nq_orb_occ_reduce (Q T)")
    t_sol = leg("reduced_solve", lambda: red.solve(Hs), launches=1, what="nq_orb_solve on the n_occ x n_occ blocks: one workgroup per molecule")
    W = orth.Z
    U = torch.empty(O, dtype=f64, device="cuda")

    def back():
        st.coeff.copy_(Q)
        with torch.cuda.device("cuda"):
            _lib.check(_lib.load().nq_orb_occ_back(_lib.ptr(st.buf), _lib.ptr(red.buf), *st._dims, red.M, red.P, _lib.ptr(no), _lib.ptr(optr), O, _lib.ptr(W), _lib.ptr(stat),
                                                   _lib.ptr(U), _lib.stream_ptr()))
    t_copy = leg("copy_of_q", lambda: st.coeff.copy_(Q), what="the device copy inside the `back` leg, to subtract")
    t_back = leg("back", back, launches=3, what="nq_orb_occ_back (V Q, U W, sign rule and NaN rows), with the copy of Q in front")
    rec["back"]["ms_without_copy"] = t_back - t_copy
    t_occ = leg("occupied", lambda: pur.occupied(), what="occupied(): two state preparations, the four stages")
    rec["stages_sum_ms"] = t_fac + t_red + t_sol + t_back - t_copy
    rec["reduced_solve_share_of_stages"] = t_sol / rec["stages_sum_ms"]
    g = torch.ones(ps.M, dtype=f64, device="cuda")
    leg("gradients", lambda: occ.weighted_gram(g, -(occ.energies * g)), launches=1, what="nq_orb_wgram over k < n_occ: gH and gS")
    # the whole route for two Hamiltonians and the figures, beside the solver's
    pur2 = nq.BatchedPurification(op, "cuda")

    def route():
        o = pur.orthogonalize(S)
        a = pur.purify(H, n_occ, 100, o).occupied()
        b = pur2.purify(H2, n_occ, 100, o).occupied()
        return b.compare(a, S)
    t_route = leg("route_two_hamiltonians_and_compare", route, what="one orthogonaliser, two purifications, two occupied(), compare")
    orb, orb2 = nq.BatchedOrbitals(op, "cuda"), nq.BatchedOrbitals(op, "cuda")
    n_host = torch.from_numpy(np.asarray(n_occ, dtype=np.int32))
    t_solver = leg("solve_two_hamiltonians_and_compare", lambda: orb2.solve(H2, S).compare(orb.solve(H, S), n_host, S), what="BatchedOrbitals.solve twice + compare")
    rec["route_over_solver"] = t_route / t_solver
    figs, full = route().cpu().numpy(), orb2.solve(H2, S).compare(orb.solve(H, S), n_host, S).cpu().numpy()
    rows = [nq.orbitals.FIGURES.index(k) for k in ("eps_mae_occ", "psi_sim_occ", "psi_sim_min_occ", "homo_abs_err")]
    rec["against_solver"] = {k: float(np.abs(figs[i] - full[j]).max()) for i, (k, j) in enumerate(zip(nq.orbitals.OCCUPIED_FIGURES, rows))}
    t_one = leg("route_one_hamiltonian", lambda: pur.purify(H, n_occ, 100, pur.orthogonalize(S)).occupied(), what="the whole route from (H, S)")
    t_one_solver = leg("solve_one_hamiltonian", lambda: orb.solve(H, S), what="BatchedOrbitals.solve")
    rec["route_one_over_solver"] = t_one / t_one_solver
    rec["torch_eigh"], te = leg_eigh(ps, H, S, n_occ, w, r)
    eo = pur.purify(H, n_occ, 100, orth).occupied().energies
    sel = ~torch.isnan(eo)
    rec["torch_eigh"]["max_difference"] = float((eo[sel] - te[sel]).abs().max())
    print(json.dumps(dict(leg="torch_eigh", **rec["torch_eigh"])), flush=True)
    rec["route_one_over_torch_eigh"] = t_one / rec["torch_eigh"]["ms"]
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
