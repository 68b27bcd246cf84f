"""The eigensolver-free density route (csrc/orbpurify.hip, ``BatchedPurification``, ``purified_density_matrix``) beside the solver route it replaces, one
process, HIP events, warm-up first, on the sizes of the synthetic conformers of scripts/bench_orbital_loss.py.  The matrices are
``orbital_density_ref.gapped_case`` problems (HOMO-LUMO gap 0.3 in a 22-unit spectrum, kappa_2(S) about 1e2): purification needs an open gap, which
``orbitals_ref.case`` leaves to chance; every leg, the solver's and torch's included, runs on the same matrices.

  (a) the orthogonaliser: one launch of nq_orb_pur_orthogonalizer (Cholesky + triangular inverse, one workgroup per molecule);
  (b) the congruence Ht = Z H Z^T: two triangular products (nq_orb_pur_congruence);
  (c) the SP2 loop: nq_orb_pur_init + nq_orb_pur_run with max_iter = 100 (two launches per iteration, finished molecules exit at once), with the
      iterations per molecule, and the product kernel's useful rate (2 m^3 flop per molecule and iteration actually run);
  (d) the back-transform D = 2 Z^T X Z;
  (e) the response loop with and without the S half (``response``: the congruence of G, nq_orb_pur_response_init / _run, the back-transforms, and for S
      four general products), with the useful rate of the loop's product kernel (6 m^3 flop per molecule and iteration: X X, X1 X and X X1);
  (f) forward + backward of ``sum G o D`` through ``purified_density_matrix`` (orthogonaliser included) and through ``orbital_solution`` (solve + density
      + response chain) in the same run, and the ``torch.linalg`` autograd route of scripts/bench_orbital_density.py;
  With --model: the QHNet training step (config/qhnet.yaml sizes, 16 conformers) with a density term through ``QHNetDensityLightning``'s route and through
  ``QHNetPurifiedDensityLightning``'s (one orthogonaliser for prediction and target).

No figure here is a gate.  Run each invocation under its own time limit:

    timeout -k 10 600 python scripts/bench_orbital_purify.py --molecules 32 --model --out profiles/orbital_purify_step.json && \\
    timeout -k 10 600 python scripts/bench_orbital_purify.py --molecules 512 --append --out profiles/orbital_purify_step.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scripts.bench_orbital_density import leg_eigh  # noqa: E402
from scripts.bench_orbital_loss import closed_shell_counts, conformers  # noqa: E402
from scripts.bench_orbitals import event_ms  # noqa: E402


def gapped_problems(ms, n_occ, gap=0.3, seed=300):
    """One ``gapped_case`` per distinct (m, n_occ), shifted per molecule (H + c S moves every level by c: another problem of the same cost and gap)."""
    import orbital_density_ref as DR
    cache, out = {}, []
    for b, (m, n) in enumerate(zip(ms, n_occ)):
        if (m, n) not in cache:
            cache[(m, n)] = DR.gapped_case(m, n, gap, 1e2, seed + m)
        H, S = cache[(m, n)]
        out.append((H + 0.01 * (b % 17) * S, S))
    return out


def leg_model(warmup, repeat, molecules=16):
    """The QHNet training step with a density term through the solver and through purification, on device-resident targets and overlaps.  An untrained
    network's prediction has no HOMO-LUMO gap to speak of, so both routes take their density of ``H_gap + c p``: the ``gapped_case`` matrices of the batch's
    sizes plus the prediction p scaled so that it moves no level by more than 0.05 (c max|p| max m = 0.05).  The gradient still flows to every parameter, the
    cost does not depend on c, and both routes see the same matrices; the iterations are reported."""
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
    l_h, l_d = HamiltonianLoss(), nq.DensityMatrixLoss("mae")
    seen = {}

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
            D_p, pur_p = nq.purified_density_matrix(H_gap + c * p.double(), S, op, n_occ, orth, return_solution=True)
            loss = loss + 0.1 * l_d(D_p, D_t, op)
            seen["pur"] = (pur_p, pur_t)
        loss.backward()
        opt.step()
    out = dict(molecules=molecules, m_mean=float(np.mean(ms)))
    for route in ("plain", "solver", "purify"):
        t, runs = event_ms(lambda: step(route), warmup, repeat)
        out[f"step_{route}_ms"], out[f"step_{route}_runs"] = t, runs
    for name, pur in zip(("prediction", "target"), seen["pur"]):
        it, st = pur.iterations.cpu().numpy(), pur.status.cpu().numpy()
        out[f"{name}_iterations"] = dict(min=int(it.min()), mean=float(it.mean()), max=int(it.max()), not_converged=int((st == 4).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--model", action="store_true", help="also time the QHNet training step at 16 conformers with the density term through both routes")
    ap.add_argument("--append", action="store_true", help="add this record to the list already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbital_purify_step.json"))
    args = ap.parse_args()
    import torch
    import nabladft_amd as nq
    from nabladft_amd.orbitals import BatchedOrbitals, BatchedPurification
    assert torch.cuda.is_available(), "bench_orbital_purify.py needs the MI355X"
    ms, atoms, per_atom, ne = conformers(args.molecules)
    n_occ = closed_shell_counts(ms, ne)
    probs = gapped_problems(ms, n_occ)
    op = np.concatenate([[0], np.cumsum(ms)])
    H = torch.from_numpy(np.concatenate([p[0].ravel() for p in probs])).cuda()
    S = torch.from_numpy(np.concatenate([p[1].ravel() for p in probs])).cuda()
    G = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).normal(size=int(H.numel()))).cuda()
    rec = dict(molecules=args.molecules, m_min=min(ms), m_max=max(ms), m_mean=float(np.mean(ms)), n_occ_mean=float(np.mean(n_occ)), gap=0.3,
               device=torch.cuda.get_device_name(0))
    w, r = args.warmup, args.repeat
    cube = np.array([float(m) ** 3 for m in ms])

    def leg(name, fn, **more):
        t, runs = event_ms(fn, w, r)
        rec[name] = dict(ms=t, runs=runs, **{k: (v(t) if callable(v) else v) for k, v in more.items()})
        print(json.dumps(dict(leg=name, **rec[name])), flush=True)

    rate = lambda flop: (lambda t: flop / (t * 1e-3) / 1e12)
    pur = BatchedPurification(op, "cuda")
    leg("orthogonalizer", lambda: pur.orthogonalize(S), launches=1)
    orth = pur.orthogonalizer
    st = pur.state
    # two triangular products: about m^3 / 3 multiply-adds useful in the first (k <= j), m^3 / 6 in the second (k <= i, j <= i)
    leg("congruence", lambda: pur.congruence(orth.Z, H, False, out=st.work), launches=3, useful_tflops=rate(2.0 * cube.sum() * (1.0 / 2.0 + 1.0 / 6.0)))
    leg("sp2_loop", lambda: pur.purify(H, n_occ, 100, orth), launches=3 + 1 + 201)
    pur.check()
    it = pur.iterations.cpu().numpy().astype(np.float64)
    # the loop's share: the leg minus the congruence it starts with; it holds the init and the elementwise updates beside the products (one more product than updates)
    rec["sp2_loop"].update(iterations=dict(min=int(it.min()), mean=float(it.mean()), max=int(it.max())),
                           useful_tflops_products=2.0 * float((cube * (it + 1.0)).sum()) / ((rec["sp2_loop"]["ms"] - rec["congruence"]["ms"]) * 1e-3) / 1e12)
    leg("back_transform", lambda: pur.density(), launches=3, useful_tflops=rate(2.0 * cube.sum() * (1.0 / 2.0 + 1.0 / 6.0)))
    leg("response", lambda: pur.response(G, True), useful_tflops_products=rate(6.0 * float((cube * it).sum())))
    leg("response_without_overlap_gradient", lambda: pur.response(G, False), useful_tflops_products=rate(6.0 * float((cube * it).sum())))

    def route(purified):
        Hl, Sl = H.detach().clone().requires_grad_(True), S.detach().clone().requires_grad_(True)
        D = nq.purified_density_matrix(Hl, Sl, op, n_occ) if purified else nq.density_matrix(Hl, Sl, op, n_occ)
        (G * D).sum().backward()
        return Hl.grad, Sl.grad
    leg("purified_forward_backward", lambda: route(True))
    leg("orbital_solution_forward_backward", lambda: route(False))
    a, b = route(True), route(False)
    rec["agreement"] = dict(max_difference_gH=float((a[0] - b[0]).abs().max()), max_abs_gH=float(b[0].abs().max()),
                            max_difference_gS=float((a[1] - b[1]).abs().max()), max_abs_gS=float(b[1].abs().max()))
    rec["ratio_solver_over_purified"] = rec["orbital_solution_forward_backward"]["ms"] / rec["purified_forward_backward"]["ms"]
    orb = BatchedOrbitals(op, "cuda").solve(H, S)
    rec["torch_eigh_autograd"], _ = leg_eigh(orb, H, S, G, n_occ, w, r)
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
