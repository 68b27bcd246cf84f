"""Operator timings behind the GemNet-OC "bf16_act" mode on one MI355X: the ScaledSiLU products with fp32 / bf16 operands and outputs in HBM, the SiLU reverse
with an fp32 / bf16 pre-activation, and the weight gradient that reads a bf16 activation against the fp32 split-K kernel below the 2048-row threshold of the
"bf16" mode.  Device events around `iters` back-to-back launches, `rounds` rounds with the flavours taking turns; per flavour the median round and the spread
(max - min) in microseconds per launch, and the compulsory bytes over that time.

    python scripts/bench_dense_bf16_act.py [--rows 20468,81872] [--units 512] [--iters 50] [--rounds 3]

NABLAQ_LIB selects a development build of the library (store-width / occupancy variants of the epilogue)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per launch


def _rounds(cases, iters, rounds):
    """cases: {name: (fn, compulsory bytes)} -> {name: {us, spread_us, GBs}} with the cases taking turns in every round."""
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (fn, _) in cases.items():
            t[k].append(_time(fn, iters))
    out = {}
    for k, v in t.items():
        s = sorted(v)
        med = s[len(s) // 2]
        out[k] = {"us": round(med, 2), "spread_us": round(s[-1] - s[0], 2), "GBs": round(cases[k][1] / med / 1e3, 1)}
    return out


def main():
    import torch
    from nabladft_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="20468,81872")              # main-graph edge rows of 16 and 64 synthetic conformers at the yaml configuration
    ap.add_argument("--units", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--wgrad-rows", default="256,512,1024,2047")
    a = ap.parse_args()
    lib, dev, st = _lib.load(), torch.device("cuda:0"), _lib.stream_ptr
    BF, P = torch.bfloat16, _lib.ptr
    U = a.units
    g = torch.Generator(device="cpu").manual_seed(0)
    W = torch.randn(U, U, generator=g).mul(U ** -0.5).to(dev)
    Wb, WbT = torch.empty(U, U, device=dev, dtype=BF), torch.empty(U, U, device=dev, dtype=BF)
    _lib.check(lib.nq_bf16_pack(P(W), U, U, P(Wb), P(WbT), st()))
    res = {"lib": os.environ.get("NABLAQ_LIB", "libnablaq.so"), "units": U, "iters": a.iters, "rounds": a.rounds, "forward": {}, "ssilu_bwd": {}, "wgrad": {}}
    for M in (int(v) for v in a.rows.split(",")):
        x = torch.randn(M, U, generator=g).to(dev)
        xb = x.to(BF)
        pre, act = torch.empty(M, U, device=dev), torch.empty(M, U, device=dev)
        preb, actb = torch.empty(M, U, device=dev, dtype=BF), torch.empty(M, U, device=dev, dtype=BF)
        MU, WB = M * U, 2 * U * U

        def f32(r=None):
            _lib.check(lib.nq_linear_forward_bf16(P(x), P(Wb), P(pre), P(act), r, 0.7, 1.2, M, U, U, st()))

        def out(A, a_bf, O, o_bf, r=None):
            _lib.check(lib.nq_linear_forward_bf16_out(P(A), a_bf, P(Wb), P(preb), P(O), o_bf, r, 0.7, 1.2, M, U, U, st()))

        res["forward"][M] = _rounds({
            "f32 A -> f32 pre, f32 act            (bf16 mode, first product)": (lambda: f32(), 12 * MU + WB),
            "f32 A -> f32 pre, f32 act + resid    (bf16 mode, second product)": (lambda: f32(P(x)), 16 * MU + WB),
            "f32 A -> bf16 pre, bf16 act          (bf16_act, first product)": (lambda: out(x, 0, actb, 1), 8 * MU + WB),
            "bf16 A -> bf16 pre, f32 act + resid  (bf16_act, second product)": (lambda: out(xb, 1, act, 0, P(x)), 12 * MU + WB),
            "f32 A -> bf16 pre, f32 act           (bf16_act, activated Dense)": (lambda: out(x, 0, act, 0), 10 * MU + WB)}, a.iters, a.rounds)
        z, gy, o = torch.randn(M, U, generator=g).to(dev), torch.randn(M, U, generator=g).to(dev), torch.empty(M, U, device=dev)
        zb = z.to(BF)
        res["ssilu_bwd"][M] = _rounds({
            "f32 z": (lambda: _lib.check(lib.nq_gn_ssilu_backward(P(z), P(gy), 0.7, MU, P(o), st())), 12 * MU),
            "bf16 z": (lambda: _lib.check(lib.nq_gn_ssilu_backward_bf16(P(zb), P(gy), 0.7, MU, P(o), st())), 10 * MU)}, a.iters, a.rounds)
    for M in (int(v) for v in a.wgrad_rows.split(",")):
        gy, x = torch.randn(M, U, generator=g).to(dev), torch.randn(M, U, generator=g).to(dev)
        xb = x.to(BF)
        gW = torch.empty(U, U, device=dev)
        s32 = torch.empty(int(lib.nq_weight_grad_scratch_floats(M, U, U)) + 64, device=dev)
        s16 = torch.empty(int(lib.nq_weight_grad_bf16_scratch_bytes(M, U, U)), device=dev, dtype=torch.uint8)
        res["wgrad"][M] = _rounds({
            "f32 kernel, f32 X (bf16 mode below 2048 rows)": (lambda: _lib.check(lib.nq_linear_weight_grad(P(gy), P(x), P(gW), M, U, U, P(s32), st())), 8 * M * U + 4 * U * U),
            "bf16 kernel, bf16 X (bf16_act)": (lambda: _lib.check(lib.nq_linear_weight_grad_bf16_x(P(gy), P(xb), P(gW), M, U, U, P(s16), st())), 6 * M * U + 4 * U * U)},
            a.iters, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
