"""Time functional.quat_linear against the route the engine offered before it for the same layer.

    python tools/time_quat_linear.py [--out profiles/quat_linear.json] [--reps 30]

fused      functional.quat_linear: pk_quat_linear_fwd; backward pk_quat_linear_bwd_x + pk_quat_linear_bwd_w (its two launches),
           once per kernel family, forced with pk_quat_linear_set_variant: fused_v0 (32 * RT-row tiles), fused_v1 (128-row streamed)
assembled  functional.quat_matrix + functional.linear: assemble, GEMM; backward GEMM (dX), GEMM (dW), fold, bias column sum

All on the same seeded inputs, in = out = 1024 (components 256 x 256) with bias, N = 128, 2 048, 16 000 and 64 000 rows,
fp32 and bf16 mode.  Every (shape, mode, route, pass) is warmed up, then timed with device events around `inner` calls,
`reps` times, the three routes alternating; the median and the quartiles of the per-call time are kept, and what the rule
of pk_quat_linear_variant picks for the shape is recorded next to them.  The result goes under `cases_variants` of the
output file; whatever else that file holds (the earlier rows of variant 0 alone) is kept.  Launches are counted with
torch's profiler in a run of their own (one call per route and pass).  Weight bytes are computed from the shapes: what
each route reads and writes of weights and weight gradients in HBM per step (components, the assembled matrix and its
gradient, the row-split workspace), activations excluded.  Needs a GPU; outputs of the two routes are compared first.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")


def fused(variant):
    def fn(x, comps, bias):
        return F_.quat_linear(x, *comps, bias)
    fn.variant = variant
    return fn


def assembled(x, comps, bias):
    I, O = comps[0].shape
    return F_.linear(x, F_.quat_matrix(comps, 1, I, O), bias)


def step(fn, x, comps, bias, cot, backward):
    lib = _lib.load()
    lib.pk_quat_linear_set_variant(getattr(fn, "variant", -1))
    try:
        y = fn(x, comps, bias)
        if backward:
            torch.autograd.grad(y, [x] + comps + [bias], cot)
    finally:
        lib.pk_quat_linear_set_variant(-1)
    return y


def timed(fn, args, backward, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        step(fn, *args, backward)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # microseconds per call


def launches(fn, args, backward):
    from torch.profiler import ProfilerActivity, profile

    step(fn, *args, backward)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(fn, *args, backward)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name
               and "emset" not in e.name)


def weight_bytes(N, I, O, backward):
    comp, dense = 4 * I * O * 4, 16 * I * O * 4
    ws = int(_lib.load().pk_quat_linear_work_floats(N, I, O)) * 4
    f = {"fused_v0": comp, "assembled": comp + dense + dense}  # read comps | read comps, write W, GEMM reads W
    if backward:
        f["fused_v0"] += comp + 2 * ws + comp           # dX reads comps; workspace written and read; dcomp written
        f["assembled"] += dense + dense + dense + comp  # dX reads W; dW written; fold reads dW, writes dcomp
    f["fused_v1"] = f["fused_v0"]                       # the same slices and workspace
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quat_linear.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--rows", type=int, nargs="+", default=[128, 2048, 16000, 64000])
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "time_quat_linear.py measures on the GPU; there is nothing to time without one"
    I = O = opt.features // 4
    out = {"device": torch.cuda.get_device_name(0), "in": 4 * I, "out": 4 * O, "reps": opt.reps, "unit": "microseconds per call",
           "note": "both kernel families forced in one process next to the assembled route (fused_v0: 32*RT-row tiles, "
                   "fused_v1: 128-row streamed); rule_fwd_dx_dcomp: what pk_quat_linear_variant picks unforced", "rows": []}
    for N in opt.rows:
        g = torch.Generator().manual_seed(N)
        comps = [(torch.randn(I, O, generator=g) / (2 * I) ** 0.5).cuda().requires_grad_(True) for _ in range(4)]
        x = torch.randn(N, 4 * I, generator=g).cuda().requires_grad_(True)
        bias, cot = torch.randn(4 * O, generator=g).cuda().requires_grad_(True), torch.randn(N, 4 * O, generator=g).cuda()
        args = (x, comps, bias, cot)
        inner = 50 if N <= 1024 else 5
        for prec in ("fp32", "bf16"):
            F_.set_precision(prec)
            yb = step(assembled, *args, False)
            diff = max(float((step(fused(v), *args, False) - yb).norm() / yb.norm()) for v in (0, 1))
            assert diff < (2e-2 if prec == "bf16" else 1e-5), (N, prec, diff)
            rule = [int(_lib.load().pk_quat_linear_variant(p, 1 if prec == "bf16" else 0, N, I, O)) for p in range(3)]
            for backward in (False, True):
                routes = {"fused_v0": fused(0), "fused_v1": fused(1), "assembled": assembled}
                for fn in routes.values():
                    for _ in range(3):
                        timed(fn, args, backward, inner)
                t = {k: [] for k in routes}
                for _ in range(opt.reps):
                    for k, fn in routes.items():
                        t[k].append(timed(fn, args, backward, inner))
                case = {"N": N, "prec": prec, "pass": "forward+backward" if backward else "forward", "routes_rel_diff": diff,
                        "rule_fwd_dx_dcomp": rule,
                        "weight_bytes": weight_bytes(N, I, O, backward)}
                for k, fn in routes.items():
                    q = statistics.quantiles(t[k], n=4)
                    case[k] = {"median": round(q[1], 2), "q1": round(q[0], 2), "q3": round(q[2], 2), "launches": launches(fn, args, backward)}
                case["v0_over_v1"] = round(case["fused_v0"]["median"] / case["fused_v1"]["median"], 3)
                case["assembled_over_v1"] = round(case["assembled"]["median"] / case["fused_v1"]["median"], 3)
                print(json.dumps(case), flush=True)
                out["rows"].append(case)
        F_.set_precision("fp32")
    # everything the file holds stays (`cases`: the run of variant 0 alone, before there were two); this run replaces
    # `cases_variants`
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    whole = json.load(open(opt.out)) if os.path.exists(opt.out) else {}
    whole["cases_variants"] = out
    with open(opt.out, "w") as f:
        json.dump(whole, f, indent=1)
        f.write("\n")
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
