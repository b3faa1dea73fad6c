#!/usr/bin/env python
"""One pk_gemm call per operand precision - exact fp32 (prec 0), bf16x3 (2), plain bf16 (1) - on three products the
parity mode runs: the k-major x k-major weight gradient of a 550-unit bidirectional layer (1100 x 1104 over K = 64 000,
split as functional._splitk splits it), a projection (64 000 x 1650 x 550) and an MLP layer at its batch (128 x 1024 x
1024).  Device events around `--inner` back-to-back calls, the precisions taken in turn inside every repeat, median over
`--reps` repeats after a warm-up of every shape and precision.  Writes profiles/bf16x3_gemm.json (or --out)."""
import argparse
import datetime
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F_ = importlib.import_module("pytorch-kaldi_amd.functional")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16x3_gemm.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "timings need the GPU"

g = torch.Generator().manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731


def wgrad():
    M, N, K = 1100, 1104, 64000
    A, B, C = rnd(K, M), rnd(K, N), torch.empty(M, N, device="cuda")  # both operands k-major: dW = dY^T . X
    sk = F_._splitk(F_._tiles(M, N), K)
    return (M, N, K), "k-major x k-major, splitk %d" % sk, lambda p: F_.gemm(M, N, K, A, 1, M, B, N, 1, C, N, splitk=sk, prec=p)


def rows_times_weight(M, N, K):
    def make():
        X, W, C = rnd(M, K), rnd(N, K), torch.empty(M, N, device="cuda")  # y = x W^T: both contiguous along k
        return (M, N, K), "k-contiguous x k-contiguous", lambda p: F_.gemm(M, N, K, X, K, 1, W, 1, K, C, N, prec=p)
    return make


PRECS = ("fp32", "bf16x3", "bf16")
out = {"device": torch.cuda.get_device_name(0), "host": os.uname().nodename, "date": datetime.date.today().isoformat(),
       "load_average": os.getloadavg()[0], "protocol": "device events around %d calls, median of %d repeats, precisions "
       "in turn inside every repeat, one warm-up round" % (args.inner, args.reps), "shapes": []}
for make in (wgrad, rows_times_weight(64000, 1650, 550), rows_times_weight(128, 1024, 1024)):
    (M, N, K), layout, call = make()
    ms = {p: [] for p in PRECS}
    for rep in range(args.reps + 1):
        for p in PRECS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                call(p)
            e1.record()
            e1.synchronize()
            if rep > 0:  # (round 0 is the warm-up)
                ms[p].append(e0.elapsed_time(e1) / args.inner)
    row = {"M": M, "N": N, "K": K, "layout": layout}
    for p in PRECS:
        med = statistics.median(ms[p])
        row[p] = {"ms": round(med, 4), "tflops": round(2.0 * M * N * K / med / 1e9, 1),
                  "ms_min_max": [round(min(ms[p]), 4), round(max(ms[p]), 4)]}
    out["shapes"].append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
