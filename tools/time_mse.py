"""Time functional.mse_cost (pk_mse.hip), forward and forward + backward (both operands want a gradient only where the
recipe's do: the first, a module output), against

  * the stock expression of the reference, torch.mean((a - b) ** 2), and its autograd;
  * torch's device copy of the bytes the forward must read (a and b once: a copy of a buffer of half that size), same run;

at the two recipe shapes:

  autoencoder  TIMIT_MLP_fbank_autoencoder: 128 frames of 440 values against the 440-column feature slice of a 441-wide chunk
  joint        TIMIT_joint_training_liGRU_fbank: 64 000 frames of 40 values against a 40-column slice of an 82-wide chunk

    python tools/time_mse.py [--json profiles/mse_cost.json]

Needs a GPU.  Device events around `--inner` back-to-back calls, per-call time = window / inner; median, minimum and maximum
of `--reps` windows after a warm-up window.  The routes alternate inside every repetition.  Calls this short are bound by
the host's enqueue cost, so every route is timed a second time as a captured HIP graph of the same `--inner` calls
(`*_replayed_ms`): what the device spends on them once the host is out of the way."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
SHAPES = {"autoencoder": (128, 440, 441, 0), "joint": (64000, 40, 82, 0)}  # rows, F, chunk width, first column


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def replay_ms(fn, inner, reps):
    """The same `inner` calls captured once into a HIP graph and replayed: device time without the host's enqueue cost"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    graph.replay()
    t = [window_ms(graph.replay, 1) / inner for _ in range(reps)]
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def stock(a, b):
    return torch.mean((a - b) ** 2)


def point(rows, F, width, first, reps, inner):
    a = torch.randn(rows, F, device="cuda", requires_grad=True)
    b = torch.randn(rows, width, device="cuda")[:, first:first + F]
    moved = 2 * rows * F * 4
    src = torch.empty(moved // 8, device="cuda")
    dst = torch.empty_like(src)

    def train(cost):
        a.grad = None
        cost(a, b).backward()

    routes = {"copy": lambda: dst.copy_(src),
              "fused_fwd": lambda: F_.mse_cost(a.detach(), b), "fused_fwd_bwd": lambda: train(F_.mse_cost),
              "stock_fwd": lambda: stock(a.detach(), b), "stock_fwd_bwd": lambda: train(stock)}
    train(F_.mse_cost)
    g_fused = a.grad.clone()
    train(stock)
    r = {"rows": rows, "F": F, "chunk_width": width, "first_column": first, "bytes_read": moved,
         "loss_fused": float(F_.mse_cost(a.detach(), b)), "loss_stock": float(stock(a.detach(), b)),
         "grad_max_abs_diff": float((g_fused - a.grad).abs().max())}
    times = {k: [] for k in routes}
    for fn in routes.values():
        window_ms(fn, inner)
    for _ in range(reps):
        for k, fn in routes.items():
            times[k].append(window_ms(fn, inner))
    for k, t in times.items():
        r[k + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    for k, fn in routes.items():
        r[k + "_replayed_ms"] = replay_ms(fn, inner, reps)
    r["stock_over_fused_fwd_replayed"] = r["stock_fwd_replayed_ms"]["median"] / r["fused_fwd_replayed_ms"]["median"]
    r["stock_over_fused_fwd_bwd_replayed"] = r["stock_fwd_bwd_replayed_ms"]["median"] / r["fused_fwd_bwd_replayed_ms"]["median"]
    r["copy_GBps"] = 2 * src.numel() * 4 / r["copy_ms"]["median"] * 1e-6
    r["fused_fwd_fraction_of_copy_rate"] = r["copy_ms"]["median"] / r["fused_fwd_ms"]["median"]
    r["stock_over_fused_fwd"] = r["stock_fwd_ms"]["median"] / r["fused_fwd_ms"]["median"]
    r["stock_over_fused_fwd_bwd"] = r["stock_fwd_bwd_ms"]["median"] / r["fused_fwd_bwd_ms"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_mse.py measures on the GPU"
    torch.manual_seed(0)
    out = {"reps": a.reps, "inner": a.inner}
    for name, shape in SHAPES.items():
        out[name] = point(*shape, a.reps, a.inner)
        print(name, json.dumps(out[name]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
