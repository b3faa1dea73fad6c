"""Time nn.SincConv_fast's kernels (pk_sincfast.hip), forward and forward + backward (parameter gradients only: the input of
a first layer is data), at the recipe's shape - 128 sentences of 3200 samples, 80 filters of 251 taps, stride = dilation = 1,
no padding - against

  * torch's device copy of the bytes the forward must move (x in, y out: a copy of a buffer of half that size), same run;
  * the engine's own UNFOLDED route for the same numbers: functional.conv1d_pool at pool 1 on a torch-built [C, 1, K] bank
    (the formula of tests/sincfast_ref.py on the device);
  * stock torch.nn.functional.conv1d on that bank;

and at one strided point (stride 160, 401 taps, padding 200) against stock conv1d only - the engine's convolution has no
stride.

    python tools/time_sincfast.py [--json profiles/sincfast.json]

Needs a GPU.  Device events around `--inner` back-to-back calls, per-call time = window / inner; median, minimum and maximum
of `--reps` windows after a warm-up window.  The routes alternate inside every repetition."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
B, N, C, SR = 128, 3200, 80, 16000


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def bank(net):
    low = net.min_low_hz + net.low_hz_.abs()
    high = torch.clamp(low + net.min_band_hz + net.band_hz_.abs(), net.min_low_hz, net.sample_rate / 2)
    band = high - low
    left = (torch.sin(high * net.n_) - torch.sin(low * net.n_)) / (net.n_ / 2) * net.window_ / (2 * band)
    return torch.cat([left, torch.ones_like(band), left.flip(1)], dim=1).unsqueeze(1)


def point(K, s, p, with_engine, reps, inner):
    net = nn_amd.SincConv_fast(1, C, K, stride=s, padding=p, sample_rate=SR).cuda()
    x = 0.3 * torch.randn(B, 1, N, device="cuda")
    y = net(x).detach()
    dy = torch.randn_like(y)
    zero_bias = torch.zeros(C, device="cuda")
    moved = (x.numel() + y.numel()) * 4
    src = torch.empty(moved // 8, device="cuda")
    dst = torch.empty_like(src)

    def train(fwd):
        net.low_hz_.grad = net.band_hz_.grad = None
        fwd().backward(dy)

    routes = {"copy": lambda: dst.copy_(src),
              "folded_fwd": lambda: net(x), "folded_fwd_bwd": lambda: train(lambda: net(x)),
              "stock_fwd": lambda: torch.nn.functional.conv1d(x, bank(net), stride=s, padding=p),
              "stock_fwd_bwd": lambda: train(lambda: torch.nn.functional.conv1d(x, bank(net), stride=s, padding=p))}
    r = {"K": K, "stride": s, "padding": p, "L_out": y.shape[2], "bytes_moved": moved, "fma_unfolded": y.numel() * K,
         "folded_vs_stock_max_abs_diff": float((y - routes["stock_fwd"]().detach()).abs().max())}
    if with_engine:
        routes["unfolded_fwd"] = lambda: F_.conv1d_pool(x, bank(net), zero_bias, 1)
        routes["unfolded_fwd_bwd"] = lambda: train(lambda: F_.conv1d_pool(x, bank(net), zero_bias, 1))
        with torch.no_grad():
            wb = bank(net)
            routes["unfolded_conv_only"] = lambda: F_.conv1d_pool(x, wb, zero_bias, 1)
            r["folded_vs_unfolded_max_abs_diff"] = float((y - routes["unfolded_conv_only"]()).abs().max())
    times = {k: [] for k in routes}
    for fn in routes.values():
        window_ms(fn, inner)
    for _ in range(reps):
        for k, fn in routes.items():
            times[k].append(window_ms(fn, inner))
    for k, t in times.items():
        r[k + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    r["copy_GBps"] = 2 * src.numel() * 4 / r["copy_ms"]["median"] * 1e-6
    r["folded_fwd_fraction_of_copy_rate"] = r["copy_ms"]["median"] / r["folded_fwd_ms"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_sincfast.py measures on the GPU"
    torch.manual_seed(0)
    out = {"shape": {"B": B, "n": N, "C": C, "sample_rate": SR}, "reps": a.reps, "inner": a.inner,
           "recipe": point(251, 1, 0, True, a.reps, a.inner), "strided": point(401, 160, 200, False, a.reps, a.inner)}
    for k in ("recipe", "strided"):
        print(k, json.dumps(out[k]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
