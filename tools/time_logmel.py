"""Time functional.log_mel_fb (pk_logmel.hip) at the front-end's usual shape - 16 kHz, 3.2 s of audio, a 400-sample window
shifted by 160, 40 mel filters - for batches of 8 and 128 sentences, against

  * torch's device copy of the bytes the kernel must move (x in, y out: a copy of a buffer of half that size), same run;
  * the stock route of the reference (torch.stft, pow, sum, transposes, matmul, max, log10) on the device, if this torch
    build has a device FFT - otherwise that column is left out and the reason recorded.

    python tools/time_logmel.py [--json profiles/logmel.json]

Needs a GPU.  Device events around `--inner` back-to-back calls, per-call time = window / inner; median, minimum and maximum
of `--reps` windows after a warm-up window.  The three routes alternate inside every repetition."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
SR, WS, HOP, N_MELS, SECONDS = 16000, 400, 160, 40, 3.2


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def stock(x, window, fb):
    s = torch.view_as_real(torch.stft(x.t(), WS, hop_length=HOP, center=False, window=window, return_complex=True))
    p = s.pow(2).sum(-1).transpose(1, 2)
    return torch.log10(torch.max(torch.matmul(p, fb).transpose(0, 1), torch.full((1,), 1e-20, device=x.device)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_logmel.py measures on the GPU"
    torch.manual_seed(0)
    T = int(SR * SECONDS)
    basis = F_.logmel_basis(WS).cuda()
    fb = F_.mel_fbanks(SR, WS // 2 + 1, N_MELS).float().cuda()
    window = torch.hann_window(WS, device="cuda")
    out = {"shape": {"sample_rate": SR, "ws": WS, "hop": HOP, "n_mels": N_MELS, "T": T}, "reps": a.reps, "inner": a.inner}
    for B in (8, 128):
        x = 0.3 * torch.randn(T, B, device="cuda")
        y = F_.log_mel_fb(x, basis, fb, WS, HOP)
        moved = (x.numel() + y.numel()) * 4
        src = torch.empty(moved // 8, device="cuda")
        dst = torch.empty_like(src)
        routes = {"kernel": lambda: F_.log_mel_fb(x, basis, fb, WS, HOP), "copy": lambda: dst.copy_(src)}
        r = {"bytes_moved": moved, "flop": 2 * y.shape[0] * B * (2 * WS * (WS // 2 + 1) + (WS // 2 + 1) * N_MELS)}
        try:
            ys = stock(x, window, fb)
            r["stock_vs_kernel_max_abs_diff"] = float((ys - y).abs().max())
            routes["stock"] = lambda: stock(x, window, fb)
        except RuntimeError as e:
            r["stock"] = "left out: no device FFT in this torch build (%s)" % str(e).splitlines()[0][:120]
        times = {k: [] for k in routes}
        for fn in routes.values():
            window_ms(fn, a.inner)
        for _ in range(a.reps):
            for k, fn in routes.items():
                times[k].append(window_ms(fn, a.inner))
        for k, t in times.items():
            r[k + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        r["copy_GBps"] = 2 * src.numel() * 4 / r["copy_ms"]["median"] * 1e-6
        r["kernel_fraction_of_copy_rate"] = r["copy_ms"]["median"] / r["kernel_ms"]["median"]
        r["kernel_TFLOPs"] = r["flop"] / r["kernel_ms"]["median"] * 1e-9
        out["B%d" % B] = r
        print("B = %d" % B, json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
