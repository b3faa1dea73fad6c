"""Time the fusion layer of nn.fusionRNN_jit at the shape of cfg/DIRHA_baselines/DIRHA_fusionRNN_MFCC_6ch.cfg - T = 500,
B = 16, 6 microphones x 13 features, fusion_layer_size 3072 (two instances of 512 columns), 4 x 512 bidirectional - in bf16
and in exact-fp32 mode:

  * functional.fusion_proj, forward and backward (with and without dx), against the device copy rate for the bytes it must
    move: x in and P out (forward), x and dP in (backward; dW, db and the workspace are small next to them);
  * the same projection as torch's stock conv1d + activation + sum with autograd, on the same GPU;
  * forward + backward of the whole class against the engine's liGRU of the same depth and width on the same input
    (parameters as plain tensors, no optimizer step in either).

    python tools/time_fusion_step.py [--json profiles/fusion_proj.json]

Needs a GPU.  Device events around one call, median of `--reps` after a warm-up call; the copy rate is torch's copy of a
buffer of the size of P, measured in the same run."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
T, B, M, F, H0, H, L = 500, 16, 6, 13, 512, 512, 4


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t)


def stock(x, W, b, slope):
    pre = torch.nn.functional.conv1d(x.view(x.shape[0], 1, M * F), W.view(2 * H0, 1, F), b, stride=F)  # [N, 2*H0, M]
    s = torch.cat([slope[:1].expand(H0), slope[1:].expand(H0)]).view(1, -1, 1)
    return torch.where(pre > 0, pre, s * pre).sum(2)


def stack(kind):
    rep = lambda v: ",".join([v] * L)  # noqa: E731
    if kind == "fusionRNN_jit":
        net = nn_amd.fusionRNN_jit({"fusionRNN_lay": rep(str(H)), "fusionRNN_drop": rep("0.2"), "fusionRNN_bidir": "True",
                                    "fusionRNN_act": rep("relu"), "fusionRNN_do_fusion": "True",
                                    "fusionRNN_fusion_layer_size": str(M * H0), "fusionRNN_number_of_mic": str(M),
                                    "fusionRNN_fusion_act": "prelu", "fusionRNN_fusion_reduce": "sum", "use_cuda": "True",
                                    "to_do": "train"}, M * F)
    else:
        net = nn_amd.liGRU({"ligru_lay": rep(str(H)), "ligru_drop": rep("0.2"), "ligru_use_laynorm_inp": "False",
                            "ligru_use_batchnorm_inp": "False", "ligru_use_laynorm": rep("False"), "ligru_use_batchnorm": rep("True"),
                            "ligru_bidir": "True", "ligru_act": rep("relu"), "ligru_orthinit": "True", "use_cuda": "True",
                            "to_do": "train"}, M * F)
    return net.cuda().train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    N = T * B
    x = torch.randn(N, M * F, device="cuda")
    W = (torch.randn(2 * H0, F, device="cuda") / F ** 0.5).requires_grad_()
    b, slope = torch.zeros(2 * H0, device="cuda", requires_grad=True), torch.full((2,), 0.25, device="cuda", requires_grad=True)
    cot = torch.randn(N, 2 * H0, device="cuda")
    dst = torch.empty_like(cot)
    copy_ms = event_ms(lambda: dst.copy_(cot), a.reps)
    rate = 2 * cot.numel() * 4 / copy_ms * 1e-6  # GB/s: the copy reads and writes the buffer
    out = {"shape": {"T": T, "B": B, "M": M, "F": F, "H0": H0, "layers": L, "H": H}, "copy_GBps": rate}
    xin = torch.randn(T, B, M * F, device="cuda")
    ycot = torch.randn(T, B, 2 * H, device="cuda")
    nets = {k: stack(k) for k in ("fusionRNN_jit", "liGRU")}
    for prec in ("bf16", "fp32"):
        F_.set_precision(prec)
        r = {}
        for tag, leaf in (("", x), ("_dx", x.clone().requires_grad_())):
            P = F_.fusion_proj(leaf, W, b, slope, M, "prelu", "sum")
            r["bwd%s_ms" % tag] = event_ms(lambda: torch.autograd.grad(P, [W] + ([leaf] if tag else []), cot, retain_graph=True), a.reps)
        r["fwd_ms"] = event_ms(lambda: F_.fusion_proj(x, W, b, slope, M, "prelu", "sum"), a.reps)
        r["fwd_fraction_of_copy_rate"] = (x.numel() + cot.numel()) * 4 / r["fwd_ms"] * 1e-6 / rate
        r["bwd_fraction_of_copy_rate"] = (x.numel() + cot.numel()) * 4 / r["bwd_ms"] * 1e-6 / rate
        if prec == "fp32":
            Ps = stock(x, W, b, slope)
            r["stock_fwd_ms"] = event_ms(lambda: stock(x, W, b, slope), a.reps)
            r["stock_bwd_ms"] = event_ms(lambda: torch.autograd.grad(Ps, [W], cot, retain_graph=True), a.reps)
        for kind, net in nets.items():
            def step():
                net.zero_grad(set_to_none=True)
                (net(xin) * ycot).sum().backward()
            r["step_%s_ms" % kind] = event_ms(step, a.reps)
        out[prec] = r
        print(prec, json.dumps(r))
    F_.set_precision("fp32")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
