"""Time one training step (forward + backward + fused RMSprop) of nn.QLSTM and of its LSTM twin - the engine's own LSTM
without normalisation at the same widths, i.e. the same recurrences and GEMMs on weights that are parameters instead of
assembled matrices - at the shape of cfg/DIRHA_baselines/DIRHA_QLSTM_MFCC.cfg: 4 x 512 bidirectional, 52 inputs,
T = 500, batch 16, drop 0.2, tanh; in bf16 and in exact-fp32 mode.

    python tools/time_qlstm_step.py [--T 500] [--B 16] [--steps 10] [--rounds 3] [--json out.json]

Needs a GPU.  Both modules own an optim.FlatParams bucket and a fused RMSprop (the recipe's hyper-parameters), the step
runs inside functional.accumulating_backward() like core.run_nn's; the loss is sum(y * cot).  The modules are timed in
alternating windows of `steps` steps (host clock around a device synchronise), `rounds` windows each after 3 warm-up
steps; the figure reported is the median window, with the spread.  A third module, "LSTM_autograd", is the twin with
its weight gradients on the main stream through autograd, as QLSTM's are: it splits QLSTM's distance from the twin into
what the lost overlap costs and what assembly, fold and the components' accumulation cost.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
OPT = importlib.import_module("pytorch-kaldi_amd.optim")


def build(kind, lay, D):
    n = len(lay)
    rep = lambda v: ",".join([v] * n)  # noqa: E731
    opts = {"lstm_lay": ",".join(map(str, lay)), "lstm_drop": rep("0.2"), "lstm_act": rep("tanh"), "lstm_bidir": "True",
            "use_cuda": "True", "to_do": "train"}
    if kind == "QLSTM":
        net = nn_amd.QLSTM(dict(opts, autograd="False", quaternion_init="quaternion"), D)
    else:
        net = nn_amd.LSTM(dict(opts, lstm_use_laynorm_inp="False", lstm_use_batchnorm_inp="False", lstm_use_laynorm=rep("False"),
                               lstm_use_batchnorm=rep("False"), lstm_orthinit="False"), D)
    net.cuda().train()
    opt = OPT.FusedOptimizer(OPT.FlatParams(net), "rmsprop", 0.0016, alpha=0.95, eps=1e-8)
    opt.zero_in_step = True
    if kind == "LSTM_autograd":
        # the diagnostic variant: the twin with its weight gradients taken off the side stream (functional.side_targets_ok
        # asks for this mark), i.e. concatenated weights with autograd history, dW / dU GEMMs on the main stream and
        # autograd's own accumulation into the flat .grad - what QLSTM does, without the assembly and the fold
        for p in net.parameters():
            if p.dim() == 2:
                p._pk_flat = False
    return net, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--D", type=int, default=52)
    ap.add_argument("--lay", default="512,512,512,512")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_qlstm_step.py measures on the GPU; none is visible")
    lay = [int(v) for v in a.lay.split(",")]
    np.random.seed(1)
    torch.manual_seed(1)
    models = {k: build(k, lay, a.D) for k in ("QLSTM", "LSTM", "LSTM_autograd")}
    x = torch.randn(a.T, a.B, a.D, device="cuda")
    cot = torch.randn(a.T, a.B, 2 * lay[-1], device="cuda") / (a.T * a.B)

    def step(kind):
        net, opt = models[kind]
        with F_.accumulating_backward():
            y = net(x)
            opt.zero_grad()
            (y * cot).sum().backward()
        opt.step()

    out = {"T": a.T, "B": a.B, "D": a.D, "lay": lay, "steps": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "params": {k: sum(p.numel() for p in m[0].parameters()) for k, m in models.items()}}
    for prec in ("bf16", "fp32"):
        F_.set_precision(prec)
        for kind in models:
            for _ in range(3):
                step(kind)
        torch.cuda.synchronize()
        ms = {k: [] for k in models}
        for _ in range(a.rounds):
            for kind in models:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(kind)
                torch.cuda.synchronize()
                ms[kind].append(1e3 * (time.perf_counter() - t0) / a.steps)
        out[prec] = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}
        for k in ("QLSTM", "LSTM_autograd"):
            out[prec][k.lower() + "_over_lstm"] = out[prec][k]["ms_per_step"] / out[prec]["LSTM"]["ms_per_step"]
        print(prec, json.dumps(out[prec]), flush=True)
    F_.set_precision("fp32")
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
