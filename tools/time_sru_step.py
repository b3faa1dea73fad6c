"""Time forward + backward (+ fused Adam) of nn.SRU at the shape of cfg/TIMIT_baselines/TIMIT_SRU_fbank.cfg - 4 x 550
bidirectional, n_proj 256, dropout 0.1 / 0.1, skip term, rescale - on 440 inputs, and of the engine's Li-GRU of the same
depth and width (BatchNorm, relu: the flagship recipe) in the same process; at T = 500, B = 128 and at T = 1000, B = 8 (the
recipe's batch), in bf16 and in exact-fp32 mode.

    python tools/time_sru_step.py [--steps 5] [--rounds 3] [--json profiles/sru_step.json]

Needs a GPU.  Every module owns an optim.FlatParams bucket and a fused optimizer, the step runs inside
functional.accumulating_backward() like core.run_nn's; the loss is sum(y * cot).  The modules are timed in alternating
windows of `steps` steps (host clock around a device synchronise), `rounds` windows each after 2 warm-up steps; the figure
reported is the median window, with the spread.

The scan kernels are also timed alone (device events, median of 7 launches) for the inner layers' forms - k = 3 with a
skip source, the masked second output, both gradients - and set against the device copy rate measured in the same run
(torch's copy of a buffer of the size of U): bytes the kernel must move / its time, as a fraction of that rate.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
OPT = importlib.import_module("pytorch-kaldi_amd.optim")


def build(kind, H, L, D):
    rep = lambda v: ",".join([v] * L)  # noqa: E731
    if kind == "SRU":
        net = nn_amd.SRU({"sru_hidden_size": str(H), "sru_num_layers": str(L), "sru_dropout": "0.1", "sru_rnn_dropout": "0.1",
                          "sru_use_tanh": "False", "sru_use_relu": "False", "sru_use_selu": "False", "sru_weight_norm": "False",
                          "sru_layer_norm": "False", "sru_bidirectional": "True", "sru_is_input_normalized": "False",
                          "sru_has_skip_term": "True", "sru_rescale": "True", "sru_highway_bias": "-1", "sru_n_proj": "256",
                          "use_cuda": "True", "to_do": "train"}, D)
        opt = ("adam", 0.0004)
    else:
        net = nn_amd.liGRU({"ligru_lay": rep(str(H)), "ligru_drop": rep("0.2"), "ligru_use_laynorm_inp": "False",
                            "ligru_use_batchnorm_inp": "False", "ligru_use_laynorm": rep("False"),
                            "ligru_use_batchnorm": rep("True"), "ligru_bidir": "True", "ligru_act": rep("relu"),
                            "ligru_orthinit": "True", "use_cuda": "True", "to_do": "train"}, D)
        opt = ("rmsprop", 0.0004)
    net.cuda().train()
    if opt[0] == "adam":
        o = OPT.FusedOptimizer(OPT.FlatParams(net), "adam", opt[1], betas=(0.9, 0.999), eps=1e-8)
    else:
        o = OPT.FusedOptimizer(OPT.FlatParams(net), "rmsprop", opt[1], alpha=0.95, eps=1e-8)
    o.zero_in_step = True
    return net, o


def _event_ms(fn, reps=7):
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


def scan_alone(T, B, H):
    """The inner layers' scan (k = 3, skip source, masked copy) on its own: ms, bytes moved, fraction of the copy rate."""
    dev, out = "cuda", 2 * H
    U = torch.randn(T, B, 3 * out, device=dev)
    x = torch.randn(T, B, out, device=dev)
    wc, bias = torch.rand(2 * out, device=dev) * 2 - 1, torch.cat([torch.zeros(out), -torch.ones(out)]).to(dev)
    mh, mn = torch.ones(B, out, device=dev), torch.ones(B, out, device=dev)
    g = torch.randn(T, B, out, device=dev)
    dst = torch.empty_like(U)
    copy_ms = _event_ms(lambda: dst.copy_(U))
    copy_rate = 2 * U.numel() * 4 / (copy_ms * 1e-3)
    keep = {}

    def fwd():
        Ul = U.clone().requires_grad_()
        keep["U"] = Ul
        keep["y"] = F_.sru_scan(Ul, x, wc, bias, 1.3, "none", mask_h=mh, bidirectional=True, mask_next=mn)

    def fwd_bwd():
        fwd()
        torch.autograd.grad(list(keep["y"]), [keep["U"]], [g, g])

    clone_ms = _event_ms(lambda: U.clone())
    f_ms = _event_ms(fwd) - clone_ms
    b_ms = _event_ms(fwd_bwd) - clone_ms - f_ms
    n = T * B * out * 4
    f_bytes, b_bytes = n * (3 + 1 + 3), n * (3 + 1 + 1 + 2 + 3 + 1)  # U, x -> Y, C, Ym;  U, C, x, dY, dYm -> dU, dx_skip
    res = {"copy_ms": copy_ms, "copy_GBps": copy_rate / 1e9}
    for name, ms, nbytes in (("scan_fwd", f_ms, f_bytes), ("scan_bwd", b_ms, b_bytes)):
        res[name] = {"ms": ms, "bytes": nbytes, "GBps": nbytes / (ms * 1e-3) / 1e9,
                     "fraction_of_copy_rate": nbytes / (ms * 1e-3) / copy_rate}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=440)
    ap.add_argument("--H", type=int, default=550)
    ap.add_argument("--L", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="500x128,1000x8")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sru_step.py measures on the GPU; none is visible")
    torch.manual_seed(1)
    models = {k: build(k, a.H, a.L, a.D) for k in ("SRU", "liGRU")}
    out = {"D": a.D, "H": a.H, "L": a.L, "steps": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "params": {k: sum(p.numel() for p in m[0].parameters()) for k, m in models.items()}, "shapes": {}}
    for shape in a.shapes.split(","):
        T, B = (int(v) for v in shape.split("x"))
        x = torch.randn(T, B, a.D, device="cuda")
        cot = torch.randn(T, B, 2 * a.H, device="cuda") / (T * B)

        def step(kind):
            net, opt = models[kind]
            with F_.accumulating_backward():
                opt.zero_grad()
                (net(x) * cot).sum().backward()
            opt.step()

        res = {}
        for prec in ("bf16", "fp32"):
            F_.set_precision(prec)
            for kind in models:
                for _ in range(2):
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
            res[prec] = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}
            res[prec]["sru_over_ligru"] = res[prec]["SRU"]["ms_per_step"] / res[prec]["liGRU"]["ms_per_step"]
            print(shape, prec, json.dumps(res[prec]), flush=True)
        F_.set_precision("fp32")
        res["scan_alone"] = scan_alone(T, B, a.H)
        print(shape, "scan", json.dumps(res["scan_alone"]), flush=True)
        out["shapes"][shape] = res
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
