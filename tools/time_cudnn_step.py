"""Time forward + backward (+ fused RMSprop) of nn.LSTM_cudnn at the shape of cfg/TIMIT_baselines/TIMIT_LSTM_fmllr_cudnn.cfg
- 4 x 550 bidirectional, dropout 0.2, 40 inputs, T = 1000, batch 8 - and of the closest thing the engine ran before: its
reference-form LSTM 4 x 550 bidirectional without BatchNorm at the same shape; in bf16 and in exact-fp32 mode.

    python tools/time_cudnn_step.py [--T 1000] [--B 8] [--steps 5] [--rounds 3] [--json out.json]

Needs a GPU.  The reference-form LSTM shares one W / U between the directions and runs both in ONE recurrence launch of
2 B rows; LSTM_cudnn has a W / U per direction and runs two launches of B rows, one after the other.  Every module owns an
optim.FlatParams bucket and a fused RMSprop (the recipe's hyper-parameters), the step runs inside
functional.accumulating_backward() like core.run_nn's; the loss is sum(y * cot).  The modules are timed in alternating
windows of `steps` steps (host clock around a device synchronise), `rounds` windows each after 2 warm-up steps; the figure
reported is the median window, with the spread.  "LSTM_autograd" is the reference-form LSTM with its weight gradients on
the main stream through autograd, as LSTM_cudnn's are; "LSTM_uni_x2" is two passes of a UNIDIRECTIONAL reference-form LSTM
stack (B rows per launch, weight gradients through autograd): the recurrence launches LSTM_cudnn makes, without pack,
unpack and join.  The pack / unpack and join kernels are also timed on their own (device events, all launches one step
makes), so that the distance to the partner splits into: second recurrence launch, pack / unpack, join, main-stream weight
gradients.
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
    if kind == "LSTM_cudnn":
        net = nn_amd.LSTM_cudnn({"hidden_size": str(H), "num_layers": str(L), "bias": "True", "batch_first": "True",
                                 "dropout": "0.2", "bidirectional": "True", "use_cuda": "True", "to_do": "train"}, D)
    else:
        net = nn_amd.LSTM({"lstm_lay": rep(str(H)), "lstm_drop": rep("0.2"), "lstm_act": rep("tanh"),
                           "lstm_bidir": str(kind != "LSTM_uni_x2"), "lstm_use_laynorm_inp": "False",
                           "lstm_use_batchnorm_inp": "False", "lstm_use_laynorm": rep("False"), "lstm_use_batchnorm": rep("False"),
                           "lstm_orthinit": "False", "use_cuda": "True", "to_do": "train"}, D)
    net.cuda().train()
    opt = OPT.FusedOptimizer(OPT.FlatParams(net), "rmsprop", 0.0016, alpha=0.95, eps=1e-8)
    opt.zero_in_step = True
    if kind in ("LSTM_autograd", "LSTM_uni_x2"):
        for p in net.parameters():  # weight gradients off the side stream (functional.side_targets_ok asks for this mark)
            if p.dim() == 2:
                p._pk_flat = False
    return net, opt


def _event_ms(fn, reps=5):
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


def kernels_alone(T, B, D, H, L):
    """All pack / unpack launches and all join launches of one LSTM_cudnn step, on their own (ms)."""
    dev = "cuda"
    perm = F_.GATE_PERM["LSTM"]
    ws = [(torch.randn(4 * H, D if k == 0 else 2 * H, device=dev, requires_grad=True), torch.randn(4 * H, H, device=dev, requires_grad=True),
           torch.randn(4 * H, device=dev, requires_grad=True), torch.randn(4 * H, device=dev, requires_grad=True))
          for k in range(L) for _ in range(2)]
    packed = []

    def pack():
        packed[:] = [F_.gates_pack(*w, perm) for w in ws]

    def unpack():
        for (W, U, b), w in zip(packed, ws):
            torch.autograd.grad([W, U, b], list(w), [torch.ones_like(W), torch.ones_like(U), torch.ones_like(b)])

    yf, yb = (torch.randn(T, B, H, device=dev, requires_grad=True) for _ in range(2))
    x = torch.randn(T, B, D, device=dev)
    mask = torch.empty(T, B, 2 * H, device=dev).bernoulli_(0.8)
    g = torch.randn(T, B, 2 * H, device=dev)
    joined = []

    def join():
        joined[:] = [F_.seq_join(x, want_y=False, want_rev=True)]
        joined.extend(F_.seq_join(yf, yb, mask, 1.25, True, True) for _ in range(L - 1))
        joined.append(F_.seq_join(yf, yb, None, 1.0, True, False))

    def join_bwd():
        for y, y_rev in joined[1:-1]:
            torch.autograd.grad([y, y_rev], [yf, yb], [g, g])
        torch.autograd.grad([joined[-1][0]], [yf, yb], [g])

    out = {"pack_ms": _event_ms(pack)}
    out["unpack_ms"] = _event_ms(lambda: (pack(), unpack())) - out["pack_ms"]
    out["join_fwd_ms"] = _event_ms(join)
    out["join_bwd_ms"] = _event_ms(lambda: (join(), join_bwd())) - out["join_fwd_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--D", type=int, default=40)
    ap.add_argument("--H", type=int, default=550)
    ap.add_argument("--L", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_cudnn_step.py measures on the GPU; none is visible")
    torch.manual_seed(1)
    models = {k: build(k, a.H, a.L, a.D) for k in ("LSTM_cudnn", "LSTM", "LSTM_autograd", "LSTM_uni_x2")}
    x = torch.randn(a.T, a.B, a.D, device="cuda")
    cot = torch.randn(a.T, a.B, 2 * a.H, device="cuda") / (a.T * a.B)

    def step(kind):
        net, opt = models[kind]
        with F_.accumulating_backward():
            opt.zero_grad()
            if kind == "LSTM_uni_x2":  # the two launches of B rows per layer, as two passes of the unidirectional stack
                (net(x) * cot[:, :, :a.H]).sum().backward()
                (net(x) * cot[:, :, a.H:]).sum().backward()
            else:
                (net(x) * cot).sum().backward()
        opt.step()

    out = {"T": a.T, "B": a.B, "D": a.D, "H": a.H, "L": a.L, "steps": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "params": {k: sum(p.numel() for p in m[0].parameters()) for k, m in models.items()}}
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
        out[prec] = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}
        for k in ("LSTM_cudnn", "LSTM_autograd", "LSTM_uni_x2"):
            out[prec][k.lower() + "_over_lstm"] = out[prec][k]["ms_per_step"] / out[prec]["LSTM"]["ms_per_step"]
        print(prec, json.dumps(out[prec]), flush=True)
    F_.set_precision("fp32")
    out["kernels_alone"] = kernels_alone(a.T, a.B, a.D, a.H, a.L)
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
