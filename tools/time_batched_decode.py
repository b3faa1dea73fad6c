"""Time the decoding of a `to_do = forward` chunk sentence by sentence (PK_FORWARD_BATCH = 1, the loop core.run_nn_dp has
always run) against length-aware batches of 16 and 64 sentences (functional.sentence_lengths), in one process.

    python tools/time_batched_decode.py [--sentences 192] [--rounds 3] [--json profiles/batched_decode.json]

Needs a GPU.  The model is the TIMIT Li-GRU recipe's shape: 5 x 550 bidirectional Li-GRU with BatchNorm on 40 inputs and a
1938-class softmax head, eval mode, torch.no_grad().  The decode set is synthetic: `--sentences` sentences with lengths
drawn uniformly from 100 .. 700 (seed 0), in that order (nothing is sorted).  The two loops are run_nn_dp's, without the
ark writer: frames to the device, the stack, the head, ONE device-to-host copy per forward call (`decode_ms`); and the
recurrent stack alone, no head and no copy (`trunk_ms`).  Windows alternate between the batch sizes - one window decodes
the whole set `--passes` times, host clock around device synchronises, reported per pass - `--rounds` windows each after a warm-up window; the figure
reported is the median, with the spread, in bf16 and in exact-fp32 mode.  `padding_share` is the fraction of the padded
batches' rows that hold no frame; `speedup` is n = 1 over n, same process, same weights; `rel_diff_to_n1` is the
norm-relative distance of the first 64 sentences' log-posteriors from the n = 1 loop's.

    python tools/time_batched_decode.py --tail [--json profiles/forward_tail.json]

times what follows the head in run_nn_dp instead, the part the figures above leave out: log-prior normalisation, padding
strip, device-to-host copy and core.write_mat into /dev/null, for every sentence of the set.  The head's outputs of all
groups (random log-posteriors of the right shapes) are resident before a window starts, so a window holds the tail only.
Two arms per group size, in the same process, alternating: `host` - gather of the frame rows on the device, copy, numpy
`out - logprior` per sentence (PK_EXPERIMENT post_norm_device=0) - and `device` - functional.post_normalize, copy
(post_norm_device=1).  Both for the float32 log-priors data_io.load_counts leads to (the arks of the recipes are float32
matrices) and for float64 ones (float64 counts: numpy widens every posterior and the ark holds doubles)."""
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
core = importlib.import_module("pytorch-kaldi_amd.core")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")


def build(L, H, D, classes):
    rep = lambda v: ",".join([v] * L)  # noqa: E731
    net = nn_amd.liGRU({"ligru_lay": rep(str(H)), "ligru_drop": rep("0.2"), "ligru_use_laynorm_inp": "False",
                        "ligru_use_batchnorm_inp": "False", "ligru_use_laynorm": rep("False"), "ligru_use_batchnorm": rep("True"),
                        "ligru_bidir": "True", "ligru_act": rep("relu"), "ligru_orthinit": "True", "use_cuda": "True",
                        "to_do": "forward"}, D)
    head = nn_amd.MLP({"dnn_lay": str(classes), "dnn_drop": "0.0", "dnn_use_laynorm_inp": "False",
                       "dnn_use_batchnorm_inp": "False", "dnn_use_batchnorm": "False", "dnn_use_laynorm": "False",
                       "dnn_act": "softmax"}, net.out_dim)
    return net.cuda().eval(), head.cuda().eval()


def _rows(y, n_rows):
    """(T, B, F) -> (T*B, F) the way utils.forward_model does it: the bf16 copy of a perf-mode stack goes along."""
    twin = getattr(y, "_pk_twin", None)
    y = y.reshape(n_rows, -1)
    if twin is not None:
        y._pk_twin = (twin[0], twin[1], y._version)
    return y


def decode(net, head, data, end, n, whole, keep=None):
    """One pass over the set, n sentences per forward call.  whole: head and device-to-host copy included; keep: a list
    that receives the host arrays."""
    lens_all = core.sentence_lengths(end)
    kept = 0
    with torch.no_grad():
        for s, e, max_len in core.forward_groups(lens_all, n):
            lens, nb = [int(v) for v in lens_all[s:e]], e - s
            frames = data[int(end[s]) - lens[0]:int(end[e - 1])]
            if n == 1:  # run_nn_dp's sentence-by-sentence loop
                y = net(frames.view(lens[0], 1, -1))
                if whole:
                    host = head(_rows(y, lens[0])).cpu().numpy()
                    kept += host.shape[0]
                    if keep is not None:
                        keep.append(host)
                continue
            rows = torch.from_numpy(core.padded_rows(lens, max_len)).to(frames.device)
            inp = torch.zeros(max_len * nb, frames.shape[1], device=frames.device).index_copy_(0, rows, frames)
            with F_.sentence_lengths(lens):
                y = net(inp.view(max_len, nb, -1))
            if whole:
                host = head(_rows(y, max_len * nb)).index_select(0, rows).cpu().numpy()
                kept += host.shape[0]
                if keep is not None:
                    keep.append(host)
    torch.cuda.synchronize()
    assert not whole or kept == int(end[-1])


def tail_groups(lens, n, classes, seed):
    """Per group: (lens, rows on the device or None, rows on the host, the head's output [R, classes] on the device)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for s, e, max_len in core.forward_groups(lens, n):
        ls = [int(v) for v in lens[s:e]]
        if n == 1:
            rows = rows_host = None
            R = ls[0]
        else:
            rows_host = core.padded_rows(ls, max_len)
            rows = torch.from_numpy(rows_host).cuda()
            R = max_len * len(ls)
        out.append((ls, rows, rows_host, -30.0 * torch.rand(R, classes, device="cuda", generator=gen)))
    return out


def tail(groups, arm, lp_host, lp_dev, sink, keep=None):
    """One pass over the set: what run_nn_dp does behind the head for a normalised output."""
    for ls, rows, rows_host, x in groups:
        if arm == "device":
            host = F_.post_normalize(x, lp_dev, rows, rows_host).cpu().numpy()
        else:
            host = (x if rows is None else x.index_select(0, rows)).cpu().numpy()
        beg = 0
        for k, L in enumerate(ls):
            m = host[beg:beg + L]
            if arm == "host":
                m = m - lp_host
            core.write_mat(sink, m, "utt%05d" % k)
            if keep is not None:
                keep.append(m)
            beg += L


def tail_main(a):
    ns = [int(v) for v in a.batches.split(",")]
    lens = np.random.RandomState(0).randint(a.min_len, a.max_len + 1, size=a.sentences)
    counts = np.random.RandomState(3).randint(1, 100000, size=a.classes)
    out = {"mode": "tail", "sentences": a.sentences, "frames": int(lens.sum()), "lengths": [a.min_len, a.max_len],
           "classes": a.classes, "rounds": a.rounds, "passes": a.passes, "device": torch.cuda.get_device_name(0),
           "elements": int(lens.sum()) * a.classes, "sink": os.devnull}
    with open(os.devnull, "wb") as sink:
        for dtype in ("float32", "float64"):
            c = counts.astype(dtype)
            lp_host = np.log(c / np.sum(c))
            lp_dev = torch.from_numpy(lp_host).cuda()
            arms = [(n, arm) for n in ns for arm in ("host", "device")]
            sets = {n: tail_groups(lens, n, a.classes, 10 + n) for n in ns}
            for n in ns:  # same bytes first
                got = {arm: [] for arm in ("host", "device")}
                for arm in got:
                    tail(sets[n][:4], arm, lp_host, lp_dev, sink, got[arm])
                assert all(h.dtype == d.dtype == lp_host.dtype and np.array_equal(h, d) for h, d in zip(got["host"], got["device"]))
            for n, arm in arms:  # warm-up window: allocator, pinned staging, first launch
                tail(sets[n], arm, lp_host, lp_dev, sink)
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(a.rounds):
                for n, arm in arms:
                    torch.cuda.synchronize()  # (nothing of the previous arm's window is left on the device)
                    t0 = time.perf_counter()
                    for _ in range(a.passes):
                        tail(sets[n], arm, lp_host, lp_dev, sink)
                    torch.cuda.synchronize()
                    ms[(n, arm)].append(1e3 * (time.perf_counter() - t0) / a.passes)
            out[dtype] = {str(n): {arm: {"median": statistics.median(ms[(n, arm)]), "min": min(ms[(n, arm)]),
                                         "max": max(ms[(n, arm)])} for arm in ("host", "device")} for n in ns}
            for n in ns:
                d = out[dtype][str(n)]
                d["host_over_device"] = d["host"]["median"] / d["device"]["median"]
            print(dtype, "tail_ms", json.dumps(out[dtype]), flush=True)
            del sets
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=192)
    ap.add_argument("--min-len", type=int, default=100)
    ap.add_argument("--max-len", type=int, default=700)
    ap.add_argument("--L", type=int, default=5)
    ap.add_argument("--H", type=int, default=550)
    ap.add_argument("--D", type=int, default=40)
    ap.add_argument("--classes", type=int, default=1938)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2, help="passes over the set per timed window")
    ap.add_argument("--check", type=int, default=64, help="sentences whose outputs are compared between the batch sizes")
    ap.add_argument("--json", default=None)
    ap.add_argument("--tail", action="store_true", help="time what follows the head: normalisation, copy, ark writer")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_batched_decode.py measures on the GPU; none is visible")
    if a.tail:
        return tail_main(a)
    ns = [int(v) for v in a.batches.split(",")]
    assert ns[0] == 1, "the baseline, n = 1, comes first"
    torch.manual_seed(1)
    net, head = build(a.L, a.H, a.D, a.classes)
    lens = np.random.RandomState(0).randint(a.min_len, a.max_len + 1, size=a.sentences)
    end = np.cumsum(lens)
    data = torch.randn(int(end[-1]), a.D, generator=torch.Generator().manual_seed(2)).cuda()
    out = {"sentences": a.sentences, "frames": int(end[-1]), "lengths": [a.min_len, a.max_len], "L": a.L, "H": a.H, "D": a.D,
           "classes": a.classes, "rounds": a.rounds, "passes": a.passes, "device": torch.cuda.get_device_name(0),
           "padding_share": {str(n): 1.0 - float(end[-1]) / sum((e - s) * t for s, e, t in core.forward_groups(lens, n))
                             for n in ns}}
    for prec in ("bf16", "fp32"):
        F_.set_precision(prec)
        out[prec] = {}
        # same results first: the log-posteriors of the first sentences, every batch size against n = 1 (norm-relative)
        m = min(a.check, a.sentences)
        got = {}
        for n in ns:
            got[n] = []
            decode(net, head, data[:int(end[m - 1])], end[:m], n, True, got[n])
            got[n] = np.concatenate(got[n], 0).astype(np.float64)
        out[prec]["rel_diff_to_n1"] = {str(n): float(np.linalg.norm(got[n] - got[1]) / np.linalg.norm(got[1])) for n in ns[1:]}
        print(prec, "rel_diff_to_n1", json.dumps(out[prec]["rel_diff_to_n1"]), flush=True)
        del got
        for key, whole in (("decode_ms", True), ("trunk_ms", False)):
            for n in ns:  # warm-up window: allocator, weight copies, first-launch costs
                decode(net, head, data, end, n, whole)
            ms = {n: [] for n in ns}
            for _ in range(a.rounds):
                for n in ns:
                    t0 = time.perf_counter()
                    for _ in range(a.passes):
                        decode(net, head, data, end, n, whole)
                    ms[n].append(1e3 * (time.perf_counter() - t0) / a.passes)
            _lib.raise_if_persist_failed()
            base = statistics.median(ms[1])
            out[prec][key] = {str(n): {"median": statistics.median(v), "min": min(v), "max": max(v),
                                       "speedup": base / statistics.median(v)} for n, v in ms.items()}
            print(prec, key, json.dumps(out[prec][key]), flush=True)
    F_.set_precision("fp32")
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
