#!/usr/bin/env python
"""Micro-benchmark of the fused optimizer steps through the C ABI: every form of pk_fused_step and pk_fused_step_ex,
timed with HIP events (warm-up, then --reps timed launches, the median), at two sizes - the flat bucket of the benchmark's
Li-GRU stack (its buffers stay in the 256 MB last-level cache) and 32 Mi elements (they do not).  Reports microseconds
and achieved GB/s from the bytes the form must move per parameter: 4 B read for each of p, g and every state buffer, 4 B
written for p and every state buffer, 4 B more for the gradient zeroed on the way out (zero_grad is on, as the training
loop runs it; no segment table, so no bf16 copies).

--parent-lib PATH: a libpk_amd.so built from the parent commit.  Its old entry points are timed in the same process,
launch by launch in turn with this tree's library, which is how "the old forms did not get slower" is read.

Writes profiles/optim_forms.json (or --out)."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
CENTERED, NESTEROV = 1, 2

# name -> (entry, kind, (h0, h1, h2), flags, number of state buffers in (s0, s1, s2) order: 1 = used, 0 = NULL)
FORMS = {
    "rmsprop": ("pk_fused_step", 0, (0.95, 1e-8, 0.0), 0, (1, 0, 0)),
    "sgd": ("pk_fused_step", 1, (0.0, 0.0, 0.0), 0, (0, 0, 0)),
    "sgd_momentum": ("pk_fused_step", 1, (0.9, 0.0, 0.0), 0, (1, 0, 0)),
    "adam": ("pk_fused_step", 2, (0.9, 0.999, 1e-8), 0, (1, 1, 0)),
    "rmsprop_momentum": ("pk_fused_step_ex", 0, (0.95, 1e-8, 0.9), 0, (1, 1, 0)),
    "rmsprop_centered": ("pk_fused_step_ex", 0, (0.95, 1e-8, 0.0), CENTERED, (1, 0, 1)),
    "rmsprop_momentum_centered": ("pk_fused_step_ex", 0, (0.95, 1e-8, 0.9), CENTERED, (1, 1, 1)),
    "sgd_nesterov": ("pk_fused_step_ex", 1, (0.9, 0.0, 0.0), NESTEROV, (1, 0, 0)),
    "sgd_dampening": ("pk_fused_step_ex", 1, (0.9, 0.3, 0.0), 0, (1, 0, 0)),
}


def bytes_per_param(form, zero_grad=True):
    nstate = sum(FORMS[form][4])
    return 4 * (2 + nstate), 4 * (1 + nstate) + (4 if zero_grad else 0)


def ligru_bucket():
    """Elements of the flat bucket the fused step of bench.py's Li-GRU stack covers (built on the host: only its size is used)."""
    U = importlib.import_module("pytorch-kaldi_amd.utils")
    R = importlib.import_module("pytorch-kaldi_amd.recipes")
    OPT = importlib.import_module("pytorch-kaldi_amd.optim")
    rcp = R.recipe("timit_ligru")
    nns, _ = U.model_init({"fea": rcp["fea_dict"]["fea"][5:]}, rcp["model"], rcp["cfg"], rcp["arch_dict"], False, False, "train")
    return max(OPT.FlatParams(m).n_active for m in nns.values())


def open_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("pk_fused_step", "pk_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def launcher(lib, form, n, bufs):
    entry, kind, h, flags, used = FORMS[form]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, g = bufs[0].data_ptr(), bufs[1].data_ptr()
    s = [bufs[2 + i].data_ptr() if u else None for i, u in enumerate(used)]
    fn = getattr(lib, entry)
    if entry == "pk_fused_step":
        args = (st, kind, p, g, s[0], s[1], s[2], n, 1e-3, h[0], h[1], h[2], 0.0, 2, 1, None, 0, None)
    else:
        args = (st, kind, p, g, s[0], s[1], s[2], n, 1e-3, h[0], h[1], h[2], 0.0, flags, 2, 1, None, 0, None)

    def run():
        if fn(*args) != 0:
            raise RuntimeError("%s failed: %s" % (entry, lib.pk_last_error()))
    return run


def time_in_turn(runs, reps, warmup):
    """One launch of every entry of `runs` per repetition, in turn (rotating who goes first), each between its own pair of
    events: median and minimum microseconds per entry."""
    for _ in range(warmup):
        for r in runs:
            r()
    torch.cuda.synchronize()
    ts = [[] for _ in runs]
    for rep in range(reps):
        # the launch that follows a synchronise starts on an idle GPU and reads as ~0.5 us longer: an untimed launch goes
        # first, and who comes first among the timed ones changes with every repetition
        order = [(rep + k) % len(runs) for k in range(len(runs))]
        runs[order[-1]]()
        evs = []
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[k]()
            e1.record()
            evs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_forms.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed launches")
    if not torch.cuda.is_available():
        sys.exit("bench_optim.py needs a GPU (no CPU timing)")
    lib = _lib.load()
    parent = open_parent(args.parent_lib) if args.parent_lib else None
    sizes = {"ligru_bucket": ligru_bucket(), "32Mi": 32 << 20}
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "zero_grad": 1, "sizes": sizes,
           "note": "median of per-launch HIP-event times; parent and this tree's library launched in turn in one process",
           "forms": [], "old_forms_vs_parent": []}
    for size_name, n in sizes.items():
        gen = torch.Generator(device="cuda").manual_seed(1)
        bufs = [torch.randn(n, device="cuda", generator=gen) for _ in range(2)] + [torch.zeros(n, device="cuda") for _ in range(3)]
        for form, (entry, *_rest) in FORMS.items():
            for b in bufs[2:]:
                b.zero_()
            bufs[1].normal_(generator=gen)
            runs = [launcher(lib, form, n, bufs)]
            if parent is not None and entry == "pk_fused_step":
                runs.append(launcher(parent, form, n, bufs))
            res = time_in_turn(runs, args.reps, args.warmup)
            rd, wr = bytes_per_param(form)
            med, mn = res[0]
            row = {"form": form, "entry": entry, "size": size_name, "n": n, "median_us": round(med, 2), "min_us": round(mn, 2),
                   "bytes_read_per_param": rd, "bytes_written_per_param": wr, "gb_per_s": round((rd + wr) * n / med / 1e3, 1)}
            rec["forms"].append(row)
            line = "%-26s %-12s %9.1f us  %7.1f GB/s" % (form, size_name, med, row["gb_per_s"])
            if len(res) > 1:
                pm = res[1][0]
                rec["old_forms_vs_parent"].append({"form": form, "size": size_name, "n": n, "parent_median_us": round(pm, 2),
                                                   "new_median_us": round(med, 2), "new_over_parent": round(med / pm, 4)})
                line += "   parent %9.1f us  new/parent %.4f" % (pm, med / pm)
            print(line, flush=True)
        del bufs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
