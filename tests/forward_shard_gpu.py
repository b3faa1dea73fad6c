"""Worker of tests/test_gpu_forward_shard.py: one `to_do = forward` chunk through core.run_nn_dp on N ranks of ONE GPU (gloo:
RCCL refuses several ranks per device), at PK_FORWARD_BATCH = 1 and 3.  The chunk is the forward run of the
chunk_ligru_run_nn fixture (tests/test_core_chunk.py builds it the same way), log-prior normalisation on; chunk()
synthesises a chunk instead should the fixture's ever stop being worth sharding.  The test
prepares the folders - checkpoints and counts in --tmp, one cfg per mode in --tmp/<tag>_n<n>/ - and runs the same chunk in
its own process through run_chunk(); every rank leaves core.last_forward of both modes in --tmp/rank<r>.json.

TEST INFRASTRUCTURE (the engine is compared with itself: N ranks against one)."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from golden_util import Golden  # noqa: E402

CASE = "chunk_ligru_run_nn"
MODES = (1, 3)  # PK_FORWARD_BATCH


def prepare(tmp, tags):
    """Checkpoints, counts and one folder with a cfg per (tag, mode) under tmp."""
    from test_core_chunk import checkpoint_from_fixture, engine_cfg

    g = Golden(CASE)
    for i in (1, 2, 3):
        torch.save(checkpoint_from_fixture(g, "ck1", "architecture%d" % i), os.path.join(tmp, "ck1_architecture%d.pkl" % i))
    with open(os.path.join(tmp, "counts"), "w") as f:
        f.write("[ " + " ".join(str(int(c)) for c in g.arrays["counts"]) + " ]\n")
    text = engine_cfg(g, "forward", tmp)
    assert "normalize_posteriors = True" in text
    for tag in tags:
        for n in MODES:
            out = os.path.join(tmp, "%s_n%d" % (tag, n))
            os.makedirs(out)
            with open(os.path.join(out, "forward.cfg"), "w") as f:
                f.write(text.replace(str(tmp) + "/forward.info", out + "/forward.info"))
    return g


SYNTHETIC_LENS = (3, 3, 5, 8, 13, 21, 34)


def chunk(g):
    """(names, data, end) of the chunk that is decoded: the fixture's - or, should it ever have fewer than 3 sentences or
    only one length (nothing to share, or nothing a padded batch would have to get right), 7 seeded sentences of lengths
    3, 3, 5, 8, 13, 21, 34 at the fixture's feature width, label columns 0; the fixture's checkpoints either way."""
    data, end = g.arrays["data_set"], g.arrays["data_end_index"]
    lens = np.diff(end, prepend=0)
    if len(lens) >= 3 and len(set(int(v) for v in lens)) > 1:
        return g.meta["data_name"], data, end
    end = np.cumsum(SYNTHETIC_LENS).astype(end.dtype)
    synth = np.random.RandomState(0).randn(int(end[-1]), data.shape[1]).astype(data.dtype)
    for lab in g.meta["lab_dict"].values():
        synth[:, int(lab[3])] = 0.0
    return ["syn%02d" % i for i in range(len(SYNTHETIC_LENS))], synth, end


def run_chunk(g, tmp, tag, n):
    """The forward chunk with PK_FORWARD_BATCH = n into tmp/<tag>_n<n>/; returns core.last_forward."""
    core = importlib.import_module("pytorch-kaldi_amd.core")
    meta = g.meta
    os.environ["PK_FORWARD_BATCH"] = str(n)
    path = os.path.join(tmp, "%s_n%d" % (tag, n), "forward.cfg")
    names, data, end = chunk(g)
    args = [names, torch.from_numpy(data).cuda(), end,
            {k: list(v) for k, v in meta["fea_dict"].items()}, meta["lab_dict"], meta["arch_dict"]]
    core.run_nn_dp(*args, path, False, path, reader=lambda *a: None)
    return dict(core.last_forward)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tmp", required=True)
    ap.add_argument("--tag", required=True)
    ap.add_argument("--world", type=int, required=True)
    a = ap.parse_args()
    os.environ["LOCAL_RANK"] = "0"  # every rank on the one GPU of the box
    os.environ["PK_DP_BACKEND"] = "gloo"
    DP = importlib.import_module("pytorch-kaldi_amd.dp")
    rank, world, _ = DP.init_from_env("gloo")
    assert world == a.world
    g = Golden(CASE)
    did = {str(n): run_chunk(g, a.tmp, a.tag, n) for n in MODES}
    with open(os.path.join(a.tmp, "rank%d.json" % rank), "w") as f:
        json.dump(did, f)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
