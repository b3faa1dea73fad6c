"""A `to_do = forward` chunk through core.run_nn_dp on three ranks of one GPU against the same chunk on one rank, at
PK_FORWARD_BATCH = 1 and 3 (worker: tests/forward_shard_gpu.py).  Every rank decodes a contiguous run of the sentence groups
(core.forward_shards), ranks above 0 write part files, rank 0 appends them: the arks must equal the one-rank arks byte for
byte, no part file may remain, the work must really be shared, and `.info` is written once.  Transport: gloo (RCCL refuses
several ranks per device); at most four processes hold the GPU - pytest and the three ranks.  Several ranks on one GPU prove
correctness, not speed."""
import configparser
import importlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import forward_shard_gpu as W

core = importlib.import_module("pytorch-kaldi_amd.core")
pytestmark = pytest.mark.gpu
WORLD = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_forward_chunk_on_three_ranks_equals_one_rank(tmp_path, monkeypatch):
    tmp = str(tmp_path)
    g = W.prepare(tmp, ("one", "dp"))
    lens = np.diff(W.chunk(g)[2], prepend=0)  # (the fixture's chunk, or the synthetic one if that is not worth sharding)
    assert len(lens) >= 3 and len(set(int(v) for v in lens)) > 1
    monkeypatch.setenv("PK_FORWARD_BATCH", "1")  # (run_chunk sets it per mode; restored afterwards)
    for n in W.MODES:
        did = W.run_chunk(g, tmp, "one", n)
        assert did["world"] == 1 and did["rank"] == 0 and did["sentences"] == len(lens) and did["frames"] == int(lens.sum())
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(WORLD), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), W.__file__, "--tmp", tmp, "--tag", "dp", "--world", str(WORLD)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    did = [json.load(open(tmp_path / ("rank%d.json" % k))) for k in range(WORLD)]
    for n in W.MODES:
        one, dp = tmp_path / ("one_n%d" % n), tmp_path / ("dp_n%d" % n)
        arks = sorted(p.name for p in one.glob("*.ark"))
        assert arks == ["forward_out_dnn2_to_decode.ark"]
        # no part file remains, the arks are the one-rank arks, .info is there once
        assert sorted(p.name for p in dp.iterdir()) == sorted(p.name for p in one.iterdir()) == sorted(arks + ["forward.cfg", "forward.info"])
        for name in arks:
            want = open(one / name, "rb").read()
            assert len(want) > 0 and open(dp / name, "rb").read() == want, (n, name)
        info = configparser.ConfigParser()
        info.read(dp / "forward.info")
        assert "loss" not in info["results"] and float(info["results"]["elapsed_time_chunk"]) > 0
        # the work is shared: the ranks' sentences add up to the chunk and at least two ranks decoded some
        per_rank = [d[str(n)] for d in did]
        assert [d["rank"] for d in per_rank] == list(range(WORLD)) and all(d["world"] == WORLD for d in per_rank)
        assert sum(d["sentences"] for d in per_rank) == len(lens), per_rank
        assert sum(d["frames"] for d in per_rank) == int(lens.sum()), per_rank
        assert sum(d["sentences"] > 0 for d in per_rank) >= 2, per_rank
        want_groups = [len(p) for p in core.forward_shards(lens, n, WORLD, True)]
        assert [d["groups"] for d in per_rank] == want_groups, (per_rank, want_groups)
