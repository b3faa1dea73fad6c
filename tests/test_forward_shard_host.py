"""Host pieces of sharded forward chunks (pytorch-kaldi_amd/core.py; no GPU): core.forward_shards deals the sentence groups
of a `to_do = forward` chunk to the ranks as contiguous runs cut at the quantiles of the cumulative cost, and
core.merge_parts appends the ranks' part files to rank 0's ark."""
import importlib
import io
import os

import numpy as np
import pytest

core = importlib.import_module("pytorch-kaldi_amd.core")


def _cost(group, lens, seq_model):
    s, e, max_len = group
    return max_len * (e - s) if seq_model else int(sum(lens[s:e]))


@pytest.mark.parametrize("seq_model", [True, False], ids=["seq", "frames"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_forward_shards_partition_properties(n, world, seq_model):
    rng = np.random.RandomState(1000 * n + 10 * world + seq_model)
    for _ in range(40):
        lens = rng.randint(1, 51, size=rng.randint(1, 61))
        groups = core.forward_groups(lens, n)
        shards = core.forward_shards(lens, n, world, seq_model)
        assert len(shards) == world
        # the ranks' lists one after the other are the groups, in order: every rank holds one contiguous run
        assert [g for part in shards for g in part] == groups
        at = 0
        for part in shards:
            assert part == groups[at:at + len(part)]
            at += len(part)
        if world == 1:
            assert shards == [groups]
        # a rank is empty only behind the last group: more ranks than groups leaves the trailing ranks without work
        filled = [len(part) > 0 for part in shards]
        assert filled == sorted(filled, reverse=True), filled
        if world > len(groups):
            assert not any(filled[len(groups):])
        # the balance condition
        costs = [_cost(g, lens, seq_model) for g in groups]
        bound = sum(costs) / world + max(costs)
        for part in shards:
            assert sum(_cost(g, lens, seq_model) for g in part) <= bound, (list(lens), n, world, shards)


def test_forward_shards_cuts_at_the_cost_quantiles():
    # equal groups split evenly; one dear group does not starve the ranks behind it
    assert [len(p) for p in core.forward_shards([5] * 12, 1, 3, True)] == [4, 4, 4]
    assert [len(p) for p in core.forward_shards([5] * 12, 1, 3, False)] == [4, 4, 4]
    assert core.forward_shards([40, 1, 1], 1, 3, True) == [[(0, 1, 40)], [(1, 2, 1)], [(2, 3, 1)]]
    # padded frames, not frames, weigh a sequence model's groups: (10, 1) costs 20 padded and 11 real frames
    lens = [10, 1, 5, 5, 3, 3]  # groups of 2: 20, 10, 6 padded frames (half = 18), 11, 10, 6 frames (half = 13.5)
    assert [len(p) for p in core.forward_shards(lens, 2, 2, True)] == [1, 2]
    assert [len(p) for p in core.forward_shards(lens, 2, 2, False)] == [2, 1]
    assert core.forward_shards([], 4, 3, True) == [[], [], []]
    with pytest.raises(ValueError):
        core.forward_shards([3], 1, 0, True)


def test_merge_parts_equals_one_writer(tmp_path):
    rng = np.random.RandomState(7)
    mats = [rng.randn(3, 5).astype(np.float32), rng.randn(1, 4).astype(np.float64), rng.randn(6, 1).astype(np.float32),
            rng.randn(2, 2).astype(np.float64), rng.randn(4, 3).astype(np.float32), rng.randn(1, 1).astype(np.float64),
            rng.randn(7, 2).astype(np.float32)]
    keys = ["utt%d" % i for i in range(len(mats))]
    one = io.BytesIO()
    for k, m in zip(keys, mats):
        core.write_mat(one, m, k)
    final = tmp_path / "out_to_decode.ark"
    parts = [str(final) + ".part%d" % r for r in (1, 2, 3)]
    split = {str(final): range(0, 2), parts[0]: range(2, 5), parts[1]: range(0), parts[2]: range(5, 7)}  # the middle part empty
    for path, idx in split.items():
        with open(path, "wb") as f:
            for i in idx:
                core.write_mat(f, mats[i], keys[i])
    assert os.path.getsize(parts[1]) == 0
    core.merge_parts(str(final), parts)
    assert open(final, "rb").read() == one.getvalue()
    assert sorted(os.listdir(tmp_path)) == [final.name]
    # no parts (one rank): the file stays as it is
    core.merge_parts(str(final), [])
    assert open(final, "rb").read() == one.getvalue()
