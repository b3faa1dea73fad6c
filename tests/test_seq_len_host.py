"""Host side of batched decoding (PK_FORWARD_BATCH, functional.sentence_lengths): the grouping of a forward chunk, the
argument checks of pk_seq_pack_len / pk_seq_join_len (they run before any device call), the lengths context, and the
pure-torch construction the GPU tests hold the kernels to (seq_len_util.py) - checked here against the reference's own
cat([x, flip(x)], dim=1) ... cat([h[:, :B], flip(h[:, B:])], dim=2) on every sentence alone."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from seq_len_util import LENS, T_MAX, host_join_len, host_pack_len, padded_batch

core = importlib.import_module("pytorch-kaldi_amd.core")
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

CHUNK_LENS = (12, 8, 11, 10, 9, 9, 5, 6, 12, 6)


def test_forward_groups():
    assert core.forward_groups(CHUNK_LENS, 4) == [(0, 4, 12), (4, 8, 9), (8, 10, 12)]
    assert core.forward_groups(CHUNK_LENS, 16) == [(0, 10, 12)]
    assert core.forward_groups(CHUNK_LENS, 1) == [(i, i + 1, n) for i, n in enumerate(CHUNK_LENS)]
    assert core.forward_groups(CHUNK_LENS, 10) == [(0, 10, 12)]
    assert core.forward_groups(np.asarray(CHUNK_LENS[:5]), 2) == [(0, 2, 12), (2, 4, 11), (4, 5, 9)]
    assert core.forward_groups((), 4) == []
    with pytest.raises(ValueError):
        core.forward_groups(CHUNK_LENS, 0)


def test_forward_batch_switch(monkeypatch):
    monkeypatch.delenv("PK_FORWARD_BATCH", raising=False)
    assert core.forward_batch() == 1
    monkeypatch.setenv("PK_FORWARD_BATCH", "16")
    assert core.forward_batch() == 16
    for bad in ("0", "-3", "many"):
        monkeypatch.setenv("PK_FORWARD_BATCH", bad)
        with pytest.raises(RuntimeError):
            core.forward_batch()


def test_padded_rows_scatter_and_gather():
    """Frame i of the group's concatenated sentences sits at row t * B + b of the flattened end-padded batch."""
    g = torch.Generator().manual_seed(2)
    sentences = [torch.randn(n, 3, generator=g) for n in LENS]
    want, lens = padded_batch(sentences)
    rows = torch.from_numpy(core.padded_rows(lens, T_MAX))
    frames = torch.cat(sentences, 0)
    got = torch.zeros(T_MAX * len(lens), 3).index_copy_(0, rows, frames)
    assert torch.equal(got.view(T_MAX, len(lens), 3), want)
    assert torch.equal(want.reshape(T_MAX * len(lens), 3).index_select(0, rows), frames)
    assert len(set(rows.tolist())) == sum(lens)
    with pytest.raises(AssertionError):
        core.padded_rows([3, 0], 3)
    with pytest.raises(AssertionError):
        core.padded_rows([3, 4], 3)


def test_entries_return_2_for_bad_arguments():
    """NULL where a pointer is required, a size below 1, both outputs NULL, a pitch smaller than a step: 2, a message,
    and nothing launched - the checks stand before any device call, so no GPU is needed (the pointers are never read)."""
    lib = _lib.load()
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    T, B, D, H = 2, 3, 4, 4
    good_pack = dict(x=p, lens=p, T=T, B=B, D=D, out_f=p, out_r=p, ldo=B * D)
    for change in (dict(x=None), dict(lens=None), dict(T=0), dict(B=0), dict(D=0), dict(T=-1), dict(out_f=None, out_r=None),
                   dict(ldo=B * D - 1), dict(ldo=0)):
        a = dict(good_pack, **change)
        rc = lib.pk_seq_pack_len(None, a["x"], a["lens"], a["T"], a["B"], a["D"], a["out_f"], a["out_r"], a["ldo"])
        assert rc == 2 and b"pk_seq_pack_len" in lib.pk_last_error(), change
    good_join = dict(hf=p, hb=p, ldi=B * H, lens=p, T=T, B=B, H=H, y_f=p, y_r=p, ldo=2 * B * H)
    for change in (dict(hf=None), dict(hb=None), dict(lens=None), dict(T=0), dict(B=0), dict(H=0), dict(H=-2),
                   dict(y_f=None, y_r=None), dict(ldi=B * H - 1), dict(ldo=2 * B * H - 1), dict(ldi=0), dict(ldo=0)):
        a = dict(good_join, **change)
        rc = lib.pk_seq_join_len(None, a["hf"], a["hb"], a["ldi"], a["lens"], a["T"], a["B"], a["H"], a["y_f"], a["y_r"],
                                 a["ldo"])
        assert rc == 2 and b"pk_seq_join_len" in lib.pk_last_error(), change


def test_sentence_lengths_nests_and_restores():
    assert F_.current_lengths() is None
    with F_.sentence_lengths([3, 2]) as outer:
        assert F_.current_lengths() is outer and outer.lens == (3, 2)
        with F_.sentence_lengths(np.asarray([1])) as inner:
            assert F_.current_lengths() is inner and inner.lens == (1,)
        assert F_.current_lengths() is outer
        with pytest.raises(KeyError):
            with F_.sentence_lengths([5]):
                raise KeyError("leaves the block through an exception")
        assert F_.current_lengths() is outer
        with outer:  # the same object entered again
            assert F_.current_lengths() is outer
        assert F_.current_lengths() is outer
    assert F_.current_lengths() is None


def test_lengths_are_checked_on_the_host():
    x = torch.zeros(4, 2, 3)
    F_.sentence_lengths([4, 1]).check("t", x)
    for bad in ([4, 0], [5, 1], [4, -1], [4], [4, 1, 1], []):
        with pytest.raises(_lib.PkError):
            F_.sentence_lengths(bad).check("t", x)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(_lib.PkError):
        F_.sentence_lengths([4, 1]).check("t", xg)
    with torch.no_grad():
        F_.sentence_lengths([4, 1]).check("t", xg)
    # the wrappers refuse a CPU tensor like every other entry of the package (no CPU path)
    with pytest.raises(_lib.PkError):
        F_.seq_pack_len(x, [4, 1])
    with pytest.raises(_lib.PkError):
        F_.seq_join_len(x, x, [4, 1])
    with pytest.raises(_lib.PkError):
        F_.seq_pack_len(x)  # no lengths in force


def _ref_flip(x):
    """The reference's flip of a [T, rows, .] tensor in time (neural_networks.py: flip(x, 0))."""
    return torch.flip(x, [0])


def test_host_construction_equals_the_reference_on_each_sentence_alone():
    g = torch.Generator().manual_seed(4)
    D, H = 5, 3
    sentences = [torch.randn(n, D, generator=g) for n in LENS]
    x, lens = padded_batch(sentences)
    assert tuple(lens) == LENS and x.shape[0] == T_MAX
    x = x + 0.0
    x[4:, 2] = 9.0  # what a per-row input normalisation leaves in the padding rows: pack zeroes them
    out_f, out_r = host_pack_len(x, lens)
    hf, hb = torch.randn(T_MAX, len(lens), H, generator=g), torch.randn(T_MAX, len(lens), H, generator=g)
    y, y_rev = host_join_len(hf, hb, lens)
    for b, n in enumerate(lens):
        xs = sentences[b].view(n, 1, D)
        packed = torch.cat([xs, _ref_flip(xs)], 1)  # [n, 2, D]
        assert torch.equal(out_f[:n, b], packed[:, 0]) and torch.equal(out_r[:n, b], packed[:, 1])
        assert float(out_f[n:, b].abs().max() if n < T_MAX else 0) == 0 and float(out_r[n:, b].abs().max() if n < T_MAX else 0) == 0
        h = torch.stack([hf[:n, b], hb[:n, b]], 1)  # [n, 2, H]: the layer's output on the packed rows
        joined = torch.cat([h[:, 0:1], _ref_flip(h[:, 1:2].contiguous())], 2)  # [n, 1, 2H]
        assert torch.equal(y[:n, b], joined[:, 0])
        assert torch.equal(y_rev[:n, b], _ref_flip(joined)[:, 0])  # the next layer's flip(x)
        if n < T_MAX:
            assert float(y[n:, b].abs().max()) == 0 and float(y_rev[n:, b].abs().max()) == 0


def test_host_construction_through_a_causal_stack_equals_each_sentence_alone():
    """Two bidirectional layers of a toy causal recurrence with shared weights, h_t = tanh(W x_t + 0.5 h_{t-1}): the
    batch run as a unidirectional layer on 2B packed rows with joins in between, against the reference's
    cat / flip form on each sentence alone.  Same arithmetic row by row, so the comparison is exact."""
    g = torch.Generator().manual_seed(6)
    D, H = 4, 3
    Ws = [torch.randn(D, H, generator=g), torch.randn(2 * H, H, generator=g)]

    def layer(x, W):  # [T, rows, .] -> [T, rows, H], causal, row by row
        h, out = torch.zeros(x.shape[1], W.shape[1]), []
        for t in range(x.shape[0]):
            h = torch.tanh((x[t].unsqueeze(2) * W.unsqueeze(0)).sum(1) + 0.5 * h)  # (a sum per row: no GEMM blocking)
            out.append(h)
        return torch.stack(out)

    sentences = [torch.randn(n, D, generator=g) for n in LENS]
    x, lens = padded_batch(sentences)
    B = len(lens)
    cur = torch.cat(host_pack_len(x, lens), 1)
    for i, W in enumerate(Ws):
        h = layer(cur, W)
        y, y_rev = host_join_len(h[:, :B], h[:, B:], lens)
        cur = torch.cat([y, y_rev], 1)
    for b, n in enumerate(lens):
        xs = sentences[b].view(n, 1, D)
        for W in Ws:
            xs = torch.cat([xs, _ref_flip(xs)], 1)
            h = layer(xs, W)
            xs = torch.cat([h[:, 0:1], _ref_flip(h[:, 1:2].contiguous())], 2)
        assert torch.equal(y[:n, b], xs[:, 0]), b
        if n < T_MAX:
            assert float(y[n:, b].abs().max()) == 0
