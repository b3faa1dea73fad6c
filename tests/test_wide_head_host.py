"""The fused output head for 2049 .. 8192 classes without a GPU: the argument checks of the six C-ABI entries (which come
before any device call), the workspace sizes of the wave-per-row kernels (unchanged: pinned to what the library returned
before the block-per-row kernels existed) and of the block-per-row ones, the PK_EXPERIMENT head_block lever as the
workspace-size function sees it, and the gate in functional.linear_log_softmax_ok."""
import importlib

import pytest
import torch

F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

FAKE = 4096  # never dereferenced: the checks come first
BLOCK_CAP = 1024  # blocks of the block-per-row backward: a row per block up to this many (pk_norm.hip, lsm_bf16_block_blocks)


def _bwd(lib, N, ldb):
    return lib.pk_logsoftmax_bwd_bf16(None, FAKE, FAKE, 4, N, FAKE, ldb, FAKE, FAKE)


def _nll_bwd(lib, N, ldb):
    return lib.pk_nll_logsoftmax_bwd_bf16(None, FAKE, FAKE, FAKE, FAKE, -100, 4, N, FAKE, ldb, FAKE, FAKE)


def _bwd_p(lib, N, ldb, pitch=None):
    return lib.pk_logsoftmax_bwd_bf16_p(None, FAKE, FAKE, 4, N, FAKE, ldb, ldb + 64 if pitch is None else pitch, FAKE, FAKE)


def _nll_bwd_p(lib, N, ldb, pitch=None):
    return lib.pk_nll_logsoftmax_bwd_bf16_p(None, FAKE, FAKE, FAKE, FAKE, -100, 4, N, FAKE, ldb, ldb + 64 if pitch is None else pitch,
                                            FAKE, FAKE)


@pytest.mark.parametrize("name,call", [("pk_logsoftmax_bwd_bf16", _bwd), ("pk_nll_logsoftmax_bwd_bf16", _nll_bwd),
                                       ("pk_logsoftmax_bwd_bf16_p", _bwd_p), ("pk_nll_logsoftmax_bwd_bf16_p", _nll_bwd_p)])
def test_backward_entries_refuse_bad_widths_before_any_device_call(name, call):
    lib = _lib.load()
    for N, ldb in [(8193, 8256),     # one class too many
                   (8193, 8192),
                   (8190, 8200),     # the padded width beyond what a block covers
                   (3400, 3392),     # pitch shorter than a row
                   (2049, 2049),     # not a multiple of 8
                   (3400, 3404),
                   (0, 64)]:
        assert call(lib, N, ldb) != 0, (N, ldb)
        assert name.encode() + b":" in lib.pk_last_error(), (N, ldb, lib.pk_last_error())


def test_pitched_entries_refuse_a_pitch_below_the_written_width():
    lib = _lib.load()
    for call, name in ((_bwd_p, b"pk_logsoftmax_bwd_bf16_p:"), (_nll_bwd_p, b"pk_nll_logsoftmax_bwd_bf16_p:")):
        assert call(lib, 3400, 3456, pitch=3448) != 0
        assert name in lib.pk_last_error()
        assert call(lib, 3400, 3456, pitch=3460) != 0   # not a multiple of 8
        assert name in lib.pk_last_error()


def test_forward_and_cost_entries_refuse_bad_widths_before_any_device_call():
    lib = _lib.load()
    assert lib.pk_logsoftmax_fwd_ld_argmax(None, FAKE, 8224, 4, 8193, FAKE, FAKE) != 0
    assert b"pk_logsoftmax_fwd_ld_argmax:" in lib.pk_last_error()
    assert lib.pk_logsoftmax_fwd_ld_argmax(None, FAKE, 3392, 4, 3400, FAKE, FAKE) != 0   # pitch shorter than a row
    assert b"pk_logsoftmax_fwd_ld_argmax:" in lib.pk_last_error()
    assert lib.pk_logsoftmax_fwd_ld_argmax(None, FAKE, 64, 4, 0, FAKE, FAKE) != 0
    assert lib.pk_logsoftmax_fwd_ld_argmax(None, FAKE, 3424, 4, 3400, FAKE, None) != 0
    assert b"pk_logsoftmax_fwd_ld_argmax:" in lib.pk_last_error()
    assert lib.pk_nll_err_fwd(None, FAKE, FAKE, -100, 4, 8193, FAKE, FAKE, None, None) != 0
    assert b"pk_nll_err_fwd:" in lib.pk_last_error()
    assert lib.pk_nll_err_fwd(None, FAKE, FAKE, -100, 0, 3400, FAKE, FAKE, None, None) != 0
    assert lib.pk_nll_err_fwd(None, FAKE, FAKE, -100, 4, 3400, None, FAKE, None, None) != 0
    assert b"pk_nll_err_fwd:" in lib.pk_last_error()


def test_null_workspaces_are_refused_at_the_new_widths():
    lib = _lib.load()
    assert lib.pk_logsoftmax_bwd_bf16(None, FAKE, FAKE, 4, 3400, FAKE, 3456, None, FAKE) != 0
    assert b"pk_logsoftmax_bwd_bf16:" in lib.pk_last_error()
    assert lib.pk_nll_logsoftmax_bwd_bf16(None, FAKE, None, FAKE, FAKE, -100, 4, 3400, FAKE, 3456, FAKE, FAKE) != 0
    assert b"pk_nll_logsoftmax_bwd_bf16:" in lib.pk_last_error()


# what the library returned before the block-per-row kernels existed (computed on the parent commit)
PINNED = [((64000, 1938), 2003892, 16384), ((64000, 48), 384000, 16384), ((128, 1944), 124416, 512), ((5, 2048), 8192, 32)]


@pytest.mark.parametrize("shape,bwd_floats,nll_floats", PINNED)
def test_workspaces_of_the_wave_kernels_are_unchanged(shape, bwd_floats, nll_floats, monkeypatch):
    monkeypatch.delenv("PK_EXPERIMENT", raising=False)
    lib = _lib.load()
    rows, N = shape
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(rows, N) == bwd_floats
    assert lib.pk_nll_err_partial_floats(rows) == nll_floats
    monkeypatch.setenv("PK_EXPERIMENT", "head_block=0, head_argmax=0")
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(rows, N) == bwd_floats


@pytest.mark.parametrize("rows", [1, 128, 64000])
@pytest.mark.parametrize("N", [2049, 3400, 8192])
def test_workspace_of_the_block_kernels(rows, N, monkeypatch):
    monkeypatch.delenv("PK_EXPERIMENT", raising=False)
    lib = _lib.load()
    ws = lib.pk_logsoftmax_bwd_bf16_partial_floats(rows, N)
    blocks = min(rows, BLOCK_CAP)  # a small batch: a block per row
    assert ws > 0
    assert ws >= blocks * N * 2
    assert ws % (N * 2) == 0 and ws // (N * 2) <= BLOCK_CAP
    ldb = F_._up(N, 64)
    if rows >= 4096:
        assert ws * 4 <= rows * ldb * 2   # no larger than the bf16 dz it accompanies


def test_head_block_lever_is_read_per_call(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("PK_EXPERIMENT", raising=False)
    wave = lib.pk_logsoftmax_bwd_bf16_partial_floats(64000, 1938)
    wide = lib.pk_logsoftmax_bwd_bf16_partial_floats(64000, 3400)
    monkeypatch.setenv("PK_EXPERIMENT", "head_block=1")
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(64000, 1938) == BLOCK_CAP * 1938 * 2 != wave
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(70, 48) == 70 * 48 * 2
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(64000, 3400) == wide
    monkeypatch.setenv("PK_EXPERIMENT", "head_argmax=0 , head_block = 1")
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(64000, 1938) == BLOCK_CAP * 1938 * 2
    monkeypatch.setenv("PK_EXPERIMENT", "head_block=0")
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(64000, 1938) == wave
    monkeypatch.delenv("PK_EXPERIMENT")
    assert lib.pk_logsoftmax_bwd_bf16_partial_floats(64000, 1938) == wave


def test_the_gate_of_the_fused_head():
    x = torch.zeros(4, 8)
    old = F_.settings.precision
    try:
        F_.set_precision("bf16")
        for N, ok in [(2048, True), (2049, True), (3400, True), (8192, True), (8193, False)]:
            assert F_.linear_log_softmax_ok(x, torch.empty(N, 8)) is ok, N
        assert not F_.linear_log_softmax_ok(torch.zeros(2, 4, 8), torch.empty(3400, 8))
        F_.set_precision("fp32")
        assert not F_.linear_log_softmax_ok(x, torch.empty(3400, 8))
    finally:
        F_.set_precision(old)
    assert "8192" in F_.linear_log_softmax_ok.__doc__
