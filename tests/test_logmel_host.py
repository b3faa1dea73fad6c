"""nn.logMelFb and nn.channel_averaging without a GPU: construction from the reference's option names, out_dim, the empty
state dict, the filterbank against its float64 formula, the refusals of the classes and of the C entries."""
import importlib

import numpy as np
import pytest
import torch

from logmel_ref import mel_fb_ref

nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
OPTS = {"logmelfb_nr_sample_rate": "16000", "logmelfb_nr_filt": "40", "logmelfb_stft_window_size": "400",
        "logmelfb_stft_window_shift": "160", "use_cuda": "True", "to_do": "train"}
WEIGHTS = [1.0, 2.0, 0.5, 1.0, 1.0, 3.0]


def test_logmelfb_construction_and_filterbank():
    net = nn_amd.logMelFb(OPTS, 1)
    assert net.out_dim == 40 and len(net.state_dict()) == 0 and list(net.parameters()) == []
    assert net.pk_flat_groups() == [] and net.pk_unused_parameters() == []
    fb, ref = net.fb.double(), mel_fb_ref(16000, 201, 40)
    assert tuple(fb.shape) == (201, 40) and float(fb.min()) >= 0.0 and bool((fb.max(0).values > 0).all())
    assert float((fb - ref).abs().max()) <= 1e-7
    assert tuple(net.basis.shape) == (400, 13 * 32)
    n, f = 37, 150  # one entry of the basis against its definition: frequency 150 = tile 9, lane 6
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / 400)
    want = torch.tensor([w * np.cos(2 * np.pi * f * n / 400), -w * np.sin(2 * np.pi * f * n / 400)])
    assert float((net.basis[n, 9 * 32 + 12:9 * 32 + 14].double() - want).abs().max()) <= 1e-7
    assert float(net.basis[:, 12 * 32 + 2 * 9:].abs().max()) == 0.0  # frequencies 201 .. 207 of the last tile


def test_channel_averaging_construction():
    net = nn_amd.channel_averaging({"chAvg_channelWeights": ",".join(map(str, WEIGHTS)), "use_cuda": "True"}, 6)
    assert net.out_dim == 1 and len(net.state_dict()) == 0
    assert net.pk_flat_groups() == [] and net.pk_unused_parameters() == []
    want = np.asarray(WEIGHTS, np.float32) / np.float32(sum(WEIGHTS))
    assert net._weights.dtype == torch.float32 and np.array_equal(net._weights.numpy(), want)


def test_refusals():
    mel = nn_amd.logMelFb(OPTS, 1)
    avg = nn_amd.channel_averaging({"chAvg_channelWeights": "1,1", "use_cuda": "True"}, 2)
    with pytest.raises(_lib.PkError, match="GPU only"):
        mel(torch.randn(800, 2, 1))
    with pytest.raises(_lib.PkError, match="Multi channel time signal"):
        mel(torch.randn(800, 2, 2))
    with pytest.raises(_lib.PkError, match="GPU only"):
        avg(torch.randn(5, 2, 2))
    with pytest.raises(_lib.PkError, match="channel weights"):
        avg(torch.randn(5, 2, 3))
    with pytest.raises(_lib.PkError, match="logmelfb_"):
        nn_amd.logMelFb(dict(OPTS, logmelfb_stft_window_size="2048"), 1)


@pytest.mark.parametrize("T,ws,hop,n_mels", [(4000, 400, 401, 40), (4000, 1025, 160, 40), (4000, 400, 160, 129), (399, 400, 160, 40)])
def test_c_entry_refuses_bad_geometry_without_a_gpu(T, ws, hop, n_mels):
    lib = _lib.load()
    assert lib.pk_logmel_fwd(None, None, None, None, T, 2, ws, hop, n_mels, None) != 0
    assert b"pk_logmel_fwd" in lib.pk_last_error()
    assert lib.pk_chavg_fwd(None, None, None, 10, 0, None) != 0 and lib.pk_chavg_bwd(None, None, None, 0, 3, None) != 0
