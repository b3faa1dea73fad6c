"""The raw-audio front-end on the GPU: nn.logMelFb / functional.log_mel_fb (pk_logmel.hip) and functional.channel_average
against the float64 reference of logmel_ref.py.  Bound: norm-relative error 1e-4, the project's standing figure; the
float32 CPU evaluation of the same reference has to stay inside it too (a condition on the inputs: Gaussian noise plus one
sine keeps every mel energy far above fp32 rounding).  Each test prints what it measured."""
import functools
import importlib

import pytest
import torch

from golden_util import rel_err
from logmel_ref import chavg_ref, logmel_ref

pytestmark = pytest.mark.gpu
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
SR, TOL = 16000, 1e-4

# (ws, hop, n_mels, T, B).  The kernel's row tile is 16 sentences, or fewer sentences at several frames; a workgroup is
# (4 waves, 2 tiles each), (4, 1), (2, 1) or (1, 1), the largest that fits 64 KB of LDS and still gives 256 workgroups.
CASES = [
    (400, 160, 40, 400, 1),                    # one frame
    (400, 160, 40, 400 + 160 * 16 + 37, 3),    # ignored tail; 4 sentences x 4 frames per tile, one sentence masked
    (400, 160, 40, 400 + 160 * 64, 17),        # B over a tile edge
    (25, 10, 13, 95, 2),                       # odd ws, n_freq = 13
    (64, 64, 8, 64 * 5, 16),                   # no overlap
    (1024, 256, 128, 1024 + 256 * 3, 2),       # the coverage limits
    (4, 1, 1, 9, 1),                           # the smallest case
    (1024, 1024, 128, 2048, 16),               # the largest slab: 64 KB exactly
    (64, 32, 8, 64 + 32 * 1023, 32),           # 256 workgroups of (4, 2)
    (64, 32, 8, 64 + 32 * 599, 32),            # (4, 1)
    (64, 32, 8, 64 + 32 * 299, 32),            # (2, 1)
    (64, 32, 8, 64 + 32 * 4095, 8),            # (4, 2) with 8 sentences x 2 frames per tile
    (400, 160, 40, 400 + 160 * 1023, 32),      # the recipe's window at a filling size: (4, 1), since (4, 2) passes 64 KB
]


def opts(ws, hop, n_mels):
    return {"logmelfb_nr_sample_rate": str(SR), "logmelfb_nr_filt": str(n_mels), "logmelfb_stft_window_size": str(ws),
            "logmelfb_stft_window_shift": str(hop), "use_cuda": "True", "to_do": "forward"}


def audio(T, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64)[:, None]
    return (0.3 * torch.randn(T, B, generator=g) + 0.5 * torch.sin(2 * torch.pi * 440.0 / SR * t + torch.arange(B))).float()


@functools.lru_cache(maxsize=None)
def case(ws, hop, n_mels, T, B):
    x = audio(T, B)
    ref = logmel_ref(x, SR, ws, hop, n_mels)
    e32 = rel_err(logmel_ref(x, SR, ws, hop, n_mels, torch.float32), ref)
    assert e32 <= TOL, "the float32 CPU reference is %.2e off: the inputs are ill-conditioned" % e32
    return x, ref, e32


@pytest.mark.parametrize("ws,hop,n_mels,T,B", CASES)
def test_log_mel_fb(ws, hop, n_mels, T, B):
    x, ref, e32 = case(ws, hop, n_mels, T, B)
    net = nn_amd.logMelFb(opts(ws, hop, n_mels), 1).cuda()
    y = net(x.cuda().unsqueeze(-1))
    assert tuple(y.shape) == tuple(ref.shape) == (1 + (T - ws) // hop, B, n_mels)
    e = rel_err(y, ref)
    print("logmel %s: rel err %.2e (float32 on the CPU: %.2e)" % ((ws, hop, n_mels, T, B), e, e32))
    assert e <= TOL


def test_silent_sentence_gives_the_floor_and_leaves_the_others_alone():
    ws, hop, n_mels, T, B = 400, 160, 40, 400 + 160 * 20, 5
    net = nn_amd.logMelFb(opts(ws, hop, n_mels), 1).cuda()
    x = audio(T, B).cuda()
    y = net(x.unsqueeze(-1))
    x[:, 2] = 0.0
    y0 = net(x.unsqueeze(-1))
    print("silent sentence: max |y + 20| = %.2e" % float((y0[:, 2] + 20.0).abs().max()))
    assert float((y0[:, 2] + 20.0).abs().max()) <= 1e-5
    others = [0, 1, 3, 4]
    assert torch.equal(y0[:, others], y[:, others])


@pytest.mark.parametrize("N,C", [(1, 1), (7, 3), (1000, 6)])
def test_channel_average(N, C):
    g = torch.Generator().manual_seed(N)
    x, cot = torch.randn(N, C, generator=g), torch.randn(N, 1, generator=g)
    w = torch.rand(C, generator=g) + 0.1
    w = w / w.sum()
    leaf = x.cuda().requires_grad_()
    y = F_.channel_average(leaf, w.cuda())
    y.backward(cot.cuda())
    e_y, e_dx = rel_err(y, chavg_ref(x, w)), rel_err(leaf.grad, cot.double() * w.double())
    print("channel_average (%d, %d): y %.2e, dx %.2e" % (N, C, e_y, e_dx))
    assert tuple(y.shape) == (N, 1) and e_y <= 1e-6 and e_dx <= 1e-6


def test_six_microphones_through_both_classes():
    ws, hop, n_mels, T, B, C = 400, 160, 40, 400 + 160 * 30, 4, 6
    weights = [1.0, 2.0, 0.5, 1.0, 1.0, 3.0]
    x = torch.stack([audio(T, B, seed=c) for c in range(C)], dim=2)
    avg = nn_amd.channel_averaging({"chAvg_channelWeights": ",".join(map(str, weights)), "use_cuda": "True"}, C).cuda()
    mel = nn_amd.logMelFb(opts(ws, hop, n_mels), avg.out_dim).cuda()
    y = mel(avg(x.cuda()))
    mono = chavg_ref(x, torch.tensor(weights, dtype=torch.float64) / sum(weights))[..., 0]
    e = rel_err(y, logmel_ref(mono, SR, ws, hop, n_mels))
    print("channel_averaging -> logMelFb: rel err %.2e" % e)
    assert e <= TOL


def test_waveform_gradient_is_refused():
    net = nn_amd.logMelFb(opts(400, 160, 40), 1).cuda()
    with pytest.raises(_lib.PkError, match="forward only"):
        net(audio(800, 2).cuda().unsqueeze(-1).requires_grad_())
