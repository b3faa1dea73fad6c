"""Float64 reference of the raw-audio front-end (neural_networks.py:658-717) from torch.stft and the filterbank formula
of torchaudio's melscale_fbanks (f_min = 0, f_max = sr // 2, htk scale, no normalisation).  dtype=torch.float32 evaluates
the same expressions in float32 on the CPU."""
import math

import torch


def mel_fb_ref(sr, n_freq, n_mels):
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)  # noqa: E731
    all_freqs = torch.linspace(0, sr // 2, n_freq, dtype=torch.float64)
    m_pts = torch.linspace(mel(0.0), mel(float(sr // 2)), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    fb = torch.zeros(n_freq, n_mels, dtype=torch.float64)
    for j in range(n_mels):
        up = (all_freqs - f_pts[j]) / (f_pts[j + 1] - f_pts[j])
        down = (f_pts[j + 2] - all_freqs) / (f_pts[j + 2] - f_pts[j + 1])
        fb[:, j] = torch.clamp(torch.min(up, down), min=0.0)
    return fb


def logmel_ref(x, sr, ws, hop, n_mels, dtype=torch.float64):
    """x [T, B] -> [frames, B, n_mels]"""
    spec = torch.stft(x.to(dtype).T, ws, hop, ws, window=torch.hann_window(ws, dtype=dtype), center=False, return_complex=True)
    power = spec.abs() ** 2  # [B, n_freq, frames]
    mel = power.transpose(1, 2) @ mel_fb_ref(sr, ws // 2 + 1, n_mels).to(dtype)
    return torch.log10(mel.clamp(min=1e-20)).transpose(0, 1)


def chavg_ref(x, w):
    return torch.einsum("...c,c->...", x.double(), w.double()).unsqueeze(-1)
