"""SincConv_fast restated in plain torch from its formulas; autograd differentiates it.  The arithmetic runs in the dtype of
the arguments: float64 is the yardstick of the sincfast tests, float32 on the CPU is the stock evaluation whose distance
from it sets their bars."""
import math

import torch
import torch.nn.functional as F


def buffers(K, sample_rate):
    """(n_ [1, h], window_ [h]) of a layer with K (odd) taps, in float32 as the layer keeps them.  The half window's
    abscissae are linspace(0, K/2 - 1, int(K/2)) - K/2 a float, so the step is not 1."""
    n_lin = torch.linspace(0, (K / 2) - 1, steps=int(K / 2))
    window_ = 0.54 - 0.46 * torch.cos(2 * math.pi * n_lin / K)
    n_ = 2 * math.pi * torch.arange(-(K - 1) / 2.0, 0).view(1, -1) / sample_rate
    return n_, window_


def sinc_conv_fast(x, low_hz_, band_hz_, n_, window_, stride, padding, dilation, sample_rate, min_low_hz, min_band_hz):
    """x [B, 1, n], low_hz_ / band_hz_ [C, 1], n_ [1, h], window_ [h] -> (y [B, C, L_out], filters [C, 1, 2h + 1])."""
    low = min_low_hz + low_hz_.abs()
    high = torch.clamp(low + min_band_hz + band_hz_.abs(), min_low_hz, sample_rate / 2)
    band = high - low  # [C, 1]
    left = (torch.sin(high * n_) - torch.sin(low * n_)) / (n_ / 2) * window_ / (2 * band)
    filters = torch.cat([left, torch.ones_like(band), left.flip(1)], dim=1).unsqueeze(1)
    return F.conv1d(x, filters, stride=stride, padding=padding, dilation=dilation), filters


def run(x, low_hz_, band_hz_, n_, window_, dy, dtype, **kw):
    """Forward and backward in `dtype` on the CPU -> {"y", "filters", "dx", "dlow", "dband"}."""
    x, lo, ba = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (x, low_hz_, band_hz_))
    y, filters = sinc_conv_fast(x, lo, ba, n_.detach().cpu().to(dtype), window_.detach().cpu().to(dtype), **kw)
    y.backward(dy.detach().cpu().to(dtype))
    return {"y": y.detach(), "filters": filters.detach(), "dx": x.grad, "dlow": lo.grad, "dband": ba.grad}
