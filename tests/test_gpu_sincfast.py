"""nn.SincConv_fast on the GPU (pk_sincfast.hip) against the float64 restatement of sincfast_ref.py: output, both parameter
gradients and the input gradient, graded with golden_util.rel_err.

Bar per quantity: 1e-4, the project's parity bar, or 4 x the distance that the SAME formula evaluated by stock torch in
float32 on the CPU has from the float64 restatement on the case's inputs, whichever is larger.  The factor 4 allows for a
different summation order over up to B * L_out terms; the second term exists because dlow / dband are sums with
cancellation whose float32 floor is a property of the inputs.  Every test prints both distances."""
import importlib

import pytest
import torch

import sincfast_ref
from golden_util import Golden, list_cases, rel_err

pytestmark = pytest.mark.gpu
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
SR = 16000
KEYS = ("y", "dlow", "dband", "dx")

# (C, K, stride, padding, dilation, B, n)
CASES = [
    (5, 9, 1, 0, 1, 2, 70),         # the smallest; C below a channel tile
    (17, 33, 1, 0, 1, 2, 1500),     # crosses position tiles, ragged channel tile
    (16, 10, 2, 5, 1, 2, 301),      # even K -> 11, stride and padding
    (7, 15, 3, 4, 2, 2, 257),       # dilation, stride and padding together
    (80, 251, 1, 0, 1, 3, 3200),    # the recipe's bank
]


def gpu_run(net, x, dy):
    net = net.cuda()
    out = []
    for _ in range(2):  # twice: the results must be bit-identical (fixed-order reductions, no atomics)
        for p in net.parameters():
            p.grad = None
        xg = x.cuda().requires_grad_(True)
        y = net(xg)
        y.backward(dy.cuda())
        out.append({"y": y.detach(), "dlow": net.low_hz_.grad, "dband": net.band_hz_.grad, "dx": xg.grad})
    for k in KEYS:
        assert torch.equal(out[0][k], out[1][k]), k + " differs between two runs"
    return out[1]


def grade(tag, net, x, dy, got, stock32=None):
    args = (x, net.low_hz_, net.band_hz_, net.n_, net.window_, dy)
    kw = dict(stride=net.stride, padding=net.padding, dilation=net.dilation, sample_rate=net.sample_rate,
              min_low_hz=net.min_low_hz, min_band_hz=net.min_band_hz)
    ref = sincfast_ref.run(*args, torch.float64, **kw)
    stock32 = sincfast_ref.run(*args, torch.float32, **kw) if stock32 is None else stock32
    assert tuple(got["y"].shape) == tuple(ref["y"].shape)
    errs = {k: (rel_err(got[k], ref[k]), rel_err(stock32[k], ref[k])) for k in KEYS}
    for k, (e, floor) in errs.items():
        print("%s %s: kernel %.3e, stock fp32 %.3e" % (tag, k, e, floor))
    for k, (e, floor) in errs.items():
        assert e <= max(1e-4, 4.0 * floor), (tag, k, e, floor)
    assert float(got["dband"][-1]) == 0.0  # high clamps at sr/2: no gradient passes
    assert rel_err(net.filters, ref["filters"]) <= 1e-4 and tuple(net.filters.shape) == (net.out_channels, 1, net.kernel_size)


@pytest.mark.parametrize("C,K,s,p,d,B,n", CASES)
def test_against_float64(C, K, s, p, d, B, n):
    net = nn_amd.SincConv_fast(1, C, K, stride=s, padding=p, dilation=d, sample_rate=SR)
    with torch.no_grad():
        net.low_hz_[0] = -net.low_hz_[0]  # |.|
        net.band_hz_[-1] = float(SR)      # high clamps at sr/2
    g = torch.Generator().manual_seed(C * 1000 + K)
    x = torch.randn(B, 1, n, generator=g)
    L_out = (n + 2 * p - d * (net.kernel_size - 1) - 1) // s + 1
    dy = torch.randn(B, C, L_out, generator=g)
    grade(str((C, K, s, p, d, B, n)), net, x, dy, gpu_run(net, x, dy))


def test_fixtures_through_the_class():
    for case in list_cases("e2e_sincfast_"):
        g = Golden(case)
        net = nn_amd.SincConv_fast(**g.meta["ctor"])
        net.load_state_dict(g.group("sd/"))
        got = gpu_run(net, g.t("x"), g.t("dy"))
        grade(case, net, g.t("x"), g.t("dy"), got, stock32={k: g.t(k) for k in KEYS})
