"""nn.SincConv_fast without a GPU: the float64 restatement of sincfast_ref.py against the fixtures dumped from the reference
class (tools/make_golden_sincfast.py) - which validates the yardstick of the GPU test -, the class's parameters and tensors
against the same fixtures, and its refusals.  Bound: 1e-4 norm-relative, the project's parity bar, for fp32 results of the
reference against their float64 restatement; each figure is printed."""
import importlib

import pytest
import torch

import sincfast_ref
from golden_util import Golden, list_cases, rel_err

nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
CASES = list_cases("e2e_sincfast_")
TOL = 1e-4


def conv_args(net):
    return dict(stride=net.stride, padding=net.padding, dilation=net.dilation, sample_rate=net.sample_rate,
                min_low_hz=net.min_low_hz, min_band_hz=net.min_band_hz)


def test_three_fixtures():
    assert len(CASES) == 3


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    g = Golden(case)
    net = nn_amd.SincConv_fast(**g.meta["ctor"])
    got = sincfast_ref.run(g.t("x"), g.t("sd/low_hz_"), g.t("sd/band_hz_"), g.t("n_"), g.t("window_"), g.t("dy"), torch.float64,
                           **conv_args(net))
    for k in ("filters", "y", "dx", "dlow", "dband"):
        e = rel_err(g.t(k), got[k])
        print("%s %s: reference fp32 vs float64 restatement %.3e" % (case, k, e))
        assert e < TOL, (case, k, e)
    assert float(got["dband"][-1]) == 0.0 and float(g.t("dband")[-1]) == 0.0  # high clamps at sr/2


@pytest.mark.parametrize("case", CASES)
def test_class_matches_the_reference_layout(case):
    g = Golden(case)
    net = nn_amd.SincConv_fast(**g.meta["ctor"])
    assert net.kernel_size == g.meta["kernel_size"] and net.kernel_size % 2 == 1
    sd, init = net.state_dict(), g.group("init/")
    assert list(sd) == list(init) == ["low_hz_", "band_hz_"]
    for k, v in init.items():
        assert tuple(sd[k].shape) == tuple(v.shape) == (net.out_channels, 1) and torch.equal(sd[k], v), (case, k)
    n_, window_ = sincfast_ref.buffers(net.kernel_size, net.sample_rate)
    for name, mine, ref in (("n_", net.n_, n_), ("window_", net.window_, window_)):
        assert mine.shape == g.t(name).shape and torch.equal(mine, g.t(name)) and torch.equal(ref, g.t(name)), (case, name)
    with pytest.raises(AttributeError):
        net.filters  # exists after a forward only, as in the reference


def test_refusals():
    for kw in (dict(in_channels=2), dict(bias=True), dict(groups=2)):
        with pytest.raises(ValueError):
            nn_amd.SincConv_fast(**dict(dict(in_channels=1, out_channels=4, kernel_size=9), **kw))
    with pytest.raises(_lib.PkError):
        nn_amd.SincConv_fast(1, 4, 9)(torch.randn(2, 1, 50))


def test_argument_errors_return_codes():
    lib = _lib.load()
    for args, word in (((2, 10, 4, 9, 1, 0, 2), b"no output position"), ((2, 50, 4, 8, 1, 0, 1), b"K = 8"), ((2, 50, 4, 1, 1, 0, 1), b"K = 1"),
                       ((2, 50, 4, 9, 0, 0, 1), b"stride 0"), ((2, 50, 4, 9, 1, 0, 0), b"dilation 0"),
                       ((2, 50, 4, 9, 1, -1, 1), b"padding -1"), ((2, 50, 0, 9, 1, 0, 1), b"C = 0"),
                       ((1, 40000, 4, 32769, 1, 0, 1), b"65536 bytes")):  # (the window of one position alone is 128 KB)
        assert lib.pk_sincfast_fwd(None, None, None, *args, None) == 2 and word in lib.pk_last_error(), (args, lib.pk_last_error())
        assert lib.pk_sincfast_bwd(None, *[None] * 7, *args, 16000.0, 50.0, 50.0, None, None, None, None) == 2, args
        assert lib.pk_sincfast_partial_floats(*args) == 0
    assert lib.pk_sincfast_work_floats(17, 33) == 3 * 16 * 8 and lib.pk_sincfast_partial_floats(2, 1500, 17, 33, 1, 0, 1) > 0
