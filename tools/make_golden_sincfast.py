"""Generate the SincConv_fast fixtures of tests/golden/ from a checkout of the reference (PyTorch-Kaldi).

    python tools/make_golden_sincfast.py /path/to/pytorch-kaldi

TEST INFRASTRUCTURE ONLY, never run by a test.  Imports the reference's ``neural_networks.py`` unmodified, builds its
``SincConv_fast`` with the constructor arguments below, runs forward and backward in fp32 on the CPU on seeded inputs and
stores: the constructor arguments (meta), the initial parameters (init/...), the parameters of the run (sd/...: the initial
ones with low_hz_[0] negated and band_hz_[-1] = sample_rate, so that |.| and the clamp at sr/2 are exercised), n_, window_,
filters, x, y, dy and the gradients dx, dlow, dband.

  e2e_sincfast_plain     C 6, K 17, stride 1, padding 0, dilation 1, B 2, n 120
  e2e_sincfast_stride    C 5, K 12 (even: the layer makes it 13), stride 2, padding 6, dilation 1, B 2, n 151
  e2e_sincfast_dilated   C 4, K 9, stride 3, padding 4, dilation 2, B 3, n 97, sample_rate 8000, min_low_hz 40, min_band_hz 30

The names start with ``e2e_`` so that the tests which take every other ``tests/golden/*.npz`` as a module case of
``neural_networks.py`` leave them alone.
"""
import os
import sys

sys.dont_write_bytecode = True

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_cudnn import _import_reference, _save  # noqa: E402

CASES = {
    "e2e_sincfast_plain": (dict(in_channels=1, out_channels=6, kernel_size=17), 2, 120),
    "e2e_sincfast_stride": (dict(in_channels=1, out_channels=5, kernel_size=12, stride=2, padding=6), 2, 151),
    "e2e_sincfast_dilated": (dict(in_channels=1, out_channels=4, kernel_size=9, stride=3, padding=4, dilation=2,
                                  sample_rate=8000, min_low_hz=40, min_band_hz=30), 3, 97),
}


def case(ref, name, ctor, B, n, seed):
    torch.manual_seed(seed)
    net = ref.SincConv_fast(**ctor)
    arrays = {"init/" + k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        net.low_hz_[0] = -net.low_hz_[0]
        net.band_hz_[-1] = float(net.sample_rate)
    arrays.update({"sd/" + k: v.clone() for k, v in net.state_dict().items()})
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 1, n, generator=g).requires_grad_(True)
    y = net(x)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    arrays.update({"n_": net.n_, "window_": net.window_, "filters": net.filters, "x": x, "y": y, "dy": dy, "dx": x.grad,
                   "dlow": net.low_hz_.grad, "dband": net.band_hz_.grad})
    _save(name, {"ctor": ctor, "kernel_size": net.kernel_size, "B": B, "n": n, "seed": seed, "n_masks": 0}, arrays)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = _import_reference(sys.argv[1])
    torch.set_num_threads(1)
    for i, (name, (ctor, B, n)) in enumerate(CASES.items()):
        case(ref, name, ctor, B, n, 6101 + 101 * i)


if __name__ == "__main__":
    main()
