"""Generate tests/golden/e2e_quat_linear_ref.npz from a checkout of the reference (PyTorch-Kaldi).

    python tools/make_golden_quat_linear.py /path/to/pytorch-kaldi

TEST INFRASTRUCTURE ONLY, never run by a test.  Imports the reference's ``quaternion_neural_networks.py`` unmodified and
runs its two linear classes on the CPU in fp32.  ONE fixture, data only:

  init/<Class>/<weight_init>/<criterion>/<parameter>   the state dict right after ``np.random.seed(SEED)`` and construction
                                                       at in, out = 20, 12, for every initialiser and criterion the class
                                                       accepts (QuaternionLinear: quaternion, unitary; the Autograd form
                                                       also random; glorot and he)
  sd/<parameter>, x, y, cot, dx, grad/<parameter>      QuaternionLinear (quaternion, glorot, bias perturbed): a [T, B, 20]
                                                       input, the output, a cotangent and every gradient of the
                                                       reference's forward and hand-written backward

The name starts with ``e2e_`` so that the tests which take every other ``tests/golden/*.npz`` as a module case of
``neural_networks.py`` leave it alone.
"""
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
SEED, IN, OUTF, T, B = 5150, 20, 12, 3, 5
INITS = {"QuaternionLinear": ("quaternion", "unitary"), "QuaternionLinearAutograd": ("quaternion", "unitary", "random")}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import quaternion_neural_networks as qnn

    torch.set_num_threads(1)
    arrays = {}
    for cls, inits in INITS.items():
        for winit in inits:
            for crit in ("glorot", "he"):
                np.random.seed(SEED)
                net = getattr(qnn, cls)(IN, OUTF, bias=True, init_criterion=crit, weight_init=winit)
                for k, v in net.state_dict().items():
                    arrays["init/%s/%s/%s/%s" % (cls, winit, crit, k)] = v.clone()
    np.random.seed(SEED)
    net = qnn.QuaternionLinear(IN, OUTF)
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        net.bias.add_(0.1 * torch.randn(net.bias.shape, generator=g))  # (the initialiser leaves it zero)
    arrays.update({"sd/" + k: v.clone() for k, v in net.state_dict().items()})
    x = torch.randn(T, B, IN, generator=g).requires_grad_(True)
    y = net(x)
    cot = torch.randn(y.shape, generator=g)
    (y * cot).sum().backward()
    arrays.update({"x": x, "y": y, "cot": cot, "dx": x.grad})
    for k, p in net.named_parameters():
        arrays["grad/" + k] = p.grad
    meta = {"seed": SEED, "in": IN, "out": OUTF, "T": T, "B": B, "inits": {k: list(v) for k, v in INITS.items()},
            "criteria": ["glorot", "he"], "torch": torch.__version__, "numpy": np.__version__}
    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT, "e2e_quat_linear_ref.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
