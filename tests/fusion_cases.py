"""The projection cases of test_gpu_fusion.py, built on the CPU so that test_fusion_host.py can check their input conditions
without a GPU: inputs, the float64 reference's results, d0 (bf16 mode), the distance of the reference's pre-activations from
the kink, and - on the shapes that are too large for any seed to keep all of them away from it - the cotangent zeroed there.
geometry() restates the host arithmetic of csrc/pk_fusion.hip (fus_geom, fus_ws, FUS_DISPATCH) that the case comments name."""
import functools
from typing import NamedTuple, Optional

import torch

from fusion_ref import fusion_proj_ref
from golden_util import rel_err

KINK = 1e-5          # every piecewise-linear pre-activation of the reference is at least this far from zero ...
ZEROED_MAX = 1e-4    # ... or, on the WALKS shapes, sits under a zero of the cotangent: at most this share of dP's entries

# (N, M, F, H0) -> seed.  Tiles are 64 rows x 64 columns of the 2*H0 stacked ones, K steps of 16: below one tile both ways;
# rows and columns across tiles with a remainder, F below one K step, M = 1; F = 40 (three K steps in the four-step kernel).
SHAPES = {(21, 6, 13, 20): 0, (150, 1, 5, 72): 0, (130, 2, 40, 136): 0}

# One shape per path of the dispatch that SHAPES does not enter (NKS: the kernel instance, nks = roundup(F, 16) / 16 the K
# steps it runs; width = M * roundup(F, 16), the staged values per row; the weight-gradient kernel has
# walkers = min(64, ceil(512 / column tiles), row tiles) workgroups per column tile, each walking row tiles w, w + walkers, ..)
WALKS = {
    # NKS = 2; 129 row tiles on 64 walkers: workgroup 0 walks three tiles, the others two, and the last tile has 37 rows
    (8229, 2, 24, 20): 0,
    # 580 columns = 10 column tiles, so 52 walkers for 66 row tiles: the limit that the column tiles set, a ragged walk
    # (14 workgroups walk two tiles, the last tile has 40 rows) and slope partials from 10 column tiles
    (4200, 1, 5, 290): 0,
}
PATHS = {
    **WALKS,
    (70, 1, 64, 40): 0,     # nks == NKS == 4: the four-step kernel with every step live
    (300, 1, 128, 8): 0,    # NKS = 8 with all eight steps: F at its limit
    (200, 3, 70, 24): 3,    # nks = 5 inside NKS = 8 (three steps switched off); width 240, the fp32 LDS limit exactly
    (100, 6, 80, 12): 0,    # width 480, the bf16 LDS limit exactly: bf16 mode only, fp32 mode refuses it
}
SEEDS = {**SHAPES, **PATHS}

# what geometry() must give for the shapes above: the paths their comments claim
EXPECT = {
    (8229, 2, 24, 20): dict(nks=2, NKS=2, width=64, ctiles=1, rtiles=129, walkers=64, last_rows=37),
    (4200, 1, 5, 290): dict(nks=1, NKS=1, width=16, ctiles=10, rtiles=66, walkers=52, last_rows=40),
    (70, 1, 64, 40): dict(nks=4, NKS=4, width=64, ctiles=2, rtiles=2, walkers=2, last_rows=6),
    (300, 1, 128, 8): dict(nks=8, NKS=8, width=128, ctiles=1, rtiles=5, walkers=5, last_rows=44),
    (200, 3, 70, 24): dict(nks=5, NKS=8, width=240, ctiles=1, rtiles=4, walkers=4, last_rows=8),
    (100, 6, 80, 12): dict(nks=5, NKS=8, width=480, ctiles=1, rtiles=2, walkers=2, last_rows=36),
}
MAX_F, MAX_WIDTH = 128, {True: 480, False: 240}  # bf16 mode: True

# refused before anything is launched: (shape, bf16 mode, words of the message)
REFUSED = [((4, 1, 129, 4), False, "at most 128"), ((4, 1, 129, 4), True, "at most 128"),
           ((4, 31, 16, 4), True, "staged values per row"), ((4, 16, 16, 4), False, "staged values per row"),
           ((100, 6, 80, 12), False, "staged values per row")]


def path_cases():
    """(shape, act, reduce, bf) of every new case: two activation / reduction pairs on each shape, all four activations on
    the first; both precision modes wherever both accept the shape."""
    out = []
    for i, shape in enumerate(PATHS):
        acts = [("prelu", "sum"), ("tanh", "mean")] + ([("relu", "mean"), ("leaky_relu", "sum")] if i == 0 else [])
        out += [(shape, a, r, bf) for a, r in acts for bf in (False, True) if geometry(shape)["width"] <= MAX_WIDTH[bf]]
    return out


def geometry(shape):
    N, M, F, H0 = shape
    nks = -(-F // 16)
    ctiles, rtiles = -(-2 * H0 // 64), -(-N // 64)
    return dict(nks=nks, NKS=next(n for n in (1, 2, 4, 8, None) if n is None or nks <= n), width=M * nks * 16, ctiles=ctiles,
                rtiles=rtiles, walkers=min(64, -(-512 // ctiles), rtiles), last_rows=N - 64 * (rtiles - 1))


def ws_parts(lib, shape):
    """The wave partials (four per walking workgroup) behind the library's own workspace size:
    pk_fusion_ws_floats = parts * (C * Kp + C + 2 * column tiles)."""
    N, M, F, H0 = shape
    g = geometry(shape)
    per_part = 2 * H0 * g["nks"] * 16 + 2 * H0 + 2 * g["ctiles"]
    total = int(lib.pk_fusion_ws_floats(N, M, F, H0))
    assert total > 0 and total % per_part == 0, (total, per_part)
    return total // per_part


class ProjCase(NamedTuple):
    inputs: tuple            # x, W, b, slope, cot (float32, on the CPU)
    ref: dict                # the float64 reference's P, dx, dW, db (, dslope)
    d0: Optional[dict]       # bf16 mode: the reference's distance from itself under a relative 2^-24 move of x
    kink: float              # min |pre-activation| of the reference
    zeroed: float            # share of the cotangent's entries set to zero (WALKS shapes, piecewise-linear activations)


@functools.lru_cache(maxsize=None)
def proj_case(shape, act, reduce, bf):
    """One projection case; the reference runs once per case."""
    N, M, F, H0 = shape
    g = torch.Generator().manual_seed(SEEDS[shape])
    x, W = torch.randn(N, M * F, generator=g), torch.randn(2 * H0, F, generator=g) / F ** 0.5
    b, slope = 0.3 * torch.randn(2 * H0, generator=g), torch.tensor([0.25, 0.1]) if act == "prelu" else None
    cot = torch.randn(N, 2 * H0, generator=g)
    eps = torch.randint(0, 2, x.shape, generator=g).double() * 2 - 1

    def run(xin):
        leaves = [None if t is None else t.double().requires_grad_() for t in (xin, W, b, slope)]
        pres = []
        P = fusion_proj_ref(*leaves, M, act, reduce, bf, pres)
        (P * cot.double()).sum().backward()
        out = {"P": P.detach(), "dx": leaves[0].grad, "dW": leaves[1].grad, "db": leaves[2].grad}
        if slope is not None:
            out["dslope"] = leaves[3].grad
        return out, pres[0]

    zeroed = 0.0
    if shape in WALKS and act != "tanh":
        # Thousands of rows: no seed keeps every pre-activation KINK away from zero.  dP[n, c] = 0 wherever a microphone's
        # pre-activation of (n, c) is closer: every gradient reaches that sign through dP[n, c] only, and P is continuous.
        near = (run_pre(x, W, b, slope, M, act, reduce, bf).abs() < KINK).any(1)
        cot = cot.masked_fill(near, 0.0)
        zeroed = float(near.double().mean())
    ref, pre = run(x)
    d0 = None
    if bf:
        pert = run(x.double() * (1 + 2.0 ** -24 * eps))[0]
        d0 = {n: rel_err(pert[n], ref[n]) for n in ref}
    return ProjCase((x, W, b, slope, cot), ref, d0, float(pre.abs().min()), zeroed)


def run_pre(x, W, b, slope, M, act, reduce, bf):
    """The reference's pre-activations [N, M, 2*H0] alone."""
    pres = []
    fusion_proj_ref(*(None if t is None else t.double() for t in (x, W, b, slope)), M, act, reduce, bf, pres)
    return pres[0]
