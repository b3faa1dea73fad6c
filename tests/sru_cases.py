"""The scan cases of test_gpu_sru.py, built on the CPU so that test_sru_host.py can check their input conditions without a
GPU: inputs, the float64 reference's results and its min |c_t|.  ring_blocks() restates from csrc/pk_sru.hip which of a
thread's two block loops a walk of n steps enters."""
import functools
from typing import NamedTuple, Optional

import torch

from sru_ref import sru_scan_ref

SRU_P = 8        # steps of run-ahead per thread: the depth of the kernels' register ring
MIN_C = 1e-3     # relu / selu cases: every c_t of the reference is at least this far from the kink

# (T, B, D, H, k, act, mask_h, seed): T below, across and no multiple of the prefetch depth; 120 columns (one wave over the
# direction and the sentence boundary); odd H at the 12-byte pitch; an exact multiple of the wave.  k = 3 comes with a skip
# source except in the one-column case.  Seeds of the relu / selu cases: the reference has min |c_t| >= 1e-3.
SCAN = [(1, 1, 1, 1, 3, "none", False, 0), (3, 2, 2, 5, 4, "tanh", False, 1), (37, 3, 2, 20, 3, "relu", True, 122),
        (70, 2, 1, 67, 4, "selu", True, 11774), (130, 5, 2, 64, 3, "none", False, 4)]


class ScanCase(NamedTuple):
    T: int
    B: int
    D: int
    H: int
    k: int
    skip: Optional[bool]     # k = 3: with a skip source (None: the rule of SCAN)
    act: str
    mask_h: bool
    grads: Optional[str]     # which output gradients exist: "y", "ym" or "both"; None: no mask_next, so no Ym at all
    seed: int

    @property
    def id(self):
        return "T%d-k%d%s-%s-%s%s" % (self.T, self.k, "x" if self.skip else "", self.act, self.grads, "-mh" if self.mask_h else "")


def ring_blocks(n):
    """(unguarded, guarded) blocks of SRU_P steps in a walk of n steps, forward and backward alike: a block runs unguarded
    while all of its steps and all of the next block's exist - backward also reads c of the step behind those, which the
    same bound covers (s0 + 2 * SRU_P < n)."""
    full = len([s0 for s0 in range(0, n, SRU_P) if s0 + 2 * SRU_P < n])
    return full, len(range(0, n, SRU_P)) - full


# The register ring.  B = 3, D = 2, H = 20: 120 columns, a wave over the direction and the sentence boundary.
FORMS = [(4, False), (3, True), (3, False)]  # (k, skip source): the kernels' three (K, HASX) instances
RING = (
    # T = 41, four unguarded blocks and a guarded remainder of 8 + 1 steps: each form with each set of output gradients -
    # the nine instances of the backward kernel (dY only, dYm only - what a layer under a skip layer gets -, both)
    [ScanCase(41, 3, 2, 20, k, skip, "tanh" if k == 4 else "none", skip, g, 20 + i)
     for i, (k, skip) in enumerate(FORMS) for g in ("y", "ym", "both")]
    # every hand-over: T = 8 one guarded block, all of it from the prologue's loads; 9 a second one of one step; 16 two
    # whole guarded blocks; 17 the first unguarded block, then 8 + 1 guarded steps; 24 and 25 the same one block later.
    # At the last step backward's c_prev is the "no step behind" zero, which comes from the prologue for T <= 8, from a
    # guarded block for 9 .. 16 and from an unguarded block's hand-over beyond
    + [ScanCase(T, 3, 2, 20, 3, True, "tanh" if T % 2 else "none", True, "both", 30 + T) for T in (8, 9, 16, 17, 24, 25)]
    # the single unguarded block of the dYm-only instance
    + [ScanCase(17, 3, 2, 20, 4, False, "none", False, "ym", 60)]
    # the piecewise activations across an unguarded block: seeds with min |c_t| >= MIN_C in the reference
    + [ScanCase(25, 3, 2, 20, 3, True, "relu", True, "both", 52), ScanCase(25, 3, 2, 20, 4, False, "selu", False, "both", 0)]
)

# Sentence lengths at the function (forward only): 266 columns, so one wave holds sentences of different lengths; 41 against
# 40 and 17 against 16 put lanes of one wave into different loops at the same step
LENS = (41, 40, 25, 17, 16, 9, 1)
LENS_CASES = [ScanCase(41, 7, 2, 19, k, skip, "tanh", True, "both", 70 + i) for i, (k, skip) in enumerate(FORMS)]
# lengths that functional.sentence_lengths refuses, handed to pk_sru_fwd directly: clamped into 0 .. T by the kernel
CLAMP_LENS = (0, 25, -3, 7)
CLAMP_CASE = ScanCase(20, 4, 2, 5, 3, False, "tanh", False, None, 80)


def scan_inputs(case):
    """U, x_skip, weight_c, bias, mask_h, the cotangent of Y, mask_next and the cotangent of Ym (None where the case has none)."""
    T, B, D, H, k = case[:5]
    g = torch.Generator().manual_seed(case.seed)
    out = D * H
    U = torch.randn(T, B, out * k, generator=g)
    skip = (k == 3 and out > 1) if case.skip is None else case.skip
    x = torch.randn(T, B, out, generator=g) if skip else None
    wc = torch.rand(2 * out, generator=g) * 2 - 1
    bias = torch.cat([0.5 * torch.randn(out, generator=g), -torch.ones(out)])
    mh = (torch.rand(B, out, generator=g) > 0.3).float() / 0.7 if case.mask_h else None
    cot = torch.randn(T, B, out, generator=g)
    mn, cotm = None, None
    if case.grads is not None:
        mn, cotm = (torch.rand(B, out, generator=g) > 0.3).float() / 0.7, torch.randn(T, B, out, generator=g)
    return U, x, wc, bias, mh, cot, mn, cotm


def leaves(ts, dev, dtype):
    return [None if t is None else t.to(device=dev, dtype=dtype).requires_grad_() for t in ts]


def scan_loss(case, y, ym, cot, cotm):
    """(Y * cotY).sum(), (Ym * cotM).sum() or their sum: the gradients that case.grads names."""
    of_y, of_ym = case.grads in (None, "y", "both"), case.grads in ("ym", "both")
    return sum(([(y * cot).sum()] if of_y else []) + ([(ym * cotm).sum()] if of_ym else []))


@functools.lru_cache(maxsize=None)
def scan_reference(case):
    """Y, Ym = Y * mask_next, dU, dweight_c, dbias, dx_skip of the float64 reference (those the case has) and its min |c_t|."""
    U, x, wc, bias, mh, cot, mn, cotm = (None if t is None else t.double() for t in scan_inputs(case))
    rU, rx, rwc, rb = leaves((U, x, wc, bias), "cpu", torch.float64)
    cs = []
    y = sru_scan_ref(rU, rx, rwc, rb, 1.3, case.act, case.D, mh, cs)
    ym = None if mn is None else y * mn
    scan_loss(case, y, ym, cot, cotm).backward()
    ref = {"Y": y.detach(), "dU": rU.grad, "dweight_c": rwc.grad, "dbias": rb.grad}
    if ym is not None:
        ref["Ym"] = ym.detach()
    if x is not None:
        ref["dx_skip"] = rx.grad
    return ref, float(torch.stack(cs).detach().abs().min())
