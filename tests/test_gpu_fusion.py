"""The fusion layer on the GPU: functional.fusion_proj and nn.fusionRNN_jit against the float64 reference of fusion_ref.py.
fp32 mode: norm-relative error below 1e-4.  bf16 mode: against the same reference with its GEMM operands rounded to bf16,
err < max(1e-4, 2 * d0), d0 = that reference's distance from itself when x moves by a relative 2^-24 in front of the rounding
(the rule of test_gpu_sru.py).  Seeds are chosen so that no piecewise-linear pre-activation of the reference lies within 1e-5
of its kink; on the two shapes of thousands of rows, where no seed can, the cotangent is zero at those entries instead
(fusion_cases.py builds every case and test_fusion_host.py checks these conditions on the CPU).  Each test prints what it
measured."""
import functools
import importlib

import pytest
import torch

from fusion_cases import KINK, REFUSED, SHAPES, WALKS, ZEROED_MAX, geometry, path_cases, proj_case, ws_parts
from fusion_ref import fusion_rnn_ref
from golden_util import rel_err

pytestmark = pytest.mark.gpu
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
TOL = 1e-4


def graded(got, ref, d0):
    errs = {n: rel_err(got[n], ref[n]) for n in ref}
    print({n: "%.2e" % e + (" (d0 %.2e)" % d0[n] if d0 else "") for n, e in errs.items()})
    for n, e in errs.items():
        assert e < (max(TOL, 2 * d0[n]) if d0 else TOL), (n, e, d0 and d0[n])


def run_proj(inputs, M, act, reduce, bf, need_dx=True):
    x, W, b, slope, cot = (None if t is None else t.cuda() for t in inputs)
    leaves = [None if t is None else t.requires_grad_() for t in (W, b, slope)]
    F_.set_precision("bf16" if bf else "fp32")
    try:
        P = F_.fusion_proj(x.requires_grad_(need_dx), *leaves, M, act, reduce)
        (P * cot).sum().backward()
    finally:
        F_.set_precision("fp32")
    out = {"P": P.detach(), "dx": x.grad, "dW": leaves[0].grad, "db": leaves[1].grad}
    if slope is not None:
        out["dslope"] = leaves[2].grad
    return out


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("act", ["relu", "leaky_relu", "prelu", "tanh"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_projection_matches_reference(shape, act, reduce, bf):
    case = proj_case(shape, act, reduce, bf)
    if act != "tanh":
        assert case.kink >= KINK, case.kink
    graded(run_proj(case.inputs, shape[1], act, reduce, bf), case.ref, case.d0)


@pytest.mark.parametrize("shape,act,reduce,bf", path_cases(),
                         ids=["%s-%s-%s-%s" % ("x".join(map(str, s)), a, r, "bf16" if bf else "fp32") for s, a, r, bf in path_cases()])
def test_projection_paths_match_reference(shape, act, reduce, bf):
    """One shape per path of the dispatch (fusion_cases.PATHS says which), by the bounds of the test above."""
    case = proj_case(shape, act, reduce, bf)
    if shape in WALKS:
        # the library's own workspace says that a workgroup of the weight-gradient kernel walks more than one row tile
        parts, rtiles = ws_parts(_lib.load(), shape), geometry(shape)["rtiles"]
        print("%d wave partials = %d walkers for %d row tiles; cotangent zeroed at a share of %.2e" % (parts, parts // 4, rtiles,
                                                                                                    case.zeroed))
        assert parts % 4 == 0 and parts // 4 < rtiles == -(-shape[0] // 64)
        assert case.zeroed <= ZEROED_MAX, case.zeroed  # a condition on the inputs
    elif act != "tanh":
        assert case.kink >= KINK, case.kink
    graded(run_proj(case.inputs, shape[1], act, reduce, bf), case.ref, case.d0)


def test_projection_backward_is_deterministic():
    shape = (150, 1, 5, 72)
    inputs = proj_case(shape, "prelu", "sum", False)[0]
    a, b = run_proj(inputs, shape[1], "prelu", "sum", False), run_proj(inputs, shape[1], "prelu", "sum", False)
    assert all(torch.equal(a[n], b[n]) for n in a)


def test_walked_backward_is_deterministic():
    shape = (8229, 2, 24, 20)  # three, or two, row tiles per workgroup: the partials are still added in a fixed order
    inputs = proj_case(shape, "prelu", "sum", False).inputs
    a, b = run_proj(inputs, shape[1], "prelu", "sum", False), run_proj(inputs, shape[1], "prelu", "sum", False)
    assert all(torch.equal(a[n], b[n]) for n in a)


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(8229, 2, 24, 20), (150, 1, 5, 72)])
def test_backward_without_the_input_gradient(shape, bf):
    """What nn.fusionRNN_jit runs: x is the network input and needs no gradient, so pk_fusion_bwd gets dx = NULL and skips
    the dx kernel.  Everything else must keep its bits."""
    inputs = proj_case(shape, "prelu", "sum", bf).inputs
    full, lean = run_proj(inputs, shape[1], "prelu", "sum", bf), run_proj(inputs, shape[1], "prelu", "sum", bf, need_dx=False)
    assert full["dx"] is not None and lean.pop("dx") is None
    assert sorted(lean) == ["P", "dW", "db", "dslope"] and all(torch.equal(lean[n], full[n]) for n in lean)


@pytest.mark.parametrize("shape,bf,words", REFUSED)
def test_refusals_one_step_beyond_the_limits(shape, bf, words):
    N, M, F, H0 = shape
    F_.set_precision("bf16" if bf else "fp32")
    try:
        with pytest.raises(_lib.PkError, match=words):
            F_.fusion_proj(torch.zeros(N, M * F).cuda(), torch.zeros(2 * H0, F).cuda(), torch.zeros(2 * H0).cuda(), None, M, "relu",
                           "sum")
    finally:
        F_.set_precision("fp32")


T, B, M, F, P_DROP = 9, 3, 3, 4, 0.2
CLASS_SEED = {("prelu", "sum"): 0, ("tanh", "mean"): 0}


def options(act, reduce, lay="12,12,12"):
    return {"fusionRNN_lay": lay, "fusionRNN_drop": ",".join([str(P_DROP)] * 3), "fusionRNN_bidir": "True",
            "fusionRNN_act": "relu,relu,relu", "fusionRNN_do_fusion": "True", "fusionRNN_fusion_layer_size": "24",
            "fusionRNN_number_of_mic": str(M), "fusionRNN_fusion_act": act, "fusionRNN_fusion_reduce": reduce,
            "use_cuda": "True", "to_do": "train"}


@functools.lru_cache(maxsize=None)
def class_case(act, reduce, train, bf):
    torch.manual_seed(CLASS_SEED[(act, reduce)])
    net = nn_amd.fusionRNN_jit(options(act, reduce), M * F)
    g = torch.Generator().manual_seed(CLASS_SEED[(act, reduce)] + 1)
    with torch.no_grad():  # every parameter and statistic off its initial value: biases, shifts and running statistics count
        for n, t in net.state_dict().items():
            if n.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif t.is_floating_point() and (t.dim() == 1):
                t.add_(0.2 * torch.randn(t.shape, generator=g))
    x, cot = torch.randn(T, B, M * F, generator=g), torch.randn(T, B, 24, generator=g)
    eps = torch.randint(0, 2, x.shape, generator=g).double() * 2 - 1
    masks = [torch.ones(1)] * 3
    if train:
        masks = [(torch.rand(2 * B, h, generator=g) > P_DROP).float() / (1 - P_DROP) for h in (8, 12, 12)]

    def run(xin):
        sd = {n: t.detach().clone().double() for n, t in net.state_dict().items()}
        names = [n for n, _ in net.named_parameters()]
        for n in names:
            sd[n].requires_grad_()
        rx, kinks = xin.double().requires_grad_(), []
        y = fusion_rnn_ref(sd, rx, M, act, reduce, [m.double() if m.numel() > 1 else None for m in masks], train, bf, kinks)
        (y * cot.double()).sum().backward()
        out = dict({"y": y.detach(), "dx": rx.grad}, **{n: sd[n].grad for n in names})
        out.update({n: t for n, t in sd.items() if "running" in n})
        return out, min(float(k.min()) for k in kinks)

    ref, kink = run(x)
    d0 = None
    if bf:
        pert = run(x.double() * (1 + 2.0 ** -24 * eps))[0]
        d0 = {n: rel_err(pert[n], ref[n]) for n in ref}
    return net.state_dict(), x, cot, masks, ref, d0, kink


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("act,reduce", list(CLASS_SEED))
def test_class_matches_reference(act, reduce, train, bf):
    sd, x, cot, masks, ref, d0, kink = class_case(act, reduce, train, bf)
    assert kink >= KINK, kink
    net = nn_amd.fusionRNN_jit(options(act, reduce), M * F)
    net.load_state_dict(sd)
    net.cuda().train(train)
    ex = x.cuda().requires_grad_()
    F_.set_precision("bf16" if bf else "fp32")
    try:
        y = net(ex, drop_masks=masks)
        (y * cot.cuda()).sum().backward()
    finally:
        F_.set_precision("fp32")
    got = dict({"y": y, "dx": ex.grad}, **{n: p.grad for n, p in net.named_parameters()})
    got.update({n: t for n, t in net.state_dict().items() if "running" in n})
    ref = dict(ref)
    if train:
        # A bias in front of a training-mode BatchNorm has a gradient of exactly zero; the reference's own figure is float64
        # rounding noise, against which no relative error means anything.  Graded absolutely instead, on the scale of the
        # gradient of the normalisation's shift, the quantity the same column sums produce.
        for i in (1, 2):
            for w in ("wz", "wh"):
                n = "model.%d.%s.bias" % (i, w)
                scale = float(ref["model.%d.bn_%s.bias" % (i, w)].norm())
                assert float(ref.pop(n).norm()) < 1e-9 * scale and float(got[n].norm()) < TOL * scale
    graded(got, ref, d0)
