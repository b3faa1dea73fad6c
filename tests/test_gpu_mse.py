"""functional.mse_cost on the GPU (pk_mse.hip) against the float64 restatement ((a.double() - b.double()) ** 2).mean() and its
autograd on the CPU: the loss and both gradients, graded with golden_util.rel_err.

Bar per quantity, the rule of test_gpu_sincfast.py: 1e-4, the project's parity bar, or 4 x the distance that stock float32
torch on the CPU has from the same float64 values, whichever is larger.  Every case prints both distances.  Each case runs
twice and must give the same bits."""
import functools
import importlib

import pytest
import torch

from golden_util import rel_err

pytestmark = pytest.mark.gpu
F_ = importlib.import_module("pytorch-kaldi_amd.functional")

# name -> (shape, layout of a, layout of b); a layout is None (dense) or (width of the tensor it is a column slice of, first column)
CASES = {
    "one_element": ((1, 1), None, None),                  # the tail alone
    "flat_tail": ((63, 3), None, None),                   # flat form, rows*F % 4 = 1
    "odd_slice": ((257, 40), None, (83, 1)),              # scalar form: never 16-byte aligned, pitch % 4 = 3
    "aligned_slices": ((257, 40), (84, 0), (84, 4)),      # quad form, every row aligned
    "moving_head": ((257, 40), (83, 1), (83, 5)),         # quad form, head and tail change from row to row
    "one_wave": ((130, 64), None, None),                  # F of exactly one wave
    "long_row": ((5, 200), None, (210, 2)),               # a row longer than a wave, a few rows
    # The launch rule gives a forward workgroup at least 8192 elements (4096 backward): 1025 * 40 = 41 000 elements are
    # 6 workgroups and 6 partials forward, 11 workgroups backward, with a last run shorter than the others.
    "many_wg_flat": ((1025, 40), None, None),
    "many_wg_scalar": ((1025, 40), None, (83, 1)),
    "many_wg_quads": ((1025, 40), (83, 1), (83, 5)),
    "three_dims": ((7, 5, 40), None, (90, 3)),            # leading dimensions collapse; b stays where it is
}
MODES = {"a": (True, False), "both": (True, True), "b": (False, True)}
DLOSS = 0.37


def cut(whole, shape, layout):
    return whole if layout is None else whole[..., layout[1]:layout[1] + shape[-1]]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The tensors a and b are cut from (on the CPU), and per dtype the loss and both gradients of 0.37 * loss from stock
    torch"""
    shape, la, lb = CASES[name]
    gen = torch.Generator().manual_seed(sorted(CASES).index(name))
    wa, wb = (torch.randn(*shape[:-1], shape[-1] if lay is None else lay[0], generator=gen) for lay in (la, lb))
    a, b = cut(wa, shape, la), cut(wb, shape, lb)
    out = {}
    for dt in (torch.float64, torch.float32):
        x, y = a.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
        loss = ((x - y) ** 2).mean()
        (loss * DLOSS).backward()
        out[dt] = {"loss": loss.detach(), "da": x.grad, "db": y.grad}
    return wa, wb, out[torch.float64], out[torch.float32]


def gpu_run(name, wa, wb, need_a, need_b):
    # cut on the device: the kernel sees the pitch of the tensor the operand is a slice of
    shape, la, lb = CASES[name]
    x = cut(wa.cuda(), shape, la).detach().requires_grad_(need_a)
    y = cut(wb.cuda(), shape, lb).detach().requires_grad_(need_b)
    assert x.stride(-2) == wa.shape[-1] and y.stride(-2) == wb.shape[-1] and x.shape == y.shape == shape
    loss = F_.mse_cost(x, y)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("MseCostFn") and loss.shape == ()
    (loss * DLOSS).backward()
    got = {"loss": loss.detach()}
    if need_a:
        got["da"] = x.grad
    if need_b:
        got["db"] = y.grad
    assert (x.grad is None) == (not need_a) and (y.grad is None) == (not need_b)
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_against_float64(name, mode):
    wa, wb, ref, stock32 = case_data(name)
    first, got = gpu_run(name, wa, wb, *MODES[mode]), gpu_run(name, wa, wb, *MODES[mode])
    for k, v in got.items():
        assert torch.equal(v, first[k]), k + " differs between two runs"
        assert v.shape == ref[k].shape and v.is_contiguous()
        e, floor = rel_err(v, ref[k]), rel_err(stock32[k], ref[k])
        print("%s %s %s: kernel %.3e, stock fp32 %.3e" % (name, mode, k, e, floor))
        assert e <= max(1e-4, 4.0 * floor), (name, mode, k, e, floor)


def test_forward_model_routes_the_mse_line_without_copying_the_slice():
    U = importlib.import_module("pytorch-kaldi_amd.utils")
    N, F = 18, 40
    inp = torch.randn(N, 2 * F + 1, generator=torch.Generator().manual_seed(5)).cuda()
    net = torch.nn.Linear(F, F).cuda()
    spec = {"noisy": ["noisy", "lst", "opts", "0", "0", 0, F], "clean": ["clean", "lst", "opts", "0", "0", F, 2 * F]}
    sizes = {"noisy": ["a", "b", "c", "d", "e", 0, F, F], "clean": ["a", "b", "c", "d", "e", F, 2 * F, F], "out": [F]}
    spec["one"] = ["one", "lst", "opts", "0", "0", 2 * F, 2 * F + 1]  # a column that broadcasts: the stock expression
    model = ["out=compute(net,noisy)", "loss=mse(out,clean)", "loss_b=mse(out,one)"]
    outs = U.forward_model(spec, {}, {"net": ["architecture1", "net", False]}, model, {"net": net}, {}, inp, sizes, N, 1,
                           "train", [])
    assert type(outs["loss_b"].grad_fn).__name__.startswith("Mean")
    fn = outs["loss"].grad_fn
    assert type(fn).__name__.startswith("MseCostFn") and fn.saved_tensors[1].data_ptr() == inp[:, F:].data_ptr()
    want = torch.mean((outs["out"].double().cpu() - inp[:, F:2 * F].double().cpu()) ** 2)
    assert rel_err(outs["loss"], want) <= 1e-4


def test_nan_propagates():
    wa, wb, _, _ = case_data("odd_slice")
    a, b = wa.cuda(), wb.cuda()[:, 1:41]
    a[100, 7] = float("nan")
    assert torch.isnan(F_.mse_cost(a, b))          # the scalar form
    assert torch.isnan(F_.mse_cost(a, a.clone()))  # the flat form
