"""The 128-row streamed kernels of pk_quat_linear.hip (variant 1), forced at shapes the rule would give to variant 0, against
the real matrix of include/pk_amd.h built in float64: W[q*O + o][p*I + i] = S[q][p] * comp[q ^ p][i][o]."""
import ctypes
import importlib

import pytest
import torch

from golden_util import rel_err

pytestmark = pytest.mark.gpu
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

S = torch.tensor([[1, -1, -1, -1], [1, 1, -1, 1], [1, 1, 1, -1], [1, -1, 1, 1]], dtype=torch.float64)
# all tail | exact tile | a row past a tile, odd widths (4-byte loads) | three k steps with a k tail: both LDS stages reused,
# and a B-tile tail | dcomp: three slices of 224, 224 and 152 rows, several k steps each, the last slice short
SHAPES = [(1, 1, 1), (128, 8, 16), (129, 5, 3), (257, 70, 65), (600, 33, 40)]
TOL = 1e-4


def _ref(x, comps, bias, dy, rnd):
    x, dy, comps = x.double(), dy.double(), [c.double() for c in comps]
    I, O = comps[0].shape
    W = torch.cat([torch.cat([S[q, p] * rnd(comps[q ^ p]).t() for p in range(4)], 1) for q in range(4)], 0)
    dW = rnd(dy).t() @ rnd(x)
    dc = [sum(S[q, q ^ c] * dW[q * O:(q + 1) * O, (q ^ c) * I:((q ^ c) + 1) * I].t() for q in range(4)) for c in range(4)]
    return rnd(x) @ W.t() + (0 if bias is None else bias.double()), rnd(dy) @ W, torch.stack(dc), dy.sum(0)


@pytest.mark.parametrize("by_base", [True, False])
@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("N,I,O", SHAPES)
def test_wide_kernels_match_fp64(N, I, O, prec, use_bias, by_base):
    lib = _lib.load()
    g = torch.Generator().manual_seed(N + 7 * I + 13 * O)
    comps = [torch.randn(I, O, generator=g) for _ in range(4)]  # independent: a wrong sign or block is an O(1) error
    x, bias, dy = torch.randn(N, 4 * I, generator=g), torch.randn(4 * O, generator=g), torch.randn(N, 4 * O, generator=g)
    rnd = (lambda t: t.float().bfloat16().double()) if prec == 1 else (lambda t: t)
    y_r, dx_r, dc_r, db_r = _ref(x, comps, bias if use_bias else None, dy, rnd)
    xd, dyd, bd = x.cuda(), dy.cuda(), bias.cuda() if use_bias else None
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    names = lambda ts: (None, ptr(ts)) if by_base else ((ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts]), None)  # noqa: E731
    cd = torch.stack(comps).cuda() if by_base else [c.cuda() for c in comps]
    y, dx = torch.empty(N, 4 * O, device="cuda"), torch.empty(N, 4 * I, device="cuda")
    ws = torch.empty(int(lib.pk_quat_linear_work_floats(N, I, O)), device="cuda")
    pre = torch.randn(4, I, O, generator=g).cuda()
    st, runs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), []
    lib.pk_quat_linear_set_variant(1)
    try:
        assert all(lib.pk_quat_linear_variant(p, prec, N, I, O) == 1 for p in range(3))
        _lib.check(lib.pk_quat_linear_fwd(st, prec, N, I, O, ptr(xd), *names(cd), ptr(bd), ptr(y)), "pk_quat_linear_fwd")
        _lib.check(lib.pk_quat_linear_bwd_x(st, prec, N, I, O, ptr(dyd), *names(cd), ptr(dx)), "pk_quat_linear_bwd_x")
        for beta in (0.0, 1.0, 0.0):
            d = pre.clone() if beta else torch.full((4, I, O), float("nan"), device="cuda")
            db = torch.full((4 * O,), float("nan"), device="cuda") if use_bias else None
            _lib.check(lib.pk_quat_linear_bwd_w(st, prec, N, I, O, ptr(xd), ptr(dyd), beta, *names(d if by_base else list(d)),
                                                ptr(db), ptr(ws)), "pk_quat_linear_bwd_w")
            runs.append((d - pre if beta else d, db))
    finally:
        lib.pk_quat_linear_set_variant(-1)
    errs = {"y": rel_err(y, y_r), "dx": rel_err(dx, dx_r), "dcomp": rel_err(runs[0][0], dc_r), "dcomp beta 1": rel_err(runs[1][0], dc_r)}
    if use_bias:
        errs["dbias"] = rel_err(runs[0][1], db_r)
        assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])
    print((N, I, O), prec, errs)
    assert all(e < TOL for e in errs.values()), errs
    assert torch.equal(runs[0][0], runs[2][0])  # the row-split reduction has a fixed order


def test_module_reaches_both_variants():
    lib = _lib.load()
    net = nn_amd.QuaternionLinear(4 * 70, 4 * 65).cuda()
    g = torch.Generator().manual_seed(3)
    x0, cot = torch.randn(257, 4 * 70, generator=g).cuda(), torch.randn(257, 4 * 65, generator=g).cuda()
    out = {}
    try:
        for v in (0, 1):
            lib.pk_quat_linear_set_variant(v)
            x = x0.clone().requires_grad_(True)
            net.zero_grad()
            y = net(x)
            y.backward(cot)
            out[v] = [y.detach(), x.grad] + [p.grad.clone() for p in net.parameters()]
    finally:
        lib.pk_quat_linear_set_variant(-1)
    assert all(rel_err(a, b) < TOL for a, b in zip(out[1], out[0])), [rel_err(a, b) for a, b in zip(out[1], out[0])]
