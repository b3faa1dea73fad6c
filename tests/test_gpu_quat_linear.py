"""functional.quat_linear / nn.QuaternionLinear on the GPU (pk_quat_linear.hip) against an fp64 construction of the real
matrix of include/pk_amd.h, W[q*O + o][p*I + i] = S[q][p] * comp[q ^ p][i][o], and torch.autograd."""
import ctypes
import importlib

import pytest
import torch

from golden_util import Golden, rel_err

pytestmark = pytest.mark.gpu
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

S = torch.tensor([[1, -1, -1, -1], [1, 1, -1, 1], [1, 1, 1, -1], [1, -1, 1, 1]], dtype=torch.float64)
# the last shape: dcomp's row slices are 256 rows here (1024 workgroups wanted, slices of at least 256 rows): ten slices,
# the last of 196 rows.  One shape more than the issue lists: forward and dX take 64-row tiles (two MFMA row tiles per wave) from
# 256 workgroups on, 33 x 9 here, ragged in every dimension
SHAPES = [(1, 1, 1), (7, 5, 3), (33, 8, 8), (150, 68, 36), (2500, 4, 4), (2110, 260, 260)]
TOL = 1e-4


def _ref(x, comps, bias, cot, rnd=lambda t: t):
    """Y, dX, [dcomp], dbias in float64; rnd rounds the two operands of each product (the bf16 mode's model)."""
    W = lambda cs: torch.cat([torch.cat([S[q, p] * cs[q ^ p].t() for p in range(4)], 1) for q in range(4)], 0)  # noqa: E731
    x, cot, comps = x.double(), cot.double(), [c.double() for c in comps]
    y = rnd(x) @ W([rnd(c) for c in comps]).t() + (0 if bias is None else bias.double())
    dx = rnd(cot) @ W([rnd(c) for c in comps])
    leaves = [c.clone().requires_grad_(True) for c in comps]
    (((rnd(x) @ W(leaves).t()) * rnd(cot)).sum()).backward()
    return y, dx, [c.grad for c in leaves], cot.sum(0)


def _case(N, I, O, seed=0):
    g = torch.Generator().manual_seed(seed + N + 7 * I + 13 * O)
    comps = [torch.randn(I, O, generator=g) for _ in range(4)]  # independent: a wrong sign or block is an O(1) error
    return torch.randn(N, 4 * I, generator=g), comps, torch.randn(4 * O, generator=g), torch.randn(N, 4 * O, generator=g)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("shape", SHAPES + ["3d"])
def test_quat_linear_matches_fp64(shape, use_bias, prec):
    lead = None
    if shape == "3d":  # [T, B, 4I] with T * B = N
        lead, shape = (10, 15), (150, 68, 36)
    N, I, O = shape
    x, comps, bias, cot = _case(N, I, O)
    rnd = (lambda t: t.float().bfloat16().double()) if prec == "bf16" else (lambda t: t)
    y_r, dx_r, dc_r, db_r = _ref(x, comps, bias if use_bias else None, cot, rnd)
    xd = x.cuda().view(*(lead or (N,)), 4 * I).requires_grad_(True)
    cd = [c.cuda().requires_grad_(True) for c in comps]
    bd = bias.cuda().requires_grad_(True) if use_bias else None
    F_.set_precision(prec)
    try:
        y = F_.quat_linear(xd, *cd, bd)
        grads = [torch.autograd.grad(y, [xd] + cd + ([bd] if use_bias else []), cot.cuda().view(y.shape), retain_graph=True)
                 for _ in range(2)]
    finally:
        F_.set_precision("fp32")
    assert y.shape == (*(lead or (N,)), 4 * O)
    errs = {"y": rel_err(y.reshape(N, -1), y_r), "dx": rel_err(grads[0][0].reshape(N, -1), dx_r)}
    errs.update({"d" + "rijk"[c]: rel_err(grads[0][1 + c], dc_r[c]) for c in range(4)})
    if use_bias:
        errs["db"] = rel_err(grads[0][5], db_r)
    print(shape, prec, errs)
    assert all(e < TOL for e in errs.values()), errs
    assert all(torch.equal(a, b) for a, b in zip(*grads))  # the row-split reduction has a fixed order


@pytest.mark.parametrize("N,I,O", [(2500, 4, 4), (150, 68, 36)])
def test_bwd_w_beta(N, I, O):
    lib = _lib.load()
    x, comps, _, cot = _case(N, I, O)
    dc_r = _ref(x, comps, None, cot)[2]
    xd, dyd = x.cuda(), cot.cuda()
    ws = torch.empty(int(lib.pk_quat_linear_work_floats(N, I, O)), device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pre = torch.randn(4, I, O, generator=torch.Generator().manual_seed(5)).cuda()
    acc, over = pre.clone(), torch.full((4, I, O), float("nan"), device="cuda")
    for beta, d in ((1.0, acc), (0.0, over)):
        rc = lib.pk_quat_linear_bwd_w(st, 0, N, I, O, xd.data_ptr(), dyd.data_ptr(), beta, None, d.data_ptr(), None, ws.data_ptr())
        _lib.check(rc, "pk_quat_linear_bwd_w")
    assert bool(torch.isfinite(over).all())
    assert rel_err(over, torch.stack(dc_r)) < TOL and rel_err(acc - pre, torch.stack(dc_r)) < TOL


def test_module_reproduces_the_reference_fixture():
    g = Golden("e2e_quat_linear_ref")
    net = nn_amd.QuaternionLinear(g.meta["in"], g.meta["out"])
    net.load_state_dict(g.group("sd/"), strict=True)
    net.cuda()
    x = g.t("x").cuda().requires_grad_(True)
    y = net(x)
    y.backward(g.t("cot").cuda())
    assert rel_err(y, g.t("y")) < TOL and rel_err(x.grad, g.t("dx")) < TOL
    for k, p in net.named_parameters():
        assert rel_err(p.grad, g.t("grad/" + k)) < TOL, k
