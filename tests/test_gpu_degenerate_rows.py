"""Degenerate and ill-conditioned rows and columns through the normalisation and softmax kernels.

Every other numerical test feeds the kernels randn data and grades with a whole-tensor norm ratio.  Here: LayerNorm rows
of variance exactly 0 (zero-padded frames), BatchNorm columns with |mean| >> std, logits that overflow exp() unless the
maximum is subtracted first - graded per row, per column or per group of rows (golden_util.rel_err_rows /
rel_err_split), because a few rows with 1e6-sized gradients dominate a whole-tensor norm and a few zero rows vanish in
it.  The inputs come from tests/degenerate_inputs.py; tests/test_degenerate_inputs_host.py checks on the references
alone that they are what they claim to be.  Tolerances are the project's own numbers for each quantity, applied per
row / column / group; the BatchNorm outputs on ill-conditioned columns are bounded by max(that number, 4 x the error of
torch's own fp32 CPU BatchNorm on the same column) - see test_batchnorm_on_ill_conditioned_columns."""
import ctypes
import functools
import importlib

import pytest
import torch
import torch.nn.functional as TF

import degenerate_inputs as D
import pk_oracle as O
from golden_util import check_grads, rel_err, rel_err_rows, rel_err_split

pytestmark = pytest.mark.gpu
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
TOL = 1e-4  # fp32 recurrent parity (tests/test_gpu_parity.py)


@pytest.fixture(autouse=True)
def _fp32_mode():
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")
    yield
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")
    F_.set_forced_kinks(None)
    F_.set_forced_decisions(None, None)


def _fmt(v):
    return "[" + " ".join("%.1e" % float(e) for e in torch.as_tensor(v).reshape(-1)) + "]"


def _cols(a, b):
    """Per-entry relative error of two vectors (one figure per column)."""
    return rel_err_rows(a.reshape(1, -1), b.reshape(1, -1), 0)


# ------------------------------------------------------------------------------------------------
# A. LayerNorm: zero-variance and offset rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,F", D.LN_SHAPES)
def test_layernorm_zero_variance_and_offset_rows(rows, F):
    """F_.layer_norm on rows of zeros, of 0.5, of 1e3 + randn, with one non-zero element, and randn rows, against fp64
    autograd through the oracle's LayerNorm (torch masks the derivative of std() to 0 where std == 0, so the
    reference's gradient on a zero-variance row is the finite rinv * (g - mean(g))).  y per row, dx as two groups
    (zero-variance rows | the others) and per row, dgamma / dbeta whole - all at the 1e-5 of test_layernorm."""
    c = D.layernorm_rows(rows, F)
    xr, gr, br = (t.double().requires_grad_(True) for t in (c.x, c.gamma, c.beta))
    yr = O.layer_norm(xr, gr, br)
    (yr * c.cot.double()).sum().backward()
    xe, ge, be = (t.clone().cuda().requires_grad_(True) for t in (c.x, c.gamma, c.beta))
    y = F_.layer_norm(xe, ge, be, 1e-6)
    (y * c.cot.cuda()).sum().backward()
    e_y, e_dx = rel_err_rows(y, yr, 1), rel_err_rows(xe.grad, xr.grad, 1)
    e_deg, e_ord = rel_err_split(xe.grad, xr.grad, c.degenerate)
    e_g, e_b = rel_err(ge.grad, gr.grad), rel_err(be.grad, br.grad)
    print("\nlayer_norm %dx%d: y per row %s, dx per row %s, dx zero-variance rows %.1e / others %.1e, dgamma %.1e, dbeta %.1e"
          % (rows, F, _fmt(e_y), _fmt(e_dx), e_deg, e_ord, e_g, e_b))
    assert bool((e_y < 1e-5).all()), e_y
    assert e_deg < 1e-5 and e_ord < 1e-5, (e_deg, e_ord)
    assert bool((e_dx < 1e-5).all()), e_dx
    assert e_g < 1e-5 and e_b < 1e-5, (e_g, e_b)


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("B,C,L", D.CONV_TAIL_SHAPES)
def test_conv_tail_layernorm_zero_variance_rows(B, C, L, act, drop):
    """F_.ln_last_act_drop (one launch) and the launches it replaces (F_.layer_norm_last + F_.norm_act_drop) on a
    [B, C, L] input with two all-zero (b, c) rows and one of 0.5 - a channel whose pooled output is constant over time -
    against fp64 autograd through the oracle.  y per (b, c) row at 1e-5; dz as two groups, dgamma / dbeta per channel at
    the 2e-5 of test_conv_layer_tail_in_one_launch."""
    c = D.conv_tail_rows(B, C, L, drop)
    zr, gr, br = (t.double().requires_grad_(True) for t in (c.z, c.gamma, c.beta))
    yr = O.activation(act, O.layer_norm(zr, gr, br))
    if c.mask is not None:
        yr = yr * c.mask.double()
    (yr * c.cot.double()).sum().backward()
    mask = None if c.mask is None else c.mask.cuda()
    for form in ("one launch", "layer_norm_last"):
        ze, ge, be = (t.clone().cuda().requires_grad_(True) for t in (c.z, c.gamma, c.beta))
        if form == "one launch":
            y = F_.ln_last_act_drop(ze, ge, be, 1e-6, act, mask)
        else:
            m2 = None if mask is None else mask.reshape(B * C, L)
            y = F_.norm_act_drop(F_.layer_norm_last(ze, ge, be, 1e-6).reshape(B * C, L), None, False, True, act, m2).view(B, C, L)
        (y * c.cot.cuda()).sum().backward()
        e_y = rel_err_rows(y.reshape(B * C, L), yr.reshape(B * C, L), 1)
        e_deg, e_ord = rel_err_split(ze.grad.reshape(B * C, L), zr.grad.reshape(B * C, L), c.degenerate)
        e_g, e_b = rel_err_rows(ge.grad, gr.grad, 1), rel_err_rows(be.grad, br.grad, 1)
        print("\nconv tail %s %s (%d,%d,%d) drop=%s: y worst row %.1e, dz zero-variance rows %.1e / others %.1e, dgamma worst "
              "channel %.1e, dbeta %.1e" % (form, act, B, C, L, drop, float(e_y.max()), e_deg, e_ord, float(e_g.max()), float(e_b.max())))
        assert bool((e_y < 1e-5).all()), (form, e_y)
        assert e_deg < 2e-5 and e_ord < 2e-5, (form, e_deg, e_ord)
        assert bool((e_g < 2e-5).all()) and bool((e_b < 2e-5).all()), (form, e_g, e_b)


@functools.lru_cache(maxsize=None)
def _rec_case(kind, pre, act, H, bidir):
    return D.rec_zero_frame(kind, pre, act, H, bidir)


@functools.lru_cache(maxsize=None)
def _rec_ref(kind, pre, act, H, bidir, prec):
    """The oracle's run of a case: computed once, shared by the routes that are graded against it, never modified."""
    return D.rec_reference(_rec_case(kind, pre, act, H, bidir), prec)


# route name -> (precision, forced algorithm, what rec_route must answer for a layer with per-step LayerNorm)
def _expected_route(route, kind):
    two_phase = kind in ("GRU", "minimalGRU")
    return {"fp32-stepwise": ("fp32", "stepwise", F_.RecRoute(False, F_.REC_STEPWISE, "generic")),
            "fp32-persistent": ("fp32", "persistent", F_.RecRoute(False, F_.REC_PERSISTENT, "generic")),
            "bf16-persistent": ("bf16", "auto", F_.RecRoute(False, F_.REC_PERSISTENT, "2p_bf16_ln" if two_phase else "bf16_ln"))}[route]


def _run_rec(c, ref):
    net = getattr(nn_amd, c.kind)(c.opts, c.D)
    net.load_state_dict({k: v.clone() for k, v in c.sd.items()}, strict=True)
    net.cuda().train()
    report = F_.set_forced_kinks(ref.log) if ref.log is not None else None
    try:
        xe = c.x.clone().cuda().requires_grad_(True)
        ye = net(xe, drop_masks=c.masks)
        (ye * c.cot.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        F_.set_forced_kinks(None)
    got = {k: (q.grad.detach().cpu() if q.grad is not None else None) for k, q in net.named_parameters()}
    return ye.detach().cpu(), xe.grad.cpu(), got, report


@pytest.mark.parametrize("kind,pre,act,H,bidir,route", D.REC_CASES)
def test_per_step_layernorm_on_a_zero_frame(kind, pre, act, H, bidir, route):
    """`*_use_laynorm=True` on a batch with one all-zero frame: the direction that starts on it (h = 0, no projection
    bias) normalises an all-zero state, a row of variance exactly 0.  The oracle's gradients are finite there (up to
    ~1e6 in dx for the tanh cells); every route rec_route can answer for such a layer must match it - fp32 (step-wise,
    persistent) against the fp32 oracle at 1e-4, bf16 persistent against the bf16-operand model at 5e-3 / 2e-2 - with
    the (t, b) positions of the zero frame and all the others graded as two groups."""
    prec, algo, want = _expected_route(route, kind)
    c, ref = _rec_case(kind, pre, act, H, bidir), _rec_ref(kind, pre, act, H, bidir, prec)
    F_.set_precision(prec)
    F_.set_rec_algo(algo)
    assert F_.rec_route(kind, H, True, False, True) == want
    ye, dxe, got, report = _run_rec(c, ref)
    otol, gtol = (TOL, TOL) if prec == "fp32" else (5e-3, 2e-2)
    ey0, ey1 = rel_err_split(ye, ref.y, c.zero)
    ex0, ex1 = rel_err_split(dxe, ref.dx, c.zero)
    print("\nzero frame %s H=%d bidir=%s %s: y zero frame %.1e / others %.1e, dx zero frame %.1e / others %.1e (max |dx| of the "
          "oracle %.1e)%s" % (kind, H, bidir, route, ey0, ey1, ex0, ex1, float(ref.dx.abs().max()),
                              "" if report is None else "; kink report %s" % (report,)))
    assert ey0 < otol and ey1 < otol, (ey0, ey1)
    assert ex0 < gtol and ex1 < gtol, (ex0, ex1)
    worst = check_grads(got, ref.grads, None, gtol)
    print("  worst parameter gradient %.1e" % worst)
    assert any(k.startswith("ln.") and v is not None and float(v.abs().max()) > 0 for k, v in got.items())


# ------------------------------------------------------------------------------------------------
# B. BatchNorm statistics on ill-conditioned columns
# ------------------------------------------------------------------------------------------------
BN_TOL, _bn_graded = D.BN_TOL, D.bn_graded


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("M,N", D.BN_SHAPES)
def test_batchnorm_on_ill_conditioned_columns(M, N, act):
    """F_.norm_act_drop (training-mode BatchNorm -> act -> mask) and F_.bn_stats on columns that are constant (0, 3.0), at
    1e2 + randn, at -1e3 + randn, randn with an outlier of 100 in the row a shifted sum pivots on, and 0.5 + 2 randn.  The
    shapes cover the scalar kernel (N % 4 != 0 / 2 rows), the 16-byte kernel and row counts one past a row block.
    Per column against fp64 on the very fp32 matrix the kernel read.  The bound per column is max(the project's
    tolerance for the quantity, 4 x e_ref), e_ref = the error of torch's fp32 CPU BatchNorm1d on that column against
    fp64: fp32 arithmetic loses eps * |mean| / std through x * scale + shift whatever the kernel (the factor 4 covers an
    equally valid summation order: a Chan merge over row blocks here, a cascade in torch).  A one-pass variance is 0.25 %
    / 23 % off on the 1e2 / 1e3 columns - far outside.  The ReLU is differentiated on the fp64 run's pattern on all sides."""
    c = D.batchnorm_columns(M, N)
    r64 = D.batchnorm_reference(c, act, torch.float64)
    r32 = D.batchnorm_reference(c, act, torch.float32, relu_pattern=r64["relu"])
    bn = torch.nn.BatchNorm1d(N, momentum=0.05)
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
    bn.cuda()
    xe = c.x.clone().cuda().requires_grad_(True)
    if act == "relu":
        F_.set_forced_decisions(relu=[r64["relu"]])
    try:
        ye = F_.norm_act_drop(xe, bn, True, True, act, c.mask.cuda())
        (ye * c.cot.cuda()).sum().backward()
    finally:
        F_.set_forced_decisions(None, None)
    mean, var = F_.bn_stats(c.x.cuda())
    torch.cuda.synchronize()
    got = {"y": ye, "dx": xe.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var, "mean": mean, "var": var}
    bad = []
    for k in _bn_graded(M):
        per = rel_err_rows if got[k].dim() == 2 else (lambda a, b, _d: _cols(a, b))
        e, e_ref = per(got[k], r64[k], 0), per(r32[k], r64[k], 0)
        bound = torch.clamp(4 * e_ref, min=BN_TOL[k])
        if k == "y":
            # measured on the -1e3 column at 257 rows: 3.5e-5 against e_ref 2.3e-6 - more than the factor 4.  The engine
            # evaluates x * scale + shift, torch's CPU kernel (x - mean) * invstd * gamma + beta; the former rounds the
            # mean, mean * scale and the shift to ulps of the LEVEL (degenerate_inputs.affine_bound: three half ulps of
            # |mean| times |scale|, 1.8e-4 for that column).  That is the margin its arithmetic supports, and no more.
            bound = torch.maximum(bound, D.affine_bound(r64["mean"], r64["var"], c.gamma, 1e-5, r64["y"], float(c.mask.max())))
        sel = [D.BN_ZERO, D.BN_CONST, D.BN_100, D.BN_1000, D.BN_OUTLIER, 5]
        print("\nBatchNorm %dx%d %s %-12s columns [0 | 3.0 | 1e2 | -1e3 | outlier | plain]: engine %s, e_ref %s; worst engine / bound %.2f"
              % (M, N, act, k, _fmt(e[sel]), _fmt(e_ref[sel]), float((e / bound).max())))
        if not bool((e <= bound).all()):
            bad.append((k, [(int(j), float(e[j]), float(bound[j])) for j in torch.nonzero(~(e <= bound)).reshape(-1)]))
    assert not bad, bad


@pytest.mark.parametrize("M,N,K", D.PROJ_SHAPES)
def test_projection_statistics_with_a_common_level(M, N, K):
    """F_.gemm_bf16_bn_stats when every column of the product has |mean| ~ 100 std: the statistics of the GEMM epilogue
    (the smallest shape on the 256-tile: 64 row blocks merged by pk_bn_stats_merge, and by
    pk_bn_stats_merge_finalize_gates when the gates' BatchNorms come along) and the fallback behind it (300 rows: plain GEMM
    + pk_bn_stats) - mean and biased variance of every column against fp64 on the matrix the GEMM wrote, at the 1e-5 of
    test_projection_gemm_with_batchnorm_statistics, per column."""
    x, w = D.projection_operands(M, N, K)
    xb, wb = F_.cvt_bf16(x.cuda()), F_.cvt_bf16(w.cuda())
    C = torch.empty(M, N, device="cuda")
    mean, var = F_.gemm_bf16_bn_stats(M, N, K, xb, xb.shape[1], 1, wb, wb.shape[1], 1, C, N)
    G, H = 2, N // 2
    gamma, beta = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    rms, rvs = [torch.zeros(H, device="cuda") for _ in range(G)], [torch.ones(H, device="cuda") for _ in range(G)]
    nbs = [torch.tensor(0, dtype=torch.int64, device="cuda") for _ in range(G)]
    C2 = torch.empty(M, N, device="cuda")
    mean2, var2, scale, shift = F_.gemm_bf16_bn_stats(M, N, K, xb, xb.shape[1], 1, wb, wb.shape[1], 1, C2, N,
                                                      gates=(gamma, beta, 1e-5, H, rms, rvs, nbs, 0.05, float(M)))
    torch.cuda.synchronize()
    Cd = C.double().cpu()
    ref = x.to(torch.bfloat16).double() @ w.to(torch.bfloat16).double().t()
    mu, vr = Cd.mean(0), Cd.var(0, unbiased=False)
    ratio = float((mu.abs() / vr.sqrt()).median())
    e_c = rel_err_rows(Cd, ref, 0)
    e_m, e_v, e_m2, e_v2 = _cols(mean, mu), _cols(var, vr), _cols(mean2, mu), _cols(var2, vr)
    e_s = _cols(scale, 1.0 / (vr + 1e-5).sqrt())
    e_rm = _cols(torch.cat(rms), 0.05 * mu)
    print("\nprojection statistics %dx%dx%d, |mean| / std %.0f: C worst column %.1e, mean %.1e, var %.1e; with the gates: mean %.1e, "
          "var %.1e, scale %.1e, running mean %.1e" % (M, N, K, ratio, float(e_c.max()), float(e_m.max()), float(e_v.max()),
                                                      float(e_m2.max()), float(e_v2.max()), float(e_s.max()), float(e_rm.max())))
    assert ratio > 50
    assert torch.equal(C, C2)
    assert bool((e_c < 1e-5).all())
    assert bool((e_m < 1e-5).all()) and bool((e_v < 1e-5).all()), (float(e_m.max()), float(e_v.max()))
    assert bool((e_m2 < 1e-5).all()) and bool((e_v2 < 1e-5).all()), (float(e_m2.max()), float(e_v2.max()))
    assert bool((e_s < 1e-5).all()) and bool((e_rm < 1e-5).all())


@pytest.mark.parametrize("M,N,K,act,masked", D.SMALL_BATCH_CASES)
def test_small_batch_layer_with_a_common_level(M, N, K, act, masked):
    """The one-launch small-batch layer (pk_linear_bn_act_bf16, through F_.linear_bn_act in bf16 mode) on operands whose
    product columns have |mean| ~ 100 std: per column against the two-launch form (pk_linear_bn_act_bf16_sk) at the
    2e-5 of test_small_batch_layer_two_launch_form_matches_the_one_launch_form, and against fp64 on the bf16-rounded
    operands - z at 2e-5, the batch mean at 1e-4, the activation at max(1e-4, 4 x e_ref) with e_ref = torch's fp32
    BatchNorm on the fp32-rounded fp64 product.  The batch variance is held to 1e-4 as well: a two-pass or shifted
    variance is at a few fp32 eps whatever the level, a one-pass E[x^2] - E[x]^2 loses eps * (mean / std)^2 = 6e-4 here."""
    lib = _lib.load()
    s = D.small_batch_layer(M, N, K, act, masked)
    x, w, bias, gamma, beta, mask = s.x, s.w, s.bias, s.gamma, s.beta, s.mask
    zr, mu, vr, ar, e_ref, ratio = s.z, s.mean, s.var, s.a, s.e_ref, s.ratio
    # the module path (one launch)
    bn = torch.nn.BatchNorm1d(N, momentum=0.05)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    bn.cuda()
    F_.set_precision("bf16")
    xe, we, be = x.cuda(), w.cuda(), bias.cuda()
    assert F_.linear_bn_act_ok(xe, we, True, True, act)
    with torch.no_grad():
        y = F_.linear_bn_act(xe, we, be, bn, act, None if mask is None else mask.cuda())
    a_mod = y if mask is None else None
    # the two forms at the library's entry points
    sk = int(lib.pk_gemm_bf16_small_splitk(M, N, K))
    assert sk >= 2
    xb, wb = F_.cvt_bf16(xe), F_.cvt_bf16(we)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    gm, bt, mk = gamma.cuda(), beta.cuda(), (None if mask is None else mask.cuda())
    outs = []
    for form in (0, 1):
        z, a, yy = (torch.empty(M, N).cuda() for _ in range(3))
        yb = torch.empty(M, N, dtype=torch.bfloat16).cuda()
        mean, var = torch.empty(N).cuda(), torch.empty(N).cuda()
        rm, rv = torch.zeros(N).cuda(), torch.ones(N).cuda()
        args = [st, M, N, K, p(xb), xb.shape[1], p(wb), wb.shape[1], p(be), p(gm), p(bt), 1e-5, 0.05, p(rm), p(rv), F_.ACT[act],
                p(mk), p(z), p(a), p(yy) if masked else None, p(yb), N, p(mean), p(var)]
        if form == 0:
            _lib.check(lib.pk_linear_bn_act_bf16(*args), "one launch")
        else:
            ws = torch.empty(sk * M * N).cuda()
            _lib.check(lib.pk_linear_bn_act_bf16_sk(*args, sk, p(ws)), "two launches")
        torch.cuda.synchronize()
        outs.append({"z": z, "a": a, "y": yy if masked else a, "mean": mean, "var": var, "rm": rm, "rv": rv})
    one, two = outs
    yr = s.y
    e_forms = {k: rel_err_rows(one[k].reshape(-1, N), two[k].reshape(-1, N), 0) for k in one}
    e_z, e_a, e_mu, e_var = rel_err_rows(one["z"], zr, 0), rel_err_rows(one["a"], ar, 0), _cols(one["mean"], mu), _cols(one["var"], vr)
    e_y = rel_err_rows(y, yr, 0)
    # both forms evaluate z * scale + shift: each is within affine_bound of the exact value (see there; measured between
    # the forms 7.9e-5 on a ReLU column that is mostly zero, whose bound is 2 x 1.6e-4), so within twice that of each other
    bound_a, bound_y = torch.maximum(torch.clamp(4 * e_ref, min=1e-4), s.aff_a), torch.maximum(torch.clamp(4 * e_ref, min=1e-4), s.aff_y)
    bound_forms = {"a": torch.clamp(2 * s.aff_a, min=2e-5), "y": torch.clamp(2 * s.aff_y, min=2e-5)}
    print("\nsmall-batch layer %dx%dx%d %s, |mean| / std %.0f: one launch vs two, worst column %s; vs fp64: z %.1e, a %.1e (e_ref %.1e, "
          "worst a / bound %.2f), mean %.1e, var %.1e; module output %.1e"
          % (M, N, K, act, ratio, {k: "%.1e" % float(v.max()) for k, v in e_forms.items()}, float(e_z.max()), float(e_a.max()),
             float(e_ref.max()), float((e_a / bound_a).max()), float(e_mu.max()), float(e_var.max()), float(e_y.max())))
    assert ratio > 50
    for k, v in e_forms.items():
        assert bool((v <= bound_forms.get(k, torch.tensor(2e-5))).all()), (k, float(v.max()))
    assert bool((e_z < 2e-5).all()) and bool((e_mu < 1e-4).all()) and bool((e_var < 1e-4).all())
    assert bool((e_a <= bound_a).all()) and bool((e_y <= bound_y).all()), (float((e_a / bound_a).max()), float((e_y / bound_y).max()))
    if a_mod is not None:  # (the module takes whichever form the library recommends for the shape)
        assert torch.equal(a_mod, one["a"]) or torch.equal(a_mod, two["a"])


@functools.lru_cache(maxsize=None)
def _rec_bn_case():
    return D.rec_batchnorm_offset()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_recurrent_layer_batchnorm_with_a_common_level(prec):
    """One bidirectional liGRU layer with BatchNorm (H = 24, T * B = 300) on an input with a common level - projection
    columns with |mean| >> std through the layer's own statistics path (GEMM + statistics + finalize of the gates'
    BatchNorms, and the BatchNorm backward of the projections) - against the oracle (fp32 at 1e-4; bf16 against the
    bf16-operand model at 5e-3 / 2e-2), the ReLU recurrence differentiated on the oracle's kink pattern.  fp32, like the
    other BatchNorm cases on such columns: every quantity is held to max(1e-4, 4 x e_ref), e_ref = the fp32 oracle's own
    distance from its fp64 run (2-3e-5 here; the host test holds 4 x e_ref under 1e-3)."""
    c = _rec_bn_case()
    ref = D.rec_reference(c, prec)
    e_ref = D.rec_batchnorm_e_ref(c) if prec == "fp32" else None
    F_.set_precision(prec)
    ye, dxe, got, report = _run_rec(c, ref)
    otol, gtol = (TOL, TOL) if prec == "fp32" else (5e-3, 2e-2)
    e_y, e_x = rel_err_rows(ye, ref.y, (1, 2)), rel_err_rows(dxe, ref.dx, (1, 2))  # per time step
    e_g = {k: rel_err(got[k], v) for k, v in ref.grads.items() if float(v.norm()) > 0}
    b_y, b_x, b_g = otol, gtol, {k: gtol for k in e_g}
    if e_ref is not None:
        b_y, b_x = max(otol, 4 * e_ref["y"]), max(gtol, 4 * e_ref["dx"])
        b_g = {k: max(gtol, 4 * e_ref["grads"][k]) for k in e_g}
    print("\nliGRU + BatchNorm on a common level, %s: y worst step %.1e, dx worst step %.1e, parameter gradients %s; e_ref %s; kinks %s"
          % (prec, float(e_y.max()), float(e_x.max()), {k: "%.1e" % v for k, v in e_g.items()},
             None if e_ref is None else {"y": "%.1e" % e_ref["y"], "dx": "%.1e" % e_ref["dx"], "grads": "%.1e" % max(e_ref["grads"].values())}, report))
    assert bool((e_y < b_y).all()), e_y
    assert bool((e_x < b_x).all()), e_x
    for k, v in e_g.items():
        assert v < b_g[k], (k, v, b_g[k])


# ------------------------------------------------------------------------------------------------
# C. log-softmax and the fused cost on extreme logits
# ------------------------------------------------------------------------------------------------
def _lsm_reference(c):
    xr = c.x.double().requires_grad_(True)
    yr = TF.log_softmax(xr, 1)
    (yr * c.cot.double()).sum().backward()
    dx_dy = xr.grad.clone()
    xr.grad = None
    loss = TF.nll_loss(TF.log_softmax(xr, 1), c.lab)
    (loss * 1.7).backward()
    return yr.detach(), dx_dy, float(loss), xr.grad.clone()


@pytest.mark.parametrize("rows,N", D.LSM_SHAPES)
def test_log_softmax_on_extreme_logits(rows, N):
    """F_.log_softmax forward and backward, and the pitched backward (pk_logsoftmax_bwd_ld) where it exists (N <= 2048), on
    rows of 4 randn | the same + 1e4 | 3e3 randn | one logit 200 above the rest | zeros | two equal maxima, per row
    against fp64: y at 1e-6, dx at 1e-5 (test_logsoftmax).  2100 classes take the generic kernels."""
    lib = _lib.load()
    c = D.logits_rows(rows, N)
    yr, dxr, _, _ = _lsm_reference(c)
    xe = c.x.clone().cuda().requires_grad_(True)
    y = F_.log_softmax(xe)
    (y * c.cot.cuda()).sum().backward()
    e_y, e_dx = rel_err_rows(y, yr, 1), rel_err_rows(xe.grad, dxr, 1)
    print("\nlog_softmax %dx%d rows [4 randn | + 1e4 | 3e3 randn | + 200 | zeros | tie]: y %s, dx %s" % (rows, N, _fmt(e_y), _fmt(e_dx)))
    assert bool((e_y < 1e-6).all()), e_y
    assert bool((e_dx < 1e-5).all()), e_dx
    if N <= 2048:
        ld = F_._up(N, 4)
        buf = torch.full((rows, ld), float("nan"), device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(lib.pk_logsoftmax_bwd_ld(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(c.cot.cuda()), p(y.detach()),
                                            rows, N, p(buf), ld), "pk_logsoftmax_bwd_ld")
        torch.cuda.synchronize()
        e_ld = rel_err_rows(buf[:, :N], dxr, 1)
        print("  pitched backward (pitch %d): dx %s" % (ld, _fmt(e_ld)))
        assert bool((e_ld < 1e-5).all()), e_ld
        assert ld == N or float(buf[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("rows,N", [s for s in D.LSM_SHAPES if s[1] <= 2048])
def test_fused_head_and_cost_on_extreme_logits(rows, N, monkeypatch):
    """The perf-mode head on the same logits: they are carried EXACTLY through the bf16 GEMM in front
    (degenerate_inputs.logits_as_head_operands), so pk_logsoftmax_fwd_ld_argmax, both cost kernels
    (pk_nll_err_fwd_argmax, pk_nll_err_fwd) and the bf16 gradient kernels (pk_logsoftmax_bwd_bf16,
    pk_nll_logsoftmax_bwd_bf16) see them as they are.  Against fp64 log_softmax / nll_loss: y per row at 1e-6, the loss at
    2e-6, the bias gradient (column sums of the unrounded dz) at 1e-5; the weight gradient holds every row of the bf16 dz
    by itself (selector rows in the GEMM's other operand) and is graded per row at the 8e-3 of a bf16 rounding.  Arg-max
    and error count exactly on rows without ties; on tied rows the index must be one of the maxima."""
    c = D.logits_rows(rows, N)
    yr, dz_dy, loss_r, dz_nll = _lsm_reference(c)
    xs, w = D.logits_as_head_operands(c.x)
    lab = c.lab.cuda()
    untied = ~c.tied
    arg_r = c.x.argmax(1)
    miss_untied = int((arg_r != c.lab)[untied].sum())
    lab_is_max = c.maxima[torch.arange(rows), c.lab]
    lo, hi = miss_untied + int((~lab_is_max)[c.tied].sum()), miss_untied + int(c.tied.sum())
    F_.set_precision("bf16")
    for mode in ("1", "0"):
        monkeypatch.setenv("PK_EXPERIMENT", "head_argmax=" + mode)
        # --- the cost behind the head
        xe, we, be = xs.clone().cuda().requires_grad_(True), w.clone().cuda().requires_grad_(True), torch.zeros(N, device="cuda", requires_grad=True)
        y = F_.linear_log_softmax(xe, we, be)
        amax = y._pk_head[-1].cpu().long()
        loss, stats = F_.head_nll(y, lab)
        (loss * 1.7).backward()
        torch.cuda.synchronize()
        e_y = rel_err_rows(y, yr, 1)
        dzb = torch.stack([we.grad[:, 3 * r] for r in range(rows)]).cpu()  # row r of the bf16 dz (x 1 in the GEMM)
        e_dz, e_db = rel_err_rows(dzb, dz_nll, 1), rel_err(be.grad, dz_nll.sum(0))
        e_loss = abs(float(loss) - loss_r) / abs(loss_r)
        n_err = float(stats[1]) * rows
        print("\nfused head %dx%d head_argmax=%s: y %s, loss %.1e, cost gradient rows (bf16) %s, bias gradient %.1e, errors %.0f in [%d, %d]"
              % (rows, N, mode, _fmt(e_y), e_loss, _fmt(e_dz), e_db, n_err, lo, hi))
        assert bool((e_y < 1e-6).all()), e_y
        assert e_loss < 2e-6, e_loss
        assert bool((e_dz < 8e-3).all()), e_dz
        assert e_db < 1e-5, e_db
        assert float(stats[2]) == rows and float(stats[3]) == 0
        assert torch.equal(amax[untied], arg_r[untied])
        assert bool(c.maxima[torch.arange(rows), amax].all())  # tied rows: one of the maxima
        assert lo <= round(n_err) <= hi and abs(n_err - round(n_err)) < 1e-4
        if mode == "1":
            assert round(n_err) == int((amax != c.lab).sum())
        # --- a dense gradient into the head's output (pk_logsoftmax_bwd_bf16)
        if mode == "1":
            xe, we, be = xs.clone().cuda().requires_grad_(True), w.clone().cuda().requires_grad_(True), torch.zeros(N, device="cuda", requires_grad=True)
            y = F_.linear_log_softmax(xe, we, be)
            (y * c.cot.cuda()).sum().backward()
            torch.cuda.synchronize()
            dzb = torch.stack([we.grad[:, 3 * r] for r in range(rows)]).cpu()
            e_dz, e_db = rel_err_rows(dzb, dz_dy, 1), rel_err(be.grad, dz_dy.sum(0))
            print("  dense gradient: dz rows (bf16) %s, bias gradient %.1e" % (_fmt(e_dz), e_db))
            assert bool((e_dz < 8e-3).all()), e_dz
            assert e_db < 1e-5, e_db
