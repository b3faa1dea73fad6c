"""The inputs of tests/test_gpu_degenerate_rows.py, checked on the references alone (no GPU): the oracle / torch are
finite on them in fp32 and fp64, the rows meant to be degenerate are exactly degenerate, the ill-conditioned columns are
as ill-conditioned as intended, and the references' own fp32-vs-fp64 deviation e_ref leaves the tolerances derived from
it something to say (4 x e_ref < 1e-3 for every graded BatchNorm column).  Also the two grading helpers."""
import math

import pytest
import torch
import torch.nn.functional as TF

import degenerate_inputs as D
import pk_oracle as O
from golden_util import rel_err, rel_err_rows, rel_err_split


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


# ------------------------------------------------------------------------------------------------
# the graders
# ------------------------------------------------------------------------------------------------
def test_rel_err_rows_grades_every_slice_by_itself():
    b = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1e6, 0.0]])
    a = b.clone()
    a[0, 0] += 0.5
    a[1, 1] = 0.25
    a[2, 0] += 1.0
    e = rel_err_rows(a, b, 1)
    assert e.tolist() == pytest.approx([0.1, 0.25, 1e-6])       # a zero reference row is graded absolutely, like rel_err
    assert rel_err_rows(a, b, 0).tolist() == pytest.approx([math.sqrt(0.25 + 1.0) / math.sqrt(9.0 + 1e12), 0.25 / 4.0])
    assert float(rel_err_rows(a.view(3, 1, 2), b.view(3, 1, 2), (1, 2))[0]) == pytest.approx(0.1)
    a[2, 1] = float("nan")
    e = rel_err_rows(a, b, 1)
    assert math.isnan(float(e[2])) and not bool((e < 1e9).all())  # a NaN cannot pass a `< tol`
    assert bool((e[:2] < 1.0).all())


def test_rel_err_split_keeps_the_groups_from_hiding_each_other():
    g = torch.Generator().manual_seed(0)
    b = torch.randn(6, 10, generator=g)
    b[1] *= 1e6
    a = b.clone()
    a[4] *= 1.5                                   # an ordinary row 50 % off ...
    mask = torch.zeros(6, dtype=torch.bool)
    mask[1] = True
    assert rel_err(a, b) < 1e-6                   # ... vanishes next to the 1e6-sized row in a whole-tensor norm,
    e_big, e_rest = rel_err_split(a, b, mask)
    assert e_big == 0.0 and e_rest > 0.1          # and shows in its own group
    a = b.clone()
    a[1, 3] = float("nan")
    e_big, e_rest = rel_err_split(a, b, mask)
    assert math.isnan(e_big) and not (e_big < 1.0) and e_rest == 0.0
    m2 = torch.zeros(2, 3, dtype=torch.bool)      # a mask over two leading dimensions ((t, b) positions)
    m2[0, 1] = True
    e_big, e_rest = rel_err_split(a.view(2, 3, 10), b.view(2, 3, 10), m2)
    assert math.isnan(e_big) and e_rest == 0.0
    with pytest.raises(AssertionError):
        rel_err_split(a, b, torch.zeros(6, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------
# A. LayerNorm
# ------------------------------------------------------------------------------------------------
def _exact_partial_sums(v):
    """Every partial sum of a constant row is exact in fp32: the value times any count up to the length is representable."""
    n, val = v.numel(), float(v[0])
    return all(float(torch.tensor(val * k, dtype=torch.float32)) == val * k for k in (1, 2, 3, n // 2, n - 1, n)) and \
        float(torch.tensor(val * n, dtype=torch.float32) / n) == val


@pytest.mark.parametrize("rows,F", D.LN_SHAPES)
def test_layernorm_rows_are_what_they_claim(rows, F):
    c = D.layernorm_rows(rows, F)
    assert bool((c.x[D.LN_ZERO] == 0).all()) and bool((c.x[D.LN_HALF] == 0.5).all()) and _exact_partial_sums(c.x[D.LN_HALF])
    assert int((c.x[D.LN_SINGLE] != 0).sum()) == 1
    assert c.degenerate.tolist() == [i in (D.LN_ZERO, D.LN_HALF) for i in range(rows)]
    out = {}
    for dt in (torch.float32, torch.float64):
        xr, gr, br = (t.detach().clone().to(dt).requires_grad_(True) for t in (c.x, c.gamma, c.beta))
        y = O.layer_norm(xr, gr, br)
        (y * c.cot.to(dt)).sum().backward()
        assert _finite(y, xr.grad, gr.grad, br.grad), dt
        std = xr.detach().std(1)
        assert float(std[D.LN_ZERO]) == 0.0 and float(std[D.LN_HALF]) == 0.0 and bool((std[2:] > 0).all())
        out[dt] = (y.detach(), xr.grad)
    x64 = c.x.double()
    assert float(x64[D.LN_OFFSET].mean().abs() / x64[D.LN_OFFSET].std()) > 500
    # the reference's gradient on a zero-variance row: rinv * (g - mean(g)), rinv = 1 / eps
    gq = c.cot.double() * c.gamma.double()
    for r in (D.LN_ZERO, D.LN_HALF):
        assert rel_err(out[torch.float64][1][r], 1e6 * (gq[r] - gq[r].mean())) < 1e-12
    e_y, e_dx = rel_err_rows(out[torch.float32][0], out[torch.float64][0], 1), rel_err_rows(out[torch.float32][1], out[torch.float64][1], 1)
    print("\nlayer_norm %dx%d, torch fp32 vs fp64 per row: y %s, dx %s" % (rows, F, e_y.tolist(), e_dx.tolist()))
    ordinary = [i for i in range(rows) if i != D.LN_OFFSET]
    assert bool((e_y[ordinary] < 1e-6).all()) and bool((e_dx[ordinary] < 1e-6).all())


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("B,C,L", D.CONV_TAIL_SHAPES)
def test_conv_tail_rows_are_what_they_claim(B, C, L, act, drop):
    c = D.conv_tail_rows(B, C, L, drop)
    rows = c.z.reshape(B * C, L)
    assert int(c.degenerate.sum()) == 3 and (c.mask is not None) == drop
    for r in torch.nonzero(c.degenerate).reshape(-1):
        assert bool((rows[r] == rows[r, 0]).all()) and float(rows[r, 0]) in (0.0, 0.5) and _exact_partial_sums(rows[r])
    assert bool((rows[~c.degenerate].std(1) > 0.5).all())
    res = {}
    for dt in (torch.float32, torch.float64):
        zr, gr, br = (t.detach().clone().to(dt).requires_grad_(True) for t in (c.z, c.gamma, c.beta))
        y = O.activation(act, O.layer_norm(zr, gr, br))
        if drop:
            y = y * c.mask.to(dt)
        (y * c.cot.to(dt)).sum().backward()
        assert _finite(y, zr.grad, gr.grad, br.grad), dt
        res[dt] = (y.detach(), zr.grad)
    e = rel_err_split(res[torch.float32][1].reshape(B * C, L), res[torch.float64][1].reshape(B * C, L), c.degenerate)
    assert max(e) < 2e-6 and float(rel_err_rows(res[torch.float32][0].reshape(B * C, L), res[torch.float64][0].reshape(B * C, L), 1).max()) < 1e-6


REC_INPUTS = sorted({(k, p, a, H, bidir) for (k, p, a, H, bidir, _r) in D.REC_CASES})


@pytest.mark.parametrize("kind,pre,act,H,bidir", REC_INPUTS)
def test_zero_frame_cases_are_what_they_claim(kind, pre, act, H, bidir):
    """The oracle on the zero-frame cases: finite everywhere in fp32, fp64 and in the bf16-operand model; the state of
    the step that starts on the zero frame is exactly constant (its LayerNorm output, gamma * (h - mean) / (std + eps) +
    0, is exactly 0 in every unit); the fp32 oracle is within a quarter of the GPU tolerance of its own fp64 run in both
    grading groups, so the 1e-4 asked of the kernels is not vacuous."""
    c = D.rec_zero_frame(kind, pre, act, H, bidir)
    assert int(c.zero.sum()) == 1 and bool((c.x[c.zero] == 0).all()) and bool((c.x[~c.zero].abs().sum(-1) > 0).all())
    assert all(float(v.abs().max()) == 0.0 for k, v in c.sd.items() if k.startswith("ln.") and k.endswith("beta"))
    assert not any(k.endswith(".bias") for k in c.sd if k.startswith("w"))
    r32 = D.rec_reference(c, "fp32")
    r64 = D.rec_reference(c, "fp32", torch.float64, kinks=r32.log)
    rbf = D.rec_reference(c, "bf16")
    for r in (r32, r64, rbf):
        assert _finite(r.y, r.dx, *r.grads.values())
        started = r.y[c.zero][0, H:] if bidir else r.y[c.zero][0]
        assert float(started.abs().max()) == 0.0
    assert any(k.startswith("ln.") for k in r32.grads)
    ey, ex = rel_err_split(r32.y, r64.y, c.zero), rel_err_split(r32.dx, r64.dx, c.zero)
    eg = max(rel_err(r32.grads[k], v) for k, v in r64.grads.items() if float(v.norm()) > 0)
    print("\n%s H=%d bidir=%s: max |dx| %.1e, largest parameter gradient %.1e; oracle fp32 vs fp64: y %s, dx %s, parameters %.1e"
          % (kind, H, bidir, float(r64.dx.abs().max()), max(float(v.abs().max()) for v in r64.grads.values()), ey, ex, eg))
    assert max(ey) < 2.5e-5 and max(ex) < 2.5e-5 and eg < 2.5e-5


# ------------------------------------------------------------------------------------------------
# B. BatchNorm
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("M,N", D.BN_SHAPES)
def test_batchnorm_columns_are_what_they_claim(M, N, act):
    BN_TOL, bn_graded = D.BN_TOL, D.bn_graded
    c = D.batchnorm_columns(M, N)
    x64 = c.x.double()
    assert bool((c.x[:, D.BN_ZERO] == 0).all()) and bool((c.x[:, D.BN_CONST] == 3.0).all())
    assert float(torch.tensor(3.0 * M, dtype=torch.float32)) == 3.0 * M
    ratio = x64.mean(0).abs() / x64.std(0, unbiased=False).clamp_min(1e-300)
    assert float(ratio[D.BN_100]) > 50 and float(ratio[D.BN_1000]) > 500
    assert float(c.x[0, D.BN_OUTLIER]) == 100.0
    r64 = D.batchnorm_reference(c, act, torch.float64)
    r32 = D.batchnorm_reference(c, act, torch.float32, relu_pattern=r64["relu"])
    for r in (r32, r64):
        assert _finite(*[v.double() for v in r.values()])
    worst = {}
    for k in bn_graded(M):
        a, b = r32[k], r64[k]
        e_ref = rel_err_rows(a, b, 0) if a.dim() == 2 else rel_err_rows(a.reshape(1, -1), b.reshape(1, -1), 0)
        worst[k] = float(e_ref.max())
        # the cap that keeps max(tolerance, 4 x e_ref) honest: a condition on the inputs, checked on the reference alone
        assert bool((4 * e_ref < 1e-3).all()), (k, e_ref)
    print("\nBatchNorm %dx%d %s: |mean| / std of the 1e2 / -1e3 columns %.0f / %.0f; worst e_ref per quantity %s"
          % (M, N, act, float(ratio[D.BN_100]), float(ratio[D.BN_1000]), {k: "%.1e" % v for k, v in worst.items()}))
    assert set(BN_TOL) >= set(worst)
    aff = D.affine_bound(r64["mean"], r64["var"], c.gamma, 1e-5, r64["y"], float(c.mask.max()))
    print("  affine-form bound on y, columns [0 | 3.0 | 1e2 | -1e3 | outlier | plain]: %s" % ["%.1e" % float(aff[j]) for j in range(6)])
    assert float(aff[D.BN_ZERO]) == 0.0 and bool((aff < 1e-3).all())  # like 4 x e_ref: a bound that still says something


@pytest.mark.parametrize("M,N,K", D.PROJ_SHAPES)
def test_projection_operands_have_the_common_level(M, N, K):
    x, w = D.projection_operands(M, N, K)
    C = x.to(torch.bfloat16).double() @ w.to(torch.bfloat16).double().t()
    ratio = C.mean(0).abs() / C.std(0, unbiased=False)
    print("\nprojection %dx%dx%d: |mean| / std of the product columns: median %.0f, min %.0f" % (M, N, K, float(ratio.median()), float(ratio.min())))
    assert _finite(C) and float(ratio.median()) > 50


@pytest.mark.parametrize("M,N,K,act,masked", D.SMALL_BATCH_CASES)
def test_small_batch_layer_reference(M, N, K, act, masked):
    s = D.small_batch_layer(M, N, K, act, masked)
    print("\nsmall-batch layer %dx%dx%d: |mean| / std %.0f, worst e_ref %.1e" % (M, N, K, s.ratio, float(s.e_ref.max())))
    assert _finite(s.z, s.a, s.y) and s.ratio > 50
    assert bool((4 * s.e_ref < 1e-3).all())
    # the bound derived from the x * scale + shift form stays a bound: under 1e-3 on every column (twice that between forms)
    print("  affine-form bound per column: a worst %.1e, y worst %.1e" % (float(s.aff_a.max()), float(s.aff_y.max())))
    assert bool((s.aff_a < 1e-3).all()) and bool((s.aff_y < 1e-3).all())


def test_recurrent_batchnorm_case_reference():
    c = D.rec_batchnorm_offset()
    r32 = D.rec_reference(c, "fp32")
    r64 = D.rec_reference(c, "fp32", torch.float64, kinks=r32.log)
    rbf = D.rec_reference(c, "bf16")
    for r in (r32, r64, rbf):
        assert _finite(r.y, r.dx, *r.grads.values())
    # the projections' columns: |mean| >> std
    T, B, Dm = c.x.shape
    xx = torch.cat([c.x, torch.flip(c.x, [0])], 1).reshape(2 * T * B, Dm).double()
    P = xx @ c.sd["wh.0.weight"].double().t()
    ratio = float((P.mean(0).abs() / P.std(0)).median())
    e = D.rec_batchnorm_e_ref(c)
    worst = max([e["y"], e["dx"]] + list(e["grads"].values()))
    print("\nliGRU + BatchNorm on a common level: |mean| / std of the candidate projection %.0f; oracle fp32 vs fp64: y %.1e, dx %.1e "
          "(worst step), parameter gradients %s" % (ratio, e["y"], e["dx"], {k: "%.1e" % v for k, v in e["grads"].items()}))
    assert ratio > 50
    assert 4 * worst < 1e-3   # the cap on max(1e-4, 4 x e_ref); in fact 4 x e_ref stays within 1.2e-4
    assert 4 * worst < 1.5e-4


# ------------------------------------------------------------------------------------------------
# C. log-softmax
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,N", D.LSM_SHAPES)
def test_logits_rows_are_what_they_claim(rows, N):
    c = D.logits_rows(rows, N)
    x = c.x
    assert c.tied.tolist() == [False, False, False, False, True, True]
    assert int(c.maxima[D.LSM_TIE].sum()) == 2 and int(c.maxima[D.LSM_ZERO].sum()) == N
    assert float(x[D.LSM_SHIFTED].min()) > 9e3 and float(x[D.LSM_WIDE].abs().max()) > 5e3
    top2 = x[D.LSM_PEAK].topk(2).values
    assert float(top2[0] - top2[1]) == pytest.approx(200.0, abs=1e-3)
    assert not _finite(torch.exp(x[D.LSM_SHIFTED])) and not _finite(torch.exp(x[D.LSM_WIDE]))  # exp() overflows without the shift
    for dt in (torch.float32, torch.float64):
        xr = x.detach().clone().to(dt).requires_grad_(True)
        y = TF.log_softmax(xr, 1)
        (y * c.cot.to(dt)).sum().backward()
        loss = TF.nll_loss(TF.log_softmax(x.to(dt), 1), c.lab)
        assert _finite(y, xr.grad, loss)
    assert bool((c.lab >= 0).all()) and bool((c.lab < N).all())
    assert int(c.lab[D.LSM_PEAK]) != int(x[D.LSM_PEAK].argmax()) and int(c.lab[D.LSM_WIDE]) != int(x[D.LSM_WIDE].argmax())
    # the logits travel exactly through a bf16 product
    xs, w = D.logits_as_head_operands(x)
    assert torch.equal(xs.to(torch.bfloat16).float(), xs) and torch.equal(w.to(torch.bfloat16).float(), w)
    assert torch.equal((xs.double() @ w.double().t()).float(), x) and torch.equal(xs @ w.t(), x)
