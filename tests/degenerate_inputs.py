"""Seeded builders of degenerate and ill-conditioned inputs: zero-variance LayerNorm rows, BatchNorm columns whose
|mean| is far above their std, log-softmax rows that overflow exp() unless the maximum is subtracted first.

A plain module (not a conftest): tests/test_gpu_degenerate_rows.py feeds these inputs to the kernels, and
tests/test_degenerate_inputs_host.py runs the references alone on the very same tensors and asserts what makes the
GPU comparison meaningful (the references are finite, the degenerate rows are exactly degenerate, the columns are as
badly conditioned as intended, the references' own fp32 error leaves the tolerances room).

The constant rows hold 0 or 0.5: their partial sums are exact in fp32 in any summation order at every length used
here, so "variance exactly 0" does not depend on how a kernel adds."""
import importlib
from types import SimpleNamespace

import torch

from golden_util import rel_err_rows

# ------------------------------------------------------------------------------------------------
# A. LayerNorm
# ------------------------------------------------------------------------------------------------
LN_SHAPES = [(6, 7), (6, 550), (5, 3200)]
LN_ZERO, LN_HALF, LN_OFFSET, LN_SINGLE = 0, 1, 2, 3  # row numbers; the remaining rows are randn


def layernorm_rows(rows, F):
    """x [rows, F]: all zeros | all 0.5 | 1e3 + randn | one non-zero element | randn ..."""
    assert rows >= 5
    g = torch.Generator().manual_seed(1000 * rows + F)
    x = torch.randn(rows, F, generator=g)
    x[LN_ZERO] = 0.0
    x[LN_HALF] = 0.5
    x[LN_OFFSET] += 1e3
    x[LN_SINGLE] = 0.0
    x[LN_SINGLE, F // 3] = 1.75
    degenerate = torch.zeros(rows, dtype=torch.bool)
    degenerate[[LN_ZERO, LN_HALF]] = True
    return SimpleNamespace(x=x, gamma=torch.rand(F, generator=g) + 0.5, beta=torch.randn(F, generator=g),
                           cot=torch.randn(rows, F, generator=g), degenerate=degenerate)


CONV_TAIL_SHAPES = [(3, 5, 36), (2, 3, 130)]


def conv_tail_rows(B, C, L, drop):
    """z [B, C, L] as (b, c) rows of length L: two rows all zeros, one all 0.5, the others 2 * randn + 0.3 (what the
    tail of a conv layer sees when a channel's pooled output is constant over time)."""
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + L)
    z = torch.randn(B * C, L, generator=g) * 2 + 0.3
    rows = B * C
    zero, half = [1, rows - 2], [2]
    z[zero] = 0.0
    z[half] = 0.5
    degenerate = torch.zeros(rows, dtype=torch.bool)
    degenerate[zero + half] = True
    mask = ((torch.rand(B, C, L, generator=g) > 0.2).float() / 0.8) if drop else None
    return SimpleNamespace(z=z.view(B, C, L), gamma=torch.rand(C, L, generator=g) + 0.5, beta=torch.randn(C, L, generator=g) * 0.3,
                           cot=torch.randn(B, C, L, generator=g), mask=mask, degenerate=degenerate)


REC_CELLS = [("liGRU", "ligru", "relu"), ("RNN", "rnn", "relu"), ("LSTM", "lstm", "tanh"), ("GRU", "gru", "tanh"),
             ("minimalGRU", "minimalgru", "tanh")]
REC_T, REC_B, REC_D = 5, 3, 7
REC_ZERO_B = 1  # the sequence that holds the zero frame


# (cell, prefix, act, H, bidir, route): every route functional.rec_route can answer for a layer with per-step LayerNorm -
# fp32 step-wise, fp32 persistent (generation 2 for liGRU / RNN, 4 for the others), bf16 persistent - at H = 24, ...
REC_CASES = [(k, p, a, 24, bidir, route) for (k, p, a) in REC_CELLS for bidir in (True, False)
             for route in ("fp32-stepwise", "fp32-persistent", "bf16-persistent")]
# ... and the nine-workgroup row exchange (H = 550) once per kernel file: pk_rec.hip, pk_rec_persist2_f32.hip,
# pk_rec_persist4_f32.hip, pk_rec_persist2.hip, pk_rec_persist2_gru.hip
REC_CASES += [("liGRU", "ligru", "relu", 550, True, "fp32-stepwise"), ("liGRU", "ligru", "relu", 550, True, "fp32-persistent"),
              ("LSTM", "lstm", "tanh", 550, True, "fp32-persistent"), ("RNN", "rnn", "relu", 550, False, "bf16-persistent"),
              ("GRU", "gru", "tanh", 550, True, "bf16-persistent")]


def rec_opts(pre, lay, act, bn=False, ln=True, bidir=True, drop=0.2):
    n = len(lay)
    j = lambda v: ",".join([str(v)] * n)  # noqa: E731
    return {pre + "_lay": ",".join(map(str, lay)), pre + "_drop": j(drop), pre + "_use_laynorm_inp": "False",
            pre + "_use_batchnorm_inp": "False", pre + "_use_laynorm": j(ln), pre + "_use_batchnorm": j(bn),
            pre + "_bidir": str(bidir), pre + "_act": j(act), pre + "_orthinit": "True", "use_cuda": "True",
            "to_do": "train"}


def rec_zero_frame(kind, pre, act, H, bidir):
    """One recurrent layer with per-step LayerNorm (no BatchNorm, hence no projection bias) on T = 5, B = 3, D = 7 with ONE
    all-zero frame: the last frame of sequence 1 for a bidirectional layer (a zero-padded tail: the backward direction
    starts on it with h = 0), the first frame of sequence 1 for a unidirectional one.  The state of that first step is
    exactly 0 for every cell, so its LayerNorm sees a zero-variance row.  beta stays at its initial 0 (the rows behind the
    zero frame would otherwise start from h = beta and the case is no longer the padded one); gamma is moved off 1.
    `zero`: the (t, b) positions of the zero frame, the grading groups."""
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    T, B, D = REC_T, REC_B, REC_D
    opts = rec_opts(pre, [H], act, bidir=bidir)
    torch.manual_seed(99 + H)
    net = getattr(nn_amd, kind)(opts, D)
    with torch.no_grad():
        for name, q in net.named_parameters():
            if name.startswith("ln.") and name.endswith("gamma"):
                q.mul_(1.0 + 0.3 * torch.randn_like(q))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(5 + H)
    x = torch.randn(T, B, D, generator=g)
    t0 = T - 1 if bidir else 0
    x[t0, REC_ZERO_B] = 0.0
    zero = torch.zeros(T, B, dtype=torch.bool)
    zero[t0, REC_ZERO_B] = True
    # (O.make_drop_masks without importing the oracle here: one Bernoulli(1 - p) mask [rows, H], constant over time)
    masks = [torch.bernoulli(torch.full((2 * B if bidir else B, H), 0.8), generator=g)]
    cot = torch.randn(T, B, (2 if bidir else 1) * H, generator=g)
    return SimpleNamespace(kind=kind, opts=opts, net=net, sd=sd, x=x, masks=masks, cot=cot, zero=zero, t0=t0, D=D, H=H)


# ------------------------------------------------------------------------------------------------
# B. BatchNorm
# ------------------------------------------------------------------------------------------------
BN_SHAPES = [(2, 6), (65, 48), (257, 130), (1000, 70)]
BN_ZERO, BN_CONST, BN_100, BN_1000, BN_OUTLIER = 0, 1, 2, 3, 4  # column numbers; the others are 0.5 + 2 * randn


# the project's tolerance for each quantity (test_batchnorm_act_drop; 1e-5 for batch statistics), applied per column
BN_TOL = {"y": 1e-5, "dx": 1e-4, "dgamma": 1e-4, "dbeta": 1e-4, "running_mean": 1e-5, "running_var": 1e-5, "mean": 1e-5, "var": 1e-5}


def bn_graded(M):
    """The quantities graded at M rows.  With two rows xhat is +-1 up to eps / var and dx is what a cancellation to rounding
    level leaves (1e-5 of the terms that cancel): torch's own fp32 dx is up to 100 % off there (the host test prints it),
    there is nothing to grade against."""
    return [k for k in BN_TOL if not (M == 2 and k == "dx")]


# seeds for which the reference's own fp32 error meets the cap 4 x e_ref < 1e-3 on every graded column with both
# activations (tests/test_degenerate_inputs_host.py asserts it): a sum like dgamma = sum(g * xhat) can come out small by
# chance, and its relative error is then large whatever computes it
BN_SEEDS = {(2, 6): 20, (1000, 70): 1}  # (the other shapes: 7 * M + N)


def batchnorm_columns(M, N):
    """x [M, N]: constant 0 | constant 3.0 | 1e2 + randn | -1e3 + randn | randn with 100 in row 0 (the value a shifted sum
    pivots on) | 0.5 + 2 * randn ..."""
    assert N >= 6
    g = torch.Generator().manual_seed(BN_SEEDS.get((M, N), 7 * M + N))
    x = torch.randn(M, N, generator=g)
    x[:, 5:] = 0.5 + 2 * x[:, 5:]
    x[:, BN_ZERO] = 0.0
    x[:, BN_CONST] = 3.0
    x[:, BN_100] += 1e2
    x[:, BN_1000] -= 1e3
    x[0, BN_OUTLIER] = 100.0
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    beta[BN_CONST] = 1.0  # (the constant columns' output is act(beta): not a value next to 0, where a relative error says little)
    return SimpleNamespace(x=x, gamma=gamma, beta=beta, mask=torch.bernoulli(torch.full((M, N), 0.85), generator=g) / 0.85,
                           cot=torch.randn(M, N, generator=g))


def batchnorm_reference(c, act, dtype, relu_pattern=None):
    """torch's BatchNorm1d(momentum=0.05) -> act -> mask in `dtype` on the CPU.  -> dict of per-column-gradable tensors.
    relu_pattern: differentiate the ReLU on another run's pattern (pre-activation > 0), so that two evaluations that
    differ by rounding noise differentiate the same piecewise-linear function."""
    x = c.x.detach().clone().to(dtype).requires_grad_(True)
    bn = torch.nn.BatchNorm1d(x.shape[1], momentum=0.05).to(dtype)
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
    pre = bn(x)
    if act == "relu" and relu_pattern is not None:
        lin = pre * relu_pattern.to(dtype)
        a = lin + (torch.relu(pre) - lin).detach()
    else:
        a = torch.relu(pre) if act == "relu" else torch.tanh(pre)
    y = a * c.mask.to(dtype)
    (y * c.cot.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": x.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
            "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(),
            "mean": x.detach().mean(0), "var": x.detach().var(0, unbiased=False), "relu": (pre.detach() > 0)}


def affine_bound(mean, var, gamma, eps, y_ref, gain=1.0):
    """What the engine's form of the normalisation, y = act(x * scale + shift) with scale = gamma / sqrt(var + eps) and
    shift = beta - mean * scale (one multiply-add per element, pk_affine_act_fwd and the one-launch layers), can lose per
    column by its arithmetic alone, as a norm-relative error of the column of y_ref [M, N]: the batch mean is rounded to
    fp32 (half an ulp of |mean|), so is the product mean * scale, so is shift - three half ulps of |mean|, times |scale|,
    as a common offset of the column's pre-activation; an activation of slope <= 1 and a mask of at most `gain` pass it
    on.  (A rounding error of scale itself enters x * scale and mean * scale alike and cancels to the size of xhat.)
    Computed from the fp64 reference alone.  This is eps_fp32 * |mean| / std: 1e-5 at |mean| = 100 std, 1e-4 at 1000 - the
    loss the form accepts; torch's CPU kernel normalises (x - mean) * invstd and does not have it, so 4 x its error does
    not cover the form.  A one-pass variance is 0.25 % / 23 % off on the same columns."""
    mean, var, gamma = mean.double(), var.double(), gamma.double()
    ulp = torch.where(mean == 0, torch.zeros_like(mean), 2.0 ** (torch.floor(torch.log2(mean.abs().clamp_min(1e-300))) - 23))
    off = 1.5 * ulp * (gamma / (var + eps).sqrt()).abs() * gain
    M = y_ref.shape[0]
    den = y_ref.double().norm(dim=0)
    return off * M ** 0.5 / torch.where(den == 0, torch.ones_like(den), den)


# the smallest shape the bf16 GEMM runs on its 256-tile (M >= 16384 rows, N >= 1024: statistics in the epilogue), and 300
# rows (the fallback: plain GEMM + pk_bn_stats)
PROJ_SHAPES = [(16384, 1024, 40), (300, 70, 40)]
SMALL_BATCH_CASES = [(128, 256, 440, "relu", True), (37, 200, 520, "tanh", False)]  # M, N, K, act, masked


def proj_level(K):
    """The common level of x for which a column of x w^T, w = (1 + randn) / sqrt(K), has |mean| = 100 std:
    mean = level * sum(w) ~ level * sqrt(K), std = |w| ~ sqrt(2)."""
    return 100.0 * (2.0 / K) ** 0.5


def projection_operands(M, N, K):
    """x [M, K] at a common level and w [N, K] with a common component: the columns of x w^T have a mean of about 100 x
    their standard deviation (what a projection of un-normalised filter-bank energies looks like)."""
    g = torch.Generator().manual_seed(M + N + K)
    x = proj_level(K) + torch.randn(M, K, generator=g)
    w = (1.0 + torch.randn(N, K, generator=g)) / K ** 0.5
    return x, w


def small_batch_layer(M, N, K, act, masked):
    """drop(act(bn(x w^T + b))) of one small-batch layer on projection_operands: the operands, and the fp64 evaluation on the
    bf16-rounded operands - z, batch mean / biased variance, activation a, output y - with e_ref = the per-column error
    of torch's fp32 BatchNorm + activation on the fp32-rounded z."""
    import torch.nn.functional as TF

    x, w = projection_operands(M, N, K)
    g = torch.Generator().manual_seed(M * N)
    bias, gamma, beta = torch.randn(N, generator=g), 1 + 0.1 * torch.randn(N, generator=g), torch.randn(N, generator=g)
    mask = ((torch.rand(M, N, generator=g) > 0.15).float() / 0.85) if masked else None
    rb = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    z = rb(x) @ rb(w).t() + bias.double()
    mu, var = z.mean(0), z.var(0, unbiased=False)
    actf = (lambda t: t.clamp_min(0)) if act == "relu" else torch.tanh
    a = actf((z - mu) / (var + 1e-5).sqrt() * gamma.double() + beta.double())
    a32 = actf(TF.batch_norm(z.float(), None, None, gamma, beta, True, 0.05, 1e-5)).double()
    e_ref = rel_err_rows(a32, a, 0)
    y = a * mask.double() if masked else a
    return SimpleNamespace(x=x, w=w, bias=bias, gamma=gamma, beta=beta, mask=mask, z=z, mean=mu, var=var, a=a, y=y, e_ref=e_ref,
                           aff_a=affine_bound(mu, var, gamma, 1e-5, a), aff_y=affine_bound(mu, var, gamma, 1e-5, y, 1 / 0.85),
                           ratio=float((mu.abs() / var.sqrt()).median()))


def rec_batchnorm_offset(H=24, T=20, B=15, D=1024):
    """One bidirectional liGRU layer with BatchNorm (T * B = 300 rows) on an input with a common level: the projections'
    columns have |mean| ~ 75 std.  The input is wide (D = 1024) so that the level itself stays low (2.6 std of x): an
    error of the projection gradient dP is not mean-free over the rows and enters dW = dP^T x times level / std(x) - at
    D = 7 (level 53) the oracle's own fp32 weight gradients are 3-6e-4 from its fp64 run, at this width 1-3e-5."""
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    opts = rec_opts("ligru", [H], "relu", bn=True, ln=False, bidir=True)
    torch.manual_seed(123)
    net = nn_amd.liGRU(opts, D)
    with torch.no_grad():  # a common component in the projection weights (see projection_operands)
        for name, q in net.named_parameters():
            if name.startswith(("wh.", "wz.")) and name.endswith("weight"):
                q.add_(1.0 / D ** 0.5)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    x = 0.6 * proj_level(D) + torch.randn(T, B, D, generator=g)
    masks = [torch.bernoulli(torch.full((2 * B, H), 0.8), generator=g)]
    cot = torch.randn(T, B, 2 * H, generator=g)
    return SimpleNamespace(kind="liGRU", opts=opts, net=net, sd=sd, x=x, masks=masks, cot=cot, D=D, H=H)


def rec_batchnorm_e_ref(c):
    """The fp32 oracle's own distance from its fp64 run on rec_batchnorm_offset (same ReLU pieces): y / dx worst time step,
    every parameter gradient."""
    from golden_util import rel_err

    r32 = rec_reference(c, "fp32")
    r64 = rec_reference(c, "fp32", torch.float64, kinks=r32.log)
    return {"y": float(rel_err_rows(r32.y, r64.y, (1, 2)).max()), "dx": float(rel_err_rows(r32.dx, r64.dx, (1, 2)).max()),
            "grads": {k: rel_err(r32.grads[k], v) for k, v in r64.grads.items() if float(v.norm()) > 0}}


# ------------------------------------------------------------------------------------------------
# C. log-softmax
# ------------------------------------------------------------------------------------------------
LSM_SHAPES = [(6, 48), (6, 200), (6, 1938), (6, 2048), (6, 2100)]
LSM_CONTROL, LSM_SHIFTED, LSM_WIDE, LSM_PEAK, LSM_ZERO, LSM_TIE = range(6)  # row numbers


def logits_rows(rows, N):
    """x [6, N]: 4 * randn | the same + 1e4 | 3e3 * randn | one logit 200 above the rest | all zeros | two equal maxima.
    -> x, cot, labels, tied (rows whose maximum is not unique: the last two), maxima (bool [rows, N])."""
    assert rows == 6
    g = torch.Generator().manual_seed(31 * N)
    x = torch.randn(rows, N, generator=g) * 4
    x[LSM_SHIFTED] = x[LSM_CONTROL] + 1e4
    x[LSM_WIDE] *= 750.0
    x[LSM_PEAK, N // 2] = x[LSM_PEAK].max() + 200.0
    x[LSM_ZERO] = 0.0
    top = x[LSM_TIE].max() + 1.0
    x[LSM_TIE, N // 5] = top
    x[LSM_TIE, N - 3] = top
    lab = torch.randint(0, N, (rows,), generator=g)
    # the rows whose softmax is one-hot to fp32 precision are labelled as misses: on a hit the cost's gradient is what
    # exp() leaves below the fp32 range (1e-87 in fp64, 0 in fp32) and there is nothing to grade
    lab[LSM_PEAK] = N // 2 + 1
    lab[LSM_WIDE] = (int(x[LSM_WIDE].argmax()) + 1) % N
    lab[LSM_TIE] = N - 3            # the later of the two maxima
    maxima = x == x.max(1, keepdim=True).values
    return SimpleNamespace(x=x, cot=torch.randn(rows, N, generator=g), lab=lab, tied=maxima.sum(1) > 1, maxima=maxima)


def logits_as_head_operands(x):
    """(xs [rows, 3 * rows], w [N, 3 * rows]) whose bf16 product xs w^T is EXACTLY the fp32 matrix x: every logit is split
    into three bf16 parts (8 + 8 + 8 mantissa bits) that the selector rows of xs add up again - in fp32, exactly, in any
    order.  This carries arbitrary fp32 logits through the bf16 GEMM in front of the fused head."""
    rows, N = x.shape
    parts, rest = [], x.clone()
    for _ in range(3):
        p = rest.to(torch.bfloat16).float()
        parts.append(p)
        rest = rest - p
    assert float(rest.abs().max()) == 0.0
    xs = torch.zeros(rows, 3 * rows)
    w = torch.zeros(N, 3 * rows)
    for r in range(rows):
        for k in range(3):
            xs[r, 3 * r + k] = 1.0
            w[:, 3 * r + k] = parts[k][r]
    return xs, w


# ------------------------------------------------------------------------------------------------
# references (the oracle / torch on the CPU), shared by the host test and the GPU tests
# ------------------------------------------------------------------------------------------------
def rec_reference(c, prec="fp32", dtype=torch.float32, kinks=None):
    """The oracle on a recurrent case: fp32 (or `dtype`), or its bf16-operand model.  ReLU cells log their kink pattern
    (`log`), which a second evaluation takes as `kinks`.  -> y, dx, parameter gradients, log."""
    import contextlib

    import pk_oracle as O

    osd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in c.sd.items()}
    for k, v in osd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    xo = c.x.clone().to(dtype).requires_grad_(True)
    relu = "relu" in "".join(v for k, v in c.opts.items() if k.endswith("_act"))
    log = [] if (relu and kinks is None) else None
    with (O.bf16_operands() if prec == "bf16" else contextlib.nullcontext()):
        yo = O.recurrent_forward(c.kind, c.opts, osd, xo, training=True, to_do="train", drop_masks=c.masks, kinks=kinks,
                                 kink_log=log)
        (yo * c.cot.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in osd.items() if v.requires_grad and v.grad is not None}
    return SimpleNamespace(y=yo.detach(), dx=xo.grad, grads=grads, log=log)
