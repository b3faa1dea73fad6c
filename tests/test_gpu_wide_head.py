"""The fused output head (functional.linear_log_softmax / head_nll) for 2049 .. 8192 classes - the ~3400 senones of the
Librispeech recipes - on the block-per-row kernels of pk_norm.hip: the kernels through the C ABI between NaN guard bands,
graded per element against fp64; the same kernels against the wave-per-row ones they extend (PK_EXPERIMENT head_block=1
at widths both families cover); the autograd nodes against torch on the same output; degenerate logits; two heads on
one input (the concatenated dz operand with a slice wider than 2048 columns); the MLP class through forward_model; and
a captured training step.  Small rows and tiny K throughout: the widths are what matters."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as TF

import degenerate_inputs as D
from golden_util import rel_err, rel_err_rows

pytestmark = pytest.mark.gpu
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
U = importlib.import_module("pytorch-kaldi_amd.utils")

GUARD = 64  # elements on either side of a guarded buffer (256 bytes of floats, 128 of bf16: the middle stays 16-byte aligned)
# The grid policy (pk_norm.hip): a row per block up to 2048 blocks forward, 1024 backward.  The six widths the kernels
# must cover, with few rows; and (2050, 2049), the shape with more rows than launched blocks in both directions: blocks
# 0 and 1 take a second row forward, every block a second row (blocks 0 and 1 a third) backward.
SHAPES = [(1, 2049), (3, 2056), (5, 3400), (2, 4097), (3, 8191), (2, 8192), (2050, 2049)]


@pytest.fixture(autouse=True)
def _modes(monkeypatch):
    monkeypatch.delenv("PK_EXPERIMENT", raising=False)
    F_.set_precision("fp32")
    yield
    F_.set_precision("fp32")
    F_._DxShare.on = True
    F_.settings.fused_cost = True


def _guarded(n, dtype=torch.float32, fill=None):
    """A device buffer of n elements with GUARD elements of NaN (int32: -7) on both sides -> (whole buffer, the middle)."""
    bad = -7 if dtype == torch.int32 else float("nan")
    buf = torch.full((n + 2 * GUARD,), bad, device="cuda", dtype=dtype)
    mid = buf[GUARD:GUARD + n]
    assert mid.data_ptr() % 16 == 0
    if fill is not None:
        mid.copy_(fill.reshape(-1))
    return buf, mid


def _guards_intact(buf, n):
    lo, hi = buf[:GUARD], buf[GUARD + n:]
    if buf.dtype == torch.int32:
        return bool((lo == -7).all()) and bool((hi == -7).all())
    return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _first_max(y):
    """Arg-max by the kernels' rule: the first index of the row maximum; a row with a NaN: 0."""
    y = y.cpu()
    nan = torch.isnan(y).any(1)
    first = (torch.nan_to_num(y, nan=0.0) == torch.nan_to_num(y, nan=0.0).max(1, keepdim=True).values).float().argmax(1)
    return torch.where(nan, torch.zeros_like(first), first)


def _forward(x, N, ldx):
    """pk_logsoftmax_fwd_ld_argmax on x [rows, N] laid out at pitch ldx with NaN pad columns -> y [rows, N], amax (cpu)."""
    lib = _lib.load()
    rows = x.shape[0]
    xp = torch.full((rows, ldx), float("nan"))
    xp[:, :N] = x
    xbuf, xm = _guarded(rows * ldx, fill=xp)
    ybuf, ym = _guarded(rows * N)
    abuf, am = _guarded(rows, torch.int32)
    _lib.check(lib.pk_logsoftmax_fwd_ld_argmax(_st(), _p(xm), ldx, rows, N, _p(ym), _p(am)), "pk_logsoftmax_fwd_ld_argmax")
    torch.cuda.synchronize()
    assert _guards_intact(ybuf, rows * N) and _guards_intact(abuf, rows) and _guards_intact(xbuf, rows * ldx)
    return ym.reshape(rows, N).cpu(), am.cpu().long()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,N", SHAPES)
def test_forward_kernel_between_guard_bands(rows, N):
    """y per row against fp64 log_softmax of the same fp32 logits at 1e-6 (tests/test_gpu_degenerate_rows.py), the pad
    columns of the pitched input (NaN here) read into nothing, nothing written outside y and amax; amax exact on
    tie-free rows, the FIRST index on small-integer logits built to tie, 0 on a row with a NaN.  Row 0 lies beyond
    LSM_FAR (a common level of 1e3)."""
    g = torch.Generator().manual_seed(rows * 7 + N)
    ldx = F_._up(N, 32)
    x = torch.randn(rows, N, generator=g) * 4
    x[0] += 1e3
    yr = TF.log_softmax(x.double(), 1)
    y, amax = _forward(x, N, ldx)
    e_y = rel_err_rows(y, yr, 1)
    print("\nforward %dx%d (pitch %d): worst row %.2e" % (rows, N, ldx, float(e_y.max())))
    assert bool((e_y < 1e-6).all()), e_y.max()
    untied = (x == x.max(1, keepdim=True).values).sum(1) == 1
    assert bool(untied.any())
    assert torch.equal(amax[untied], x.argmax(1)[untied])
    assert torch.equal(amax, _first_max(y))
    # logits that tie constantly, and a NaN in the last row (not in its first column)
    xt = torch.randint(-2, 3, (rows, N), generator=g).float() * 0.5
    y, amax = _forward(xt, N, ldx)
    assert int(((y == y.max(1, keepdim=True).values).sum(1) > 1).sum()) == rows   # every row ties
    assert torch.equal(amax, _first_max(y))
    assert bool((rel_err_rows(y, TF.log_softmax(xt.double(), 1), 1) < 1e-6).all())
    xt[rows - 1, N // 3 + 1] = float("nan")
    y, amax = _forward(xt, N, ldx)
    assert bool(torch.isnan(y[rows - 1]).all()) and int(amax[rows - 1]) == 0
    assert torch.equal(amax, _first_max(y))
    assert not bool(torch.isnan(y[:rows - 1]).any())


def _backward_inputs(rows, N):
    g = torch.Generator().manual_seed(rows * 5 + N)
    x = torch.randn(rows, N, generator=g) * 3
    x[0, N // 2] += 40.0               # p -> 1 in this row
    if rows > 1:
        x[1] += 1e3                    # a far row
    y = TF.log_softmax(x.double(), 1).float()
    dy = torch.randn(rows, N, generator=g)
    lab = torch.randint(0, N, (rows,), generator=g)
    lab[0] = N // 2 + 1                # (a miss: on a hit the gradient of the p -> 1 row is below the fp32 range)
    if rows >= 3:
        lab[rows - 1] = -100           # ignored
        lab[rows - 2] = N + 3          # out of range: counted by the forward pass, a zero row here
    if rows >= 2000:
        lab[5::7] = -100
    return y, dy, lab


def _run_backward(onehot, pitched, y, dy, lab, dloss=1.7):
    """-> dz [rows, ldb] (float, from the bf16 bits), column sums [N], count of valid labels"""
    lib = _lib.load()
    rows, N = y.shape
    ldb = F_._up(N, 64)
    pitch = ldb + 64 if pitched else ldb
    dbuf, dm = _guarded(rows * pitch, torch.bfloat16)   # NaN-filled: the neighbour slice [ldb, pitch) must stay NaN
    nws = int(lib.pk_logsoftmax_bwd_bf16_partial_floats(rows, N))
    pbuf, pm = _guarded(nws)
    cbuf, cm = _guarded(N)
    yd, dyd, labd = y.cuda(), dy.cuda(), lab.cuda()
    valid = (lab >= 0) & (lab < N)
    cnt = torch.tensor([float(valid.sum())], device="cuda")
    dl = torch.tensor([dloss], device="cuda")
    if onehot and pitched:
        rc = lib.pk_nll_logsoftmax_bwd_bf16_p(_st(), _p(yd), _p(labd), _p(dl), _p(cnt), -100, rows, N, _p(dm), ldb, pitch, _p(pm), _p(cm))
    elif onehot:
        rc = lib.pk_nll_logsoftmax_bwd_bf16(_st(), _p(yd), _p(labd), _p(dl), _p(cnt), -100, rows, N, _p(dm), ldb, _p(pm), _p(cm))
    elif pitched:
        rc = lib.pk_logsoftmax_bwd_bf16_p(_st(), _p(dyd), _p(yd), rows, N, _p(dm), ldb, pitch, _p(pm), _p(cm))
    else:
        rc = lib.pk_logsoftmax_bwd_bf16(_st(), _p(dyd), _p(yd), rows, N, _p(dm), ldb, _p(pm), _p(cm))
    _lib.check(rc, "backward")
    torch.cuda.synchronize()
    assert _guards_intact(dbuf, rows * pitch) and _guards_intact(pbuf, nws) and _guards_intact(cbuf, N)
    d2 = dm.reshape(rows, pitch)
    if pitched:
        assert bool(torch.isnan(d2[:, ldb:]).all())   # another head's slice
    return d2[:, :ldb].float().cpu(), cm.cpu(), valid


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("onehot", [True, False])
@pytest.mark.parametrize("rows,N", SHAPES)
def test_backward_kernels_between_guard_bands(rows, N, onehot, pitched):
    """dz per element: |dz - ref| <= 2^-7 |ref| + 1e-6 t, ref the fp64 value from the same fp32 y, t the size of the
    element's terms (ONEHOT: scale; dense: |dy| + exp(y) sum|dy|).  One bf16 step is 2^-7: a correctly rounded fp32
    evaluation sits at half of the bound.  Pad columns [N, ldb) exactly 0, the neighbour slice [ldb, pitch) untouched,
    the column sums against fp64 at 1e-5 (the bias-gradient bound), ignored and out-of-range labels: a zero row."""
    y, dy, lab = _backward_inputs(rows, N)
    dz, colsum, valid = _run_backward(onehot, pitched, y, dy, lab)
    y64 = y.double()
    if onehot:
        scale = float(torch.tensor(1.7) / torch.tensor(float(valid.sum())))  # as the kernel forms it: an fp32 quotient
        hot = torch.zeros(rows, N, dtype=torch.float64)
        hot[valid, lab[valid]] = 1.0
        ref = scale * (y64.exp() - hot) * valid[:, None].double()
        t = torch.full_like(ref, scale)
        assert float(dz[~valid].abs().max() if bool((~valid).any()) else 0.0) == 0.0
    else:
        s = dy.double().sum(1, keepdim=True)
        ref = dy.double() - y64.exp() * s
        t = dy.double().abs() + y64.exp() * dy.double().abs().sum(1, keepdim=True)
    err = (dz[:, :N].double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-6 * t
    ratio = float((err / bound).max())
    print("\nbackward %dx%d onehot=%s pitched=%s: worst |dz - ref| / bound %.3f" % (rows, N, onehot, pitched, ratio))
    assert bool((err <= bound).all()), ratio
    assert dz.shape[1] == N or float(dz[:, N:].abs().max()) == 0.0   # (8192 classes: no pad columns)
    e_db = rel_err(colsum, ref.sum(0))
    assert e_db < 1e-5, e_db


@pytest.mark.parametrize("rows,N", [(5, 3400), (3, 8191), (2050, 2049)])
def test_cost_kernel_without_the_arg_max_positions(rows, N):
    """pk_nll_err_fwd (PK_EXPERIMENT head_argmax=0) on wide rows: loss against fp64 at 2e-6, errors / counted rows / bad
    labels exactly - on log-posteriors of small-integer logits (ties: the first index), with an ignored and an
    out-of-range label."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows + N)
    x = torch.randint(-2, 3, (rows, N), generator=g).float() * 0.5
    y = TF.log_softmax(x.double(), 1).float()
    lab = torch.randint(0, N, (rows,), generator=g)
    lab[0] = int(_first_max(y)[0])     # a hit
    lab[rows - 1] = -100
    lab[rows - 2] = N + 3
    valid = (lab >= 0) & (lab < N)
    nws = int(lib.pk_nll_err_partial_floats(rows))
    pbuf, pm = _guarded(nws)
    obuf, om = _guarded(4)
    yd, labd = y.cuda(), lab.cuda()
    _lib.check(lib.pk_nll_err_fwd(_st(), _p(yd), _p(labd), -100, rows, N, _p(pm), _p(om), None, None), "pk_nll_err_fwd")
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, nws) and _guards_intact(obuf, 4)
    out = om.cpu()
    assert bool(torch.isnan(out[0]))           # a bad label poisons the loss
    assert float(out[2]) == int(valid.sum()) and float(out[3]) == 1.0
    n_err = int((_first_max(y) != lab).sum())
    assert abs(float(out[1]) * rows - n_err) < 1e-3
    lab[rows - 2] = -100
    valid = lab >= 0
    _lib.check(lib.pk_nll_err_fwd(_st(), _p(yd), _p(lab.cuda()), -100, rows, N, _p(pm), _p(om), None, None), "pk_nll_err_fwd")
    torch.cuda.synchronize()
    out = om.cpu()
    ref = float(-y.double()[valid, lab[valid]].mean())
    assert abs(float(out[0]) - ref) <= 2e-6 * abs(ref)
    assert float(out[2]) == int(valid.sum()) and float(out[3]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the block-per-row kernels against the wave-per-row kernels they extend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [48, 1938, 2048])
def test_block_kernels_equal_the_wave_kernels(N, monkeypatch):
    """PK_EXPERIMENT head_block=1 at widths both families cover, 70 rows.  The ONEHOT dz: bit for bit (the per-element
    expression is the same and no cross-lane sum enters it); amax, counted rows, bad labels and the error rate: equal;
    y within 1e-6 per row and the loss within 2e-6 (the order of the row sum differs)."""
    lib = _lib.load()
    rows = 70
    g = torch.Generator().manual_seed(N)
    x = torch.randn(rows, N, generator=g) * 4
    x[1] += 1e3
    lab = torch.randint(0, N, (rows,), generator=g)
    lab[3:6] = -100
    lab[9] = N + 1
    ldx = F_._up(N, 32)
    xp = torch.full((rows, ldx), float("nan"))
    xp[:, :N] = x
    xd, labd = xp.cuda(), lab.cuda()
    ldb = F_._up(N, 64)
    dl = torch.tensor([1.7], device="cuda")
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PK_EXPERIMENT", "head_block=" + mode)
        y = torch.empty(rows, N, device="cuda")
        amax = torch.empty(rows, device="cuda", dtype=torch.int32)
        _lib.check(lib.pk_logsoftmax_fwd_ld_argmax(_st(), _p(xd), ldx, rows, N, _p(y), _p(amax)), "pk_logsoftmax_fwd_ld_argmax")
        if mode == "0":
            y_wave = y
        # the cost and its gradient on the SAME log-posteriors (the wave kernel's) in both modes
        part = torch.empty(int(lib.pk_nll_err_partial_floats(rows)), device="cuda")
        out4 = torch.empty(4, device="cuda")
        _lib.check(lib.pk_nll_err_fwd(_st(), _p(y_wave), _p(labd), -100, rows, N, _p(part), _p(out4), None, None), "pk_nll_err_fwd")
        good = torch.where(labd >= N, torch.full_like(labd, -100), labd)
        out4g = torch.empty(4, device="cuda")
        _lib.check(lib.pk_nll_err_fwd(_st(), _p(y_wave), _p(good), -100, rows, N, _p(part), _p(out4g), None, None), "pk_nll_err_fwd")
        dz = torch.full((rows, ldb), float("nan"), device="cuda", dtype=torch.bfloat16)
        ws = torch.empty(int(lib.pk_logsoftmax_bwd_bf16_partial_floats(rows, N)), device="cuda")
        db = torch.empty(N, device="cuda")
        cnt = out4g[2:3].clone()
        _lib.check(lib.pk_nll_logsoftmax_bwd_bf16(_st(), _p(y_wave), _p(labd), _p(dl), _p(cnt), -100, rows, N, _p(dz), ldb, _p(ws),
                                                  _p(db)), "pk_nll_logsoftmax_bwd_bf16")
        torch.cuda.synchronize()
        res[mode] = (y.cpu(), amax.cpu(), out4.cpu(), out4g.cpu(), dz.view(torch.int16).cpu(), db.cpu(), ws.numel())
    (y0, a0, s0, g0, z0, b0, w0), (y1, a1, s1, g1, z1, b1, w1) = res["0"], res["1"]
    assert w1 == rows * N * 2 and w0 != w1     # the lever reached the library
    assert torch.equal(z0, z1)
    assert torch.equal(a0, a1)
    assert torch.equal(s0[1:], s1[1:]) and float(s0[3]) == 1.0 and bool(torch.isnan(s0[0])) and bool(torch.isnan(s1[0]))
    assert torch.equal(g0[1:], g1[1:]) and float(g0[3]) == 0.0 and float(g0[2]) == rows - 4
    assert abs(float(g0[0]) - float(g1[0])) <= 2e-6 * abs(float(g0[0]))
    assert bool((rel_err_rows(y1, y0, 1) < 1e-6).all())
    assert rel_err(b1, b0) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 3. the fused head against torch on the same output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,N,ignored", [(6, 16, 2049, 0), (70, 24, 3400, 3), (40, 16, 8192, 40), (9, 16, 4097, 9)])
def test_head_nll_matches_nll_loss_behind_a_wide_head(rows, K, N, ignored):
    """The assertions of test_gpu_kernels.py::test_head_nll_matches_nll_loss_behind_the_head at the new widths (loss at 2e-6,
    error rate exactly, dX / dW bit for bit between head_nll and nll_loss on the fused y, db at 1e-5), and both against
    the fp64 evaluation on bf16-rounded operands at the bounds of test_fused_output_layer_matches_the_two_nodes (y and
    db at 1e-5, dX / dW at 1e-2: dz is rounded to bf16 for the two GEMMs)."""
    g = torch.Generator().manual_seed(rows * 3 + N)
    x = torch.randn(rows, K, generator=g)
    w = torch.randn(N, K, generator=g) / (K ** 0.5)
    b = torch.randn(N, generator=g)
    lab = torch.randint(0, N, (rows,), generator=g)
    lab[:ignored] = -100
    F_.set_precision("bf16")
    try:
        res = []
        for fused in (True, False):
            xe, we, be = (t.clone().cuda().requires_grad_(True) for t in (x, w, b))
            y = F_.linear_log_softmax(xe, we, be)
            assert getattr(y, "_pk_head", None) is not None
            if fused:
                loss, stats = F_.head_nll(y, lab.cuda())
                err = stats[1]
                assert float(stats[2]) == rows - ignored and float(stats[3]) == 0
            else:
                loss = TF.nll_loss(y, lab.cuda())
                err = (y.argmax(1) != lab.cuda()).float().mean()
            (loss * 1.7).backward()
            torch.cuda.synchronize()
            res.append((loss.detach(), err, xe.grad, we.grad, be.grad, y.detach()))
    finally:
        F_.set_precision("fp32")
    (l1, e1, dx1, dw1, db1, y1), (l2, e2, dx2, dw2, db2, _) = res
    rb = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    xr, wr = rb(x).requires_grad_(True), rb(w).requires_grad_(True)
    br = b.double().requires_grad_(True)
    yr = TF.log_softmax(TF.linear(xr, wr, br), 1)
    assert rel_err(y1, yr) < 1e-5
    if ignored == rows:
        assert torch.isnan(l1) and torch.isnan(l2)
        assert float(dx1.abs().max()) == 0.0  # torch: 0 * nan-free zeros; the engine: scale 0
        return
    assert abs(float(l1) - float(l2)) <= 2e-6 * abs(float(l2))
    assert float(e1) == pytest.approx(float(e2), abs=1e-7)
    assert torch.equal(dx1, dx2) and torch.equal(dw1, dw2)
    assert rel_err(db1, db2) < 1e-5
    (TF.nll_loss(yr, lab) * 1.7).backward()
    assert rel_err(db1, br.grad) < 1e-5
    assert rel_err(dx1, xr.grad) < 1e-2 and rel_err(dw1, wr.grad) < 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# 4. degenerate logits
# ---------------------------------------------------------------------------------------------------------------------
def _fmt(v):
    return "[" + " ".join("%.1e" % float(e) for e in torch.as_tensor(v).reshape(-1)) + "]"


def _lsm_reference(c):
    xr = c.x.double().requires_grad_(True)
    yr = TF.log_softmax(xr, 1)
    (yr * c.cot.double()).sum().backward()
    dx_dy = xr.grad.clone()
    xr.grad = None
    loss = TF.nll_loss(TF.log_softmax(xr, 1), c.lab)
    (loss * 1.7).backward()
    return yr.detach(), dx_dy, float(loss), xr.grad.clone()


@pytest.mark.parametrize("N", [2100, 3400, 8192])
def test_wide_fused_head_and_cost_on_extreme_logits(N, monkeypatch):
    """tests/test_gpu_degenerate_rows.py::test_fused_head_and_cost_on_extreme_logits, same assertions, at the widths of the
    block-per-row kernels, in both head_argmax modes."""
    rows = 6
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


# ---------------------------------------------------------------------------------------------------------------------
# 5. two heads on one input
# ---------------------------------------------------------------------------------------------------------------------
def test_two_heads_on_one_input_with_a_wide_slice(monkeypatch):
    """Heads of 3400 and 48 classes on one activation at 4096 rows: the one-GEMM input gradient (functional._cat_*) with a
    slice of 3456 columns in front of the second head's.  dX, both dW and both db against the same step with
    PK_EXPERIMENT head_dx_cat=0, at the 2e-6 tests/test_gpu_round6.py holds the narrow pair to."""
    g = torch.Generator().manual_seed(12)
    rows, K = 4096, 32
    x0 = torch.randn(rows, K, generator=g)
    w1, w2 = torch.randn(3400, K, generator=g) / 6, torch.randn(48, K, generator=g) / 6
    b1, b2 = torch.randn(3400, generator=g), torch.randn(48, generator=g)
    l1, l2 = torch.randint(0, 3400, (rows,), generator=g).cuda(), torch.randint(0, 48, (rows,), generator=g).cuda()
    F_.set_precision("bf16")
    res = {}
    for cat in ("1", "0"):
        monkeypatch.setenv("PK_EXPERIMENT", "head_dx_cat=" + cat)
        x = x0.clone().cuda().requires_grad_(True)
        h = x * 1.0
        p = [t.clone().cuda().requires_grad_(True) for t in (w1, b1, w2, b2)]
        y1, y2 = F_.linear_log_softmax(h, p[0], p[1]), F_.linear_log_softmax(h, p[2], p[3])
        loss = F_.head_nll(y1, l1)[0] + 0.5 * F_.head_nll(y2, l2)[0]
        shared = [c for c in F_._DxShare.cat.values() if len(c["heads"]) == 2]
        if cat == "1":
            assert len(shared) == 1 and shared[0]["width"] == 3456 + 64 and [h_["off"] for h_ in shared[0]["heads"]] == [0, 3456]
        else:
            assert not shared
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(x.grad).all() and not F_._DxShare.cat
        res[cat] = [x.grad.clone()] + [q.grad.clone() for q in p]
    for name, got, ref in zip(("dX", "dW1", "db1", "dW2", "db2"), res["1"], res["0"]):
        e = rel_err(got, ref)
        assert float(ref.abs().max()) > 0 and e < 2e-6, (name, e)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the class
# ---------------------------------------------------------------------------------------------------------------------
def _mlp(classes, inp_dim, hidden=None):
    lay = ([hidden] if hidden else []) + [classes]
    n = len(lay)
    j = lambda v: ",".join([str(v)] * n)  # noqa: E731
    opts = {"dnn_lay": ",".join(str(v) for v in lay), "dnn_drop": j(0.0), "dnn_use_laynorm_inp": "False", "dnn_use_batchnorm_inp": "False",
            "dnn_use_batchnorm": j(False), "dnn_use_laynorm": j(False), "dnn_act": ",".join(["relu"] * (n - 1) + ["softmax"]),
            "use_cuda": "True", "to_do": "train"}
    return nn_amd.MLP(opts, inp_dim)


def _through_forward_model(net, inp, F, to_do="train"):
    fea_dict = {"fea": ["fea", "lst", "opts", "cw_l", "cw_r", 0, F]}
    lab_dict = {"lab": ["lab", "folder", "opts", F]}
    arch_dict = {"MLP_layers": ["architecture1", "MLP_layers", False]}
    model = ["out_dnn=compute(MLP_layers,fea)", "loss=cost_nll(out_dnn,lab)", "err=cost_err(out_dnn,lab)"]
    iod = {"fea": ["a", "b", "c", "d", "e", 0, F, F], "out_dnn": [net.out_dim], "loss": [1], "err": [1]}
    return U.forward_model(fea_dict, lab_dict, arch_dict, model, {"MLP_layers": net}, {"loss": torch.nn.NLLLoss()}, inp, iod,
                           inp.shape[0], 1, to_do, [])


def test_mlp_with_a_3400_way_head_through_forward_model():
    """nn.MLP with dnn_lay = 3400, softmax, no normalisation, behind a cost_nll and a cost_err line: the output is the fused
    head's, loss and error equal the run with settings.fused_cost = False (2e-6 / exactly); 8193 classes still run, on
    the unfused path; a forward-only call under no_grad gives the grad-mode output (max(1e-6, 2 x run-to-run))."""
    rows, F = 96, 24
    g = torch.Generator().manual_seed(5)
    F_.set_precision("bf16")
    torch.manual_seed(6)
    net = _mlp(3400, F).cuda().train()
    inp = torch.cat((torch.randn(rows, F, generator=g), torch.randint(0, 3400, (rows, 1), generator=g).float()), 1).cuda()
    outs = _through_forward_model(net, inp, F)
    assert getattr(outs["out_dnn"], "_pk_head", None) is not None
    assert getattr(outs["out_dnn"], "_pk_nll_stats", None) is not None
    outs["loss"].backward()
    grads = [q.grad.clone() for q in net.wx[0].parameters()]   # (the layer's unused norm modules have parameters too)
    assert all(bool(torch.isfinite(q).all()) and float(q.abs().max()) > 0 for q in grads)
    F_.settings.fused_cost = False
    try:
        plain = _through_forward_model(net, inp, F)
    finally:
        F_.settings.fused_cost = True
    assert getattr(plain["out_dnn"], "_pk_nll_stats", None) is None
    assert abs(float(outs["loss"]) - float(plain["loss"])) <= 2e-6 * abs(float(plain["loss"]))
    assert float(outs["err"]) == pytest.approx(float(plain["err"]), abs=1e-7)
    # forward only
    again = _through_forward_model(net, inp, F)["out_dnn"].detach()
    net.eval()
    y_grad = net(inp[:, :F]).detach()
    y_grad2 = net(inp[:, :F]).detach()
    with torch.no_grad():
        y_fwd = net(inp[:, :F])
    tol = max(1e-6, 2 * rel_err(y_grad2, y_grad))
    assert rel_err(y_fwd, y_grad) <= tol
    assert rel_err(again, outs["out_dnn"]) <= tol
    # one class too many for the fused head: the layer runs as Linear + LogSoftmax nodes
    torch.manual_seed(7)
    big = _mlp(8193, F).cuda().train()
    inp2 = torch.cat((inp[:, :F], torch.randint(0, 8193, (rows, 1), generator=g).float().cuda()), 1)
    outs2 = _through_forward_model(big, inp2, F)
    assert getattr(outs2["out_dnn"], "_pk_head", None) is None
    assert outs2["out_dnn"].shape == (rows, 8193) and bool(torch.isfinite(outs2["loss"]))
    ref = TF.log_softmax(TF.linear(inp2[:, :F].to(torch.bfloat16).double(), big.wx[0].weight.detach().to(torch.bfloat16).double(),
                                   big.wx[0].bias.detach().double()), 1)
    assert rel_err(outs2["out_dnn"], ref) < 1e-5
    outs2["loss"].backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in big.wx[0].parameters())


# ---------------------------------------------------------------------------------------------------------------------
# 7. replay
# ---------------------------------------------------------------------------------------------------------------------
def test_hip_graph_replay_of_a_step_with_a_3400_way_head():
    """The 128-row MLP step with a 3400-way head (forward, fused cost, backward, fused RMSprop) captured by
    graphs.GraphedStep: three replays end where three eager steps end - parameters, optimizer state and losses equal,
    as tests/test_gpu_parity.py::test_hip_graph_replay_trains_like_eager_steps asks of the narrow head."""
    optim_ = importlib.import_module("pytorch-kaldi_amd.optim")
    graphs = importlib.import_module("pytorch-kaldi_amd.graphs")
    rows, F, N = 128, 20, 3400
    g = torch.Generator().manual_seed(9)
    packed = [torch.cat((torch.randn(rows, F, generator=g), torch.randint(0, N, (rows, 1), generator=g).float()), 1).cuda()
              for _ in range(6)]
    F_.set_precision("bf16")
    results = []
    for use_graph in (False, True):
        torch.manual_seed(4)
        net = _mlp(N, F, hidden=64).cuda().train()
        opt = optim_.FusedOptimizer(optim_.FlatParams(net), "rmsprop", 1e-3, alpha=0.95, eps=1e-8)
        fused = []

        def step(inp):
            opt.zero_grad()
            y = net(inp[:, :F])
            fused.append(getattr(y, "_pk_head", None) is not None)
            loss = F_.head_nll(y, inp[:, F].long())[0]
            loss.backward()
            opt.step()
            return loss.detach()

        losses = [step(packed[i]) for i in range(3)]
        if use_graph:
            gs = graphs.GraphedStep(step, [opt]).capture(packed[3])
            losses += [gs(packed[i]).clone() for i in range(3, 6)]
        else:
            losses += [step(packed[i]) for i in range(3, 6)]
        torch.cuda.synchronize()
        assert fused and all(fused)
        results.append((opt.flat.flat.clone(), opt.bufs["square_avg"].clone(), opt.steps, torch.stack(losses)))
    (p0, s0, n0, l0), (p1, s1, n1, l1) = results
    assert n0 == n1 == 6
    assert bool(torch.isfinite(l0).all()) and float(l0[0]) > 0
    assert torch.equal(l0, l1) and torch.equal(p0, p1) and torch.equal(s0, s1)
    F_.raise_if_bad_labels()
