"""LSTM_cudnn / RNN_cudnn on the GPU: the pk_gates_* and pk_seq_join_* kernels through the C ABI against the host
construction of the same tensors, the classes against the fixtures the reference's classes wrote
(tools/make_golden_cudnn.py), against a CPU composition of single-layer torch.nn.LSTM modules with injected dropout masks,
against the engine's own LSTM / RNN loaded with the permuted weights and the summed bias (their "twins": same kernels,
same operands), forward-only calls, and three training steps with the fused RMSprop.

Bounds.  Pack, unpack and join copy, select, or do ONE fp32 operation per element (the bias sum; the multiplication with
the dropout scale; in the join's backward one add and then one multiplication, which no compiler contracts): the host
computes the same IEEE operations, so the comparisons are torch.equal.  The reference comparisons use the project's
standing fp32 figure, 1e-4.  Against a twin the run-to-run distance d0 of the twin is measured first (two runs of the same
module on the same inputs, norm-relative); y and dx must then be within max(1e-6, 2 d0) and the weight and bias gradients,
un-permuted on the host, within max(1e-5, 2 d0) - the QLSTM twin test's bounds, for the same reason.  The keep rate of the
device-drawn masks is a binomial proportion over N = 4096 draws: within 6 sqrt(p (1 - p) / N) of 1 - p.
"""
import configparser
import ctypes
import importlib
import itertools
import math

import numpy as np
import pytest
import torch

from golden_util import Golden, check_grads, rel_err

pytestmark = pytest.mark.gpu
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_amd = importlib.import_module("pytorch-kaldi_amd.functional")
optim_amd = importlib.import_module("pytorch-kaldi_amd.optim")
U_amd = importlib.import_module("pytorch-kaldi_amd.utils")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

GUARD = 64  # floats: 256 bytes, so the guarded middle of a fresh allocation starts 16-byte aligned
PERM = {4: (1, 0, 3, 2), 1: (0,)}
SCALE = float(np.float32(1.0 / 0.8))


@pytest.fixture(autouse=True)
def _fp32_auto():
    F_amd.set_precision("fp32")
    F_amd.set_rec_algo("auto")
    yield
    F_amd.set_precision("fp32")
    F_amd.set_rec_algo("auto")


def _guarded(n, fill=None, off=0):
    """A device buffer of n floats with at least GUARD floats of NaN on both sides: (whole buffer, the n floats in the
    middle).  off = 1 moves the middle 4 bytes off its 16-byte boundary."""
    buf = torch.full((n + 2 * GUARD + off,), float("nan"), device="cuda")
    mid = buf[GUARD + off:GUARD + off + n]
    assert mid.data_ptr() % 16 == 4 * off
    if fill is not None:
        mid.copy_(fill.reshape(-1))
    return buf, mid


def _guards_intact(buf, n, off=0):
    return bool(torch.isnan(buf[:GUARD + off]).all()) and bool(torch.isnan(buf[GUARD + off + n:]).all())


def _dev(t, off=0):
    """t on the device; off = 1: as a slice that starts 4 bytes behind a 16-byte boundary."""
    if t is None:
        return None
    big = torch.empty(t.numel() + 4, device="cuda")
    out = big[off:off + t.numel()]
    out.copy_(t.reshape(-1))
    assert out.data_ptr() % 16 == 4 * off
    return out


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# pk_gates_pack / pk_gates_unpack
# ---------------------------------------------------------------------------------------------------------------------
def host_pack(t, perm, H):
    return torch.cat([t[p * H:(p + 1) * H] for p in perm], 0)


def host_unpack(t, perm, H):
    out = torch.empty_like(t)
    for g, p in enumerate(perm):
        out[p * H:(p + 1) * H] = t[g * H:(g + 1) * H]
    return out


PACK_SHAPES = [(1, 1, 1), (4, 1, 1), (4, 3, 5), (4, 33, 17), (4, 128, 128), (4, 550, 40)]


@pytest.mark.parametrize("G,H,D", PACK_SHAPES)
@pytest.mark.parametrize("biases", ["both", "ih", "hh", "none"])
def test_pack_and_unpack_kernels_are_exact(G, H, D, biases):
    lib = _lib.load()
    perm, parg = PERM[G], F_amd._perm_arg(PERM[G])
    gen = torch.Generator().manual_seed(1000 * G + 10 * H + D)
    w_ih, w_hh = torch.randn(G * H, D, generator=gen), torch.randn(G * H, H, generator=gen)
    b_ih = torch.randn(G * H, generator=gen) if biases in ("both", "ih") else None
    b_hh = torch.randn(G * H, generator=gen) if biases in ("both", "hh") else None
    want_b = None if biases == "none" else (b_ih + b_hh if biases == "both" else (b_ih if b_hh is None else b_hh))
    d_in = [None if t is None else t.cuda() for t in (w_ih, w_hh, b_ih, b_hh)]
    (wb, W), (ub, U), (bb, b) = _guarded(G * H * D), _guarded(G * H * H), _guarded(G * H)
    _lib.check(lib.pk_gates_pack(_stream(), *[_ptr(t) for t in d_in], G, H, D, parg, _ptr(W), _ptr(U), _ptr(b)), "pk_gates_pack")
    torch.cuda.synchronize()
    assert _guards_intact(wb, G * H * D) and _guards_intact(ub, G * H * H) and _guards_intact(bb, G * H)
    assert torch.equal(W.cpu().view(G * H, D), host_pack(w_ih, perm, H))
    assert torch.equal(U.cpu().view(G * H, H), host_pack(w_hh, perm, H))
    if want_b is None:
        assert bool(torch.isnan(bb).all())  # no bias: the buffer keeps its fill
    else:
        assert torch.equal(b.cpu(), host_pack(want_b, perm, H))
    # unpack(pack(.)) gives the weights back; the bias gradient goes to both biases
    (wb2, W2), (ub2, U2), (ib, bi), (hb, bh) = _guarded(G * H * D), _guarded(G * H * H), _guarded(G * H), _guarded(G * H)
    has_b = want_b is not None
    _lib.check(lib.pk_gates_unpack(_stream(), _ptr(W), _ptr(U), _ptr(b) if has_b else None, G, H, D, parg, _ptr(W2), _ptr(U2),
                                   _ptr(bi) if biases in ("both", "ih") else None,
                                   _ptr(bh) if biases in ("both", "hh") else None), "pk_gates_unpack")
    torch.cuda.synchronize()
    assert all(_guards_intact(x, n) for x, n in ((wb2, G * H * D), (ub2, G * H * H), (ib, G * H), (hb, G * H)))
    assert torch.equal(W2.cpu().view(G * H, D), w_ih) and torch.equal(U2.cpu().view(G * H, H), w_hh)
    for buf, got, on in ((ib, bi, biases in ("both", "ih")), (hb, bh, biases in ("both", "hh"))):
        if on:
            assert torch.equal(got.cpu(), want_b)
        else:
            assert bool(torch.isnan(buf).all())


def test_pack_kernel_takes_the_scalar_path_on_unaligned_pointers():
    lib = _lib.load()
    G, H, D = 4, 8, 12
    perm, parg = PERM[G], F_amd._perm_arg(PERM[G])
    gen = torch.Generator().manual_seed(5)
    w_ih, w_hh = torch.randn(G * H, D, generator=gen), torch.randn(G * H, H, generator=gen)
    (wb, W), (ub, U) = _guarded(G * H * D, off=1), _guarded(G * H * H)
    d_ih, d_hh = _dev(w_ih), _dev(w_hh, 1)
    _lib.check(lib.pk_gates_pack(_stream(), _ptr(d_ih), _ptr(d_hh), None, None, G, H, D, parg, _ptr(W), _ptr(U), None),
               "pk_gates_pack")
    torch.cuda.synchronize()
    assert _guards_intact(wb, G * H * D, 1) and _guards_intact(ub, G * H * H)
    assert torch.equal(W.cpu().view(G * H, D), host_pack(w_ih, perm, H))
    assert torch.equal(U.cpu().view(G * H, H), host_pack(w_hh, perm, H))


def test_pack_autograd_node_gives_both_biases_the_same_gradient():
    gen = torch.Generator().manual_seed(3)
    G, H, D = 4, 5, 3
    perm = PERM[G]
    w_ih, w_hh, b_ih, b_hh = (torch.randn(*s, generator=gen).cuda().requires_grad_(True)
                              for s in ((G * H, D), (G * H, H), (G * H,), (G * H,)))
    W, U, b = F_amd.gates_pack(w_ih, w_hh, b_ih, b_hh, perm)
    assert torch.equal(W.detach().cpu(), host_pack(w_ih.detach().cpu(), perm, H))
    assert torch.equal(b.detach().cpu(), host_pack((b_ih + b_hh).detach().cpu(), perm, H))
    cw, cu, cb = (torch.randn(t.shape, generator=gen) for t in (W, U, b))
    ((W * cw.cuda()).sum() + (U * cu.cuda()).sum() + (b * cb.cuda()).sum()).backward()
    assert torch.equal(w_ih.grad.cpu(), host_unpack(cw, perm, H)) and torch.equal(w_hh.grad.cpu(), host_unpack(cu, perm, H))
    assert torch.equal(b_ih.grad.cpu(), host_unpack(cb, perm, H))
    assert torch.equal(b_ih.grad, b_hh.grad)  # bit for bit
    # one gate, biases only (RNN_cudnn): no matrix is touched
    bi, bh = (torch.randn(7, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    W1, U1, b1 = F_amd.gates_pack(None, None, bi, bh, (0,))
    assert W1 is None and U1 is None and torch.equal(b1.detach(), (bi + bh).detach())
    b1.sum().backward()
    assert torch.equal(bi.grad, torch.ones_like(bi)) and torch.equal(bi.grad, bh.grad)


# ---------------------------------------------------------------------------------------------------------------------
# pk_seq_join_fwd / pk_seq_join_bwd
# ---------------------------------------------------------------------------------------------------------------------
def host_join(yf, yb, mask, scale):
    v = yf if yb is None else torch.cat([yf, yb.flip(0)], 2)
    v = v * scale
    if mask is not None:
        v = torch.where(mask != 0, v, torch.zeros_like(v))
    return v, v.flip(0)


def host_join_bwd(dy, dy_rev, mask, scale, H, ndir):
    if dy is not None and dy_rev is not None:
        g = dy + dy_rev.flip(0)
    else:
        g = dy if dy is not None else dy_rev.flip(0)
    g = g * scale
    if mask is not None:
        g = torch.where(mask != 0, g, torch.zeros_like(g))
    return g[:, :, :H].contiguous(), (g[:, :, H:].flip(0).contiguous() if ndir == 2 else None)


JOIN_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (2, 3, 5, 2), (7, 3, 33, 2), (5, 2, 128, 1), (3, 2, 550, 2)]


@pytest.mark.parametrize("T,B,H,ndir", JOIN_SHAPES)
@pytest.mark.parametrize("off", [0, 1])
def test_join_kernels_are_exact(T, B, H, ndir, off):
    """off = 1: every tensor is a slice that starts 4 bytes behind a 16-byte boundary (the scalar path at any H)."""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(100 * T + 10 * H + ndir)
    n_half, n_full = T * B * H, T * B * ndir * H
    yf = torch.randn(T, B, H, generator=gen)
    yb = torch.randn(T, B, H, generator=gen) if ndir == 2 else None
    mask_ = torch.bernoulli(torch.full((T, B, ndir * H), 0.8), generator=gen)
    dy, dy_rev = torch.randn(T, B, ndir * H, generator=gen), torch.randn(T, B, ndir * H, generator=gen)
    for mask, (want_y, want_rev) in itertools.product((mask_, None), ((True, False), (False, True), (True, True))):
        wy, wrev = host_join(yf, yb, mask, SCALE)
        (ybuf, y), (rbuf, yr) = _guarded(n_full, off=off), _guarded(n_full, off=off)
        d_yf, d_yb, d_mask = _dev(yf, off), _dev(yb, off), _dev(mask, off)  # (named: they must outlive the launches)
        _lib.check(lib.pk_seq_join_fwd(_stream(), _ptr(d_yf), _ptr(d_yb), _ptr(d_mask), SCALE, T, B, H, ndir,
                                       _ptr(y) if want_y else None, _ptr(yr) if want_rev else None), "pk_seq_join_fwd")
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, n_full, off) and _guards_intact(rbuf, n_full, off)
        for want, buf, got, expect in ((want_y, ybuf, y, wy), (want_rev, rbuf, yr, wrev)):
            if want:
                assert torch.equal(got.cpu().view(T, B, ndir * H), expect), (mask is not None, want_y, want_rev)
            else:
                assert bool(torch.isnan(buf).all())
        # backward with the same choice of tensors
        a, b = dy if want_y else None, dy_rev if want_rev else None
        wf, wb = host_join_bwd(a, b, mask, SCALE, H, ndir)
        (fbuf, dyf), (bbuf, dyb) = _guarded(n_half, off=off), _guarded(n_half, off=off)
        d_a, d_b = _dev(a, off), _dev(b, off)
        _lib.check(lib.pk_seq_join_bwd(_stream(), _ptr(d_a), _ptr(d_b), _ptr(d_mask), SCALE, T, B, H, ndir, _ptr(dyf),
                                       _ptr(dyb) if ndir == 2 else None), "pk_seq_join_bwd")
        torch.cuda.synchronize()
        assert _guards_intact(fbuf, n_half, off) and _guards_intact(bbuf, n_half, off)
        assert torch.equal(dyf.cpu().view(T, B, H), wf), (mask is not None, want_y, want_rev)
        if ndir == 2:
            assert torch.equal(dyb.cpu().view(T, B, H), wb), (mask is not None, want_y, want_rev)
        else:
            assert bool(torch.isnan(bbuf).all())


def test_join_autograd_node():
    gen = torch.Generator().manual_seed(9)
    T, B, H = 5, 2, 6
    yf, yb = (torch.randn(T, B, H, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    mask = torch.bernoulli(torch.full((T, B, 2 * H), 0.8), generator=gen)
    y, y_rev = F_amd.seq_join(yf, yb, mask.cuda(), SCALE, True, True)
    wy, wrev = host_join(yf.detach().cpu(), yb.detach().cpu(), mask, SCALE)
    assert torch.equal(y.detach().cpu(), wy) and torch.equal(y_rev.detach().cpu(), wrev)
    c1, c2 = torch.randn(y.shape, generator=gen), torch.randn(y.shape, generator=gen)
    ((y * c1.cuda()).sum() + (y_rev * c2.cuda()).sum()).backward()
    wf, wb = host_join_bwd(c1, c2, mask, SCALE, H, 2)
    assert torch.equal(yf.grad.cpu(), wf) and torch.equal(yb.grad.cpu(), wb)
    # one direction, no mask, reversal only (layer 0's backward-direction input); only that output reaches the loss
    x = torch.randn(T, B, H, generator=gen).cuda().requires_grad_(True)
    none, x_rev = F_amd.seq_join(x, want_y=False, want_rev=True)
    assert none is None and torch.equal(x_rev.detach(), x.detach().flip(0))
    (x_rev * c1[:, :, :H].cuda()).sum().backward()
    assert torch.equal(x.grad.cpu(), c1[:, :, :H].flip(0))


def test_bad_arguments_return_an_error_and_nothing_is_launched():
    lib = _lib.load()
    st = _stream()
    T, B, H = 3, 2, 4
    src = torch.randn(T * B * 2 * H).cuda()
    (ybuf, y), (rbuf, yr) = _guarded(T * B * 2 * H), _guarded(T * B * 2 * H)
    assert lib.pk_seq_join_fwd(st, _ptr(src), _ptr(src), None, 1.0, -1, B, H, 2, _ptr(y), _ptr(yr)) != 0
    assert lib.pk_seq_join_fwd(st, _ptr(src), _ptr(src), None, 1.0, T, -2, H, 2, _ptr(y), _ptr(yr)) != 0
    assert lib.pk_seq_join_fwd(st, _ptr(src), _ptr(src), None, 1.0, T, B, -4, 2, _ptr(y), _ptr(yr)) != 0
    assert lib.pk_seq_join_fwd(st, _ptr(src), _ptr(src), None, 1.0, T, B, H, 2, None, None) != 0
    assert lib.pk_seq_join_fwd(st, _ptr(src), None, None, 1.0, T, B, H, 2, _ptr(y), _ptr(yr)) != 0
    assert lib.pk_seq_join_bwd(st, None, None, None, 1.0, T, B, H, 2, _ptr(y), _ptr(yr)) != 0
    assert lib.pk_seq_join_bwd(st, _ptr(src), None, None, 1.0, T, B, -H, 2, _ptr(y), _ptr(yr)) != 0
    parg = F_amd._perm_arg(PERM[4])
    assert lib.pk_gates_pack(st, _ptr(src), _ptr(src), None, None, 4, -1, 2, parg, _ptr(y), _ptr(yr), None) != 0
    assert lib.pk_gates_pack(st, _ptr(src), _ptr(src), None, None, 4, 1, -2, parg, _ptr(y), _ptr(yr), None) != 0
    assert lib.pk_gates_unpack(st, _ptr(src), _ptr(src), None, -4, 1, 2, parg, _ptr(y), _ptr(yr), None, None) != 0
    assert lib.pk_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all()) and bool(torch.isnan(rbuf).all())  # nothing ran
    _lib.check(lib.pk_seq_join_fwd(st, _ptr(src), None, None, 1.0, T, B, 2 * H, 1, None, _ptr(yr)), "pk_seq_join_fwd")
    torch.cuda.synchronize()
    assert torch.equal(yr.view(T, B, 2 * H), src.view(T, B, 2 * H).flip(0))


# ---------------------------------------------------------------------------------------------------------------------
# the classes
# ---------------------------------------------------------------------------------------------------------------------
def _opts(**kw):
    o = {"hidden_size": "8", "num_layers": "2", "bias": "True", "batch_first": "False", "dropout": "0.0",
         "bidirectional": "True", "nonlinearity": "tanh", "use_cuda": "True", "to_do": "train"}
    o.update({k: str(v) for k, v in kw.items()})
    return o


def _engine(meta, sd):
    net = getattr(nn_amd, meta["arch_class"])(dict(meta["options"], use_cuda="True"), meta["inp_dim"])
    res = net.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net.cuda()
    net.train() if meta["training"] else net.eval()
    return net


def _run(net, x_cpu, cot_cpu, **kw):
    net.zero_grad()
    x = x_cpu.detach().clone().cuda().requires_grad_(True)
    y = net(x, **kw)
    (y * cot_cpu.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() if p.grad is not None else None for k, p in net.named_parameters()}
    return y.detach().cpu(), x.grad.detach().cpu(), grads


E2E = ["e2e_lstm_cudnn_bidir_train", "e2e_lstm_cudnn_uni_eval", "e2e_rnn_cudnn_tanh_bidir_train",
       "e2e_rnn_cudnn_relu_uni_train"]


@pytest.mark.parametrize("algo", ["auto", "stepwise"])
@pytest.mark.parametrize("case", E2E)
def test_against_the_reference(case, algo):
    g = Golden(case)
    F_amd.set_rec_algo(algo)
    net = _engine(g.meta, g.group("sd/"))
    y, dx, grads = _run(net, g.t("x"), g.t("cot"))
    ref = g.group("grad/")
    assert sorted(ref) == sorted(grads)
    e_y, e_dx = rel_err(y, g.t("y")), rel_err(dx, g.t("dx"))
    print("%s %s: y %.2e dx %.2e" % (case, algo, e_y, e_dx))
    assert e_y < 1e-4, e_y
    worst = check_grads(grads, ref, None, tol=1e-4)
    print("worst gradient %.2e" % worst)
    assert e_dx < 1e-4, e_dx


def _torch_composition(sd, pre, D, H, L, x, masks, scale):
    """The multi-layer bidirectional torch.nn.LSTM as single-layer unidirectional ones with flip / cat and an explicit
    y * mask * scale between layers (CPU).  Returns (y, the modules by (layer, direction))."""
    mods, inp = {}, x
    for k in range(L):
        outs = []
        for d, sfx in enumerate(("", "_reverse")):
            m = torch.nn.LSTM(D if k == 0 else 2 * H, H, 1)
            m.load_state_dict({n + "_l0": sd["%s%s_l%d%s" % (pre, n, k, sfx)].clone()
                               for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}, strict=True)
            mods[(k, sfx)] = m
            y = m(inp.flip(0) if d else inp)[0]
            outs.append(y.flip(0) if d else y)
        inp = torch.cat(outs, 2)
        if k < L - 1 and masks is not None:
            inp = inp * masks[k] * scale
    return inp, mods


def test_dropout_with_injected_masks_against_a_torch_composition():
    L, H, D, T, B, p = 3, 8, 6, 10, 3, 0.3
    torch.manual_seed(31)
    net = nn_amd.LSTM_cudnn(_opts(num_layers=L, dropout=p), D)
    gen = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for k, q in net.named_parameters():
            if "bias" in k:
                q.copy_(0.1 * torch.randn(q.shape, generator=gen))
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(T, B, D, generator=gen)
    cot = torch.randn(T, B, 2 * H, generator=gen)
    # the oracle is pinned first: without dropout the composition IS the multi-layer module (CPU, exact)
    whole = torch.nn.LSTM(D, H, L, bidirectional=True)
    whole.load_state_dict({k[len("lstm.0."):]: v for k, v in sd.items()}, strict=True)
    ones = [torch.ones(T, B, 2 * H)] * (L - 1)
    with torch.no_grad():
        assert float((_torch_composition(sd, "lstm.0.", D, H, L, x, ones, 1.0)[0] - whole(x)[0]).abs().max()) == 0.0
    masks = [torch.bernoulli(torch.full((T, B, 2 * H), 1 - p), generator=gen) for _ in range(L - 1)]
    scale = float(np.float32(1.0 / (1.0 - p)))
    xr = x.clone().requires_grad_(True)
    want_y, mods = _torch_composition(sd, "lstm.0.", D, H, L, xr, masks, scale)
    (want_y * cot).sum().backward()
    want = {"lstm.0.%s_l%d%s" % (n, k, sfx): getattr(m, n + "_l0").grad for (k, sfx), m in mods.items()
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    y, dx, grads = _run(net.cuda().train(), x, cot, drop_masks=masks)
    assert sorted(want) == sorted(grads)
    e_y, e_dx = rel_err(y, want_y), rel_err(dx, xr.grad)
    worst = check_grads(grads, want, None, tol=1e-4)
    print("injected dropout: y %.2e dx %.2e worst gradient %.2e" % (e_y, e_dx, worst))
    assert e_y < 1e-4 and e_dx < 1e-4, (e_y, e_dx)
    # the masks did something: without them the output is another one
    assert rel_err(_run(net.eval(), x, cot)[0], want_y) > 1e-2


def test_device_drawn_masks():
    p = 0.2
    net = nn_amd.LSTM_cudnn(_opts(num_layers=3, hidden_size=16, dropout=p), 6).cuda().train()
    m = net._draw_masks(16, 4, torch.device("cuda"))
    assert tuple(m.shape) == (2, 16, 4, 32) and m.dtype == torch.float32
    assert bool(((m == 0) | (m == 1)).all())
    N = m.numel()
    assert N == 4096
    keep = float(m.mean())
    print("keep rate %.4f (1 - p = %.1f, bound %.4f)" % (keep, 1 - p, 6 * math.sqrt(p * (1 - p) / N)))
    assert abs(keep - (1 - p)) <= 6 * math.sqrt(p * (1 - p) / N)
    assert net.eval()._draw_masks(16, 4, torch.device("cuda")) is None
    assert nn_amd.LSTM_cudnn(_opts(num_layers=1, dropout=p), 6).cuda().train()._draw_masks(16, 4, torch.device("cuda")) is None
    assert nn_amd.LSTM_cudnn(_opts(num_layers=3, dropout=0.0), 6).cuda().train()._draw_masks(16, 4, torch.device("cuda")) is None
    torch.manual_seed(41)
    two = nn_amd.LSTM_cudnn(_opts(num_layers=2, dropout=0.5), 6).cuda().train()
    x = torch.randn(16, 4, 6, generator=torch.Generator().manual_seed(42)).cuda()
    with torch.no_grad():
        a, b = two(x), two(x)
        assert not torch.equal(a, b)               # a fresh draw per forward call
        assert int((a == 0).sum()) == 0            # the last layer's output is not dropped
        two.eval()
        c, d = two(x), two(x)
        assert torch.equal(c, d)
        one = nn_amd.LSTM_cudnn(_opts(num_layers=1, dropout=0.5), 6).cuda().train()
        assert torch.equal(one(x), one(x))


# engine twin: the reference-form class of the same cell, one unidirectional layer, loaded with the permuted weights
_TWIN = {"LSTM_cudnn": ("LSTM", "lstm", ("wfx", "wix", "wox", "wcx"), ("ufh", "uih", "uoh", "uch"), (1, 0, 3, 2)),
         "RNN_cudnn": ("RNN", "rnn", ("wh",), ("uh",), (0,))}


def _twin_of(cls, w_ih, w_hh, b_ih, b_hh, act):
    kind, pre, wn, un, perm = _TWIN[cls]
    H, D = w_hh.shape[1], w_ih.shape[1]
    opts = {pre + "_lay": str(H), pre + "_drop": "0.0", pre + "_use_laynorm_inp": "False", pre + "_use_batchnorm_inp": "False",
            pre + "_use_laynorm": "False", pre + "_use_batchnorm": "False", pre + "_bidir": "False", pre + "_act": act,
            pre + "_orthinit": "False", "use_cuda": "True", "to_do": "train"}
    twin = getattr(nn_amd, kind)(opts, D)
    with torch.no_grad():
        for g, blk in enumerate(perm):
            rows = slice(blk * H, (blk + 1) * H)
            getattr(twin, wn[g])[0].weight.copy_(w_ih[rows])
            getattr(twin, un[g])[0].weight.copy_(w_hh[rows])
            getattr(twin, wn[g])[0].bias.copy_(b_ih[rows] + b_hh[rows])
    return twin.cuda().train()


def _unpermuted_twin_grads(cls, grads, H):
    """The twin's gradients as (d weight_ih, d weight_hh, d bias) in torch's block order."""
    kind, pre, wn, un, perm = _TWIN[cls]
    inv = sorted(range(len(perm)), key=lambda g: perm[g])  # torch block -> engine gate
    return (torch.cat([grads[wn[g] + ".0.weight"] for g in inv], 0), torch.cat([grads[un[g] + ".0.weight"] for g in inv], 0),
            torch.cat([grads[wn[g] + ".0.bias"] for g in inv], 0))


def _run_twin(twin, x, cot):
    B, H = x.shape[1], cot.shape[2]
    y, dx, grads = _run(twin, x, cot, drop_masks=[torch.ones(B, H)])
    return y, dx, {k: v for k, v in grads.items() if v is not None}  # (its ln / bn parameters have no gradient)


TWIN_SHAPES = [(12, 3, 6, 8), (9, 2, 7, 13), (6, 4, 40, 64)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("T,B,D,H", TWIN_SHAPES)
@pytest.mark.parametrize("cls", ["LSTM_cudnn", "RNN_cudnn"])
def test_one_layer_equals_its_engine_twin(cls, T, B, D, H, prec):
    """Measured on the MI355X, for both classes, the three shapes (T, B, D, H) = (12, 3, 6, 8), (9, 2, 7, 13), (6, 4, 40, 64)
    and both precisions - twelve cases: d0 (twin against a second run of the twin) = 0 / 0 / 0 for y / dx / the worst
    gradient, and class - twin = 0 / 0 / 0 for y / dx / every one of weight_ih, weight_hh, bias_ih, bias_hh.  The twin
    repeats itself bit for bit at these shapes (no unordered split-K reduction is reached), and the class hands the same
    operands to the same kernels: pack and unpack are copies, and the bias sum is the one add the test does on the host."""
    torch.manual_seed(50 + H)
    net = getattr(nn_amd, cls)(_opts(num_layers=1, bidirectional=False, hidden_size=H), D)
    gen = torch.Generator().manual_seed(51)
    pre = "lstm.0." if cls == "LSTM_cudnn" else "rnn.0."
    with torch.no_grad():
        for k, q in net.named_parameters():
            if "bias" in k:
                q.copy_(0.1 * torch.randn(q.shape, generator=gen))
    sd = net.state_dict()
    twin = _twin_of(cls, *[sd[pre + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")], "tanh")
    net.cuda().train()
    x, cot = torch.randn(T, B, D, generator=gen), torch.randn(T, B, H, generator=gen)
    F_amd.set_precision(prec)
    y1, dx1, g1 = _run_twin(twin, x, cot)
    y2, dx2, g2 = _run_twin(twin, x, cot)
    d0_y, d0_dx = rel_err(y2, y1), rel_err(dx2, dx1)
    d0_g = max(rel_err(g2[k], g1[k]) for k in g1)
    y, dx, g = _run(net, x, cot)
    e_y, e_dx = rel_err(y, y1), rel_err(dx, dx1)
    dw, du, db = _unpermuted_twin_grads(cls, g1, H)
    e_g = {"weight_ih": rel_err(g[pre + "weight_ih_l0"], dw), "weight_hh": rel_err(g[pre + "weight_hh_l0"], du),
           "bias_ih": rel_err(g[pre + "bias_ih_l0"], db), "bias_hh": rel_err(g[pre + "bias_hh_l0"], db)}
    print("twin %s T%d B%d D%d H%d %s: d0 y %.2e dx %.2e grad %.2e | class-twin y %.2e dx %.2e grads %s"
          % (cls, T, B, D, H, prec, d0_y, d0_dx, d0_g, e_y, e_dx, {k: "%.2e" % v for k, v in e_g.items()}))
    assert e_y <= max(1e-6, 2 * d0_y), (e_y, d0_y)
    assert e_dx <= max(1e-6, 2 * d0_dx), (e_dx, d0_dx)
    for k, e in e_g.items():
        assert e <= max(1e-5, 2 * d0_g), (k, e, d0_g)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_two_bidirectional_layers_equal_four_engine_twins(prec):
    """Measured on the MI355X, fp32 and bf16: d0 = 0 / 0 / 0 (y / dx / worst gradient of the composition against its second
    run) and class - composition = 0 / 0 / 0: the join is a copy here (no mask, scale 1), like flip and cat."""
    T, B, D, H, L = 12, 3, 6, 8, 2
    torch.manual_seed(61)
    net = nn_amd.LSTM_cudnn(_opts(num_layers=L, hidden_size=H), D)
    gen = torch.Generator().manual_seed(62)
    with torch.no_grad():
        for k, q in net.named_parameters():
            if "bias" in k:
                q.copy_(0.1 * torch.randn(q.shape, generator=gen))
    sd = net.state_dict()
    twins = {(k, sfx): _twin_of("LSTM_cudnn", *[sd["lstm.0.%s_l%d%s" % (n, k, sfx)] for n in
                                                ("weight_ih", "weight_hh", "bias_ih", "bias_hh")], "tanh")
             for k in range(L) for sfx in ("", "_reverse")}
    net.cuda().train()
    x, cot = torch.randn(T, B, D, generator=gen), torch.randn(T, B, 2 * H, generator=gen)
    ones = [torch.ones(B, H)]

    def composition():
        for t in twins.values():
            t.zero_grad()
        xr = x.clone().cuda().requires_grad_(True)
        inp = xr
        for k in range(L):
            yf = twins[(k, "")](inp, drop_masks=ones)
            yb = torch.flip(twins[(k, "_reverse")](torch.flip(inp, [0]), drop_masks=ones), [0])
            inp = torch.cat([yf, yb], 2)
        (inp * cot.cuda()).sum().backward()
        torch.cuda.synchronize()
        grads = {}
        for (k, sfx), t in twins.items():
            tg = {n: q.grad.detach().cpu() for n, q in t.named_parameters() if q.grad is not None}
            dw, du, db = _unpermuted_twin_grads("LSTM_cudnn", tg, H)
            grads.update({"lstm.0.weight_ih_l%d%s" % (k, sfx): dw, "lstm.0.weight_hh_l%d%s" % (k, sfx): du,
                          "lstm.0.bias_ih_l%d%s" % (k, sfx): db, "lstm.0.bias_hh_l%d%s" % (k, sfx): db})
        return inp.detach().cpu(), xr.grad.detach().cpu(), grads

    F_amd.set_precision(prec)
    y1, dx1, g1 = composition()
    y2, dx2, g2 = composition()
    d0_y, d0_dx, d0_g = rel_err(y2, y1), rel_err(dx2, dx1), max(rel_err(g2[k], g1[k]) for k in g1)
    y, dx, g = _run(net, x, cot)
    assert sorted(g) == sorted(g1)
    e_y, e_dx = rel_err(y, y1), rel_err(dx, dx1)
    e_g = {k: rel_err(g[k], g1[k]) for k in g1}
    worst = max(e_g, key=e_g.get)
    print("four twins %s: d0 y %.2e dx %.2e grad %.2e | class-composition y %.2e dx %.2e worst grad %.2e (%s)"
          % (prec, d0_y, d0_dx, d0_g, e_y, e_dx, e_g[worst], worst))
    assert e_y <= max(1e-6, 2 * d0_y), (e_y, d0_y)
    assert e_dx <= max(1e-6, 2 * d0_dx), (e_dx, d0_dx)
    for k, e in e_g.items():
        assert e <= max(1e-5, 2 * d0_g), (k, e, d0_g)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("cls", ["LSTM_cudnn", "RNN_cudnn"])
def test_forward_only_equals_the_grad_mode_output(cls, prec):
    T, B, D = 7, 3, 6
    torch.manual_seed(71)
    net = getattr(nn_amd, cls)(_opts(num_layers=3, dropout=0.2), D).cuda().eval()
    x = torch.randn(T, B, D, generator=torch.Generator().manual_seed(72)).cuda()
    F_amd.set_precision(prec)
    ya = net(x.clone().requires_grad_(True)).detach().cpu()
    yb = net(x.clone().requires_grad_(True)).detach().cpu()
    with torch.no_grad():
        yn = net(x.clone()).cpu()
    torch.cuda.synchronize()
    assert float(ya.abs().max()) > 0 and bool(torch.isfinite(yn).all())
    d0 = rel_err(yb, ya)
    print("forward-only %s %s: d0 %.2e, no_grad vs grad mode %.2e" % (cls, prec, d0, rel_err(yn, ya)))
    assert rel_err(yn, ya) <= max(1e-6, 2 * d0), (rel_err(yn, ya), d0)


def test_no_bias_layer_keeps_its_autograd_edge():
    """bias=False and an input that needs no gradient: the packed matrices carry the edge, the weights get gradients."""
    for cls in ("LSTM_cudnn", "RNN_cudnn"):
        net = getattr(nn_amd, cls)(_opts(bias=False), 6).cuda().train()
        y = net(torch.randn(5, 2, 6).cuda())
        y.sum().backward()
        assert all(q.grad is not None and float(q.grad.abs().sum()) > 0 for q in net.parameters()), cls
        assert not hasattr(y, "_pk_twin")


def test_three_training_steps_with_the_fused_rmsprop():
    g = Golden("train_lstm_cudnn_3steps")
    m = g.meta
    cfg = configparser.ConfigParser()
    cfg["exp"] = {"to_do": "train", "use_cuda": "True"}
    for sec, opts in m["options"].items():
        cfg[sec] = dict(opts, arch_library="pytorch-kaldi_amd.nn")
    nfea = m["nfea"]
    fea_dict = {"fea": ["fea", "lst", "opts", "0", "0", 0, nfea, nfea]}
    lab_dict = {"lab_cd": ["lab_cd", "f", "o", nfea]}
    arch_dict = {"LSTM_cudnn_layers": ["architecture1", "LSTM_cudnn_layers", True],
                 "MLP_layers": ["architecture2", "MLP_layers", False]}
    iod = {"fea": fea_dict["fea"][5:]}
    nns, costs = U_amd.model_init(iod, m["model"], cfg, arch_dict, True, False, "train")
    assert type(nns["LSTM_cudnn_layers"]) is nn_amd.LSTM_cudnn
    for name, net in nns.items():
        net.load_state_dict(g.group("sd/%s/" % name), strict=True)
        net.cuda()
    opts = optim_amd.fused_optimizer_init(nns, cfg, arch_dict)
    inp = g.t("inp").cuda()
    losses = []
    for _ in range(m["n_steps"]):
        outs = U_amd.forward_model(fea_dict, lab_dict, arch_dict, m["model"], nns, costs, inp, iod, m["T"], m["B"], "train", [])
        for o in opts.values():
            o.zero_grad()
        outs["loss_final"].backward()
        for o in opts.values():
            o.step()
        losses.append(outs["loss_final"].detach())
    torch.cuda.synchronize()
    loss = torch.stack(losses).double().cpu().numpy()
    ref = g.arrays["loss"]
    rel = np.abs(loss - ref) / np.abs(ref)
    print("losses", loss, "reference", ref, "rel", rel)
    assert rel.max() < 1e-4, rel
    for name, net in nns.items():
        fin = g.group("sd_final/%s/" % name)
        sd = net.state_dict()
        assert list(sd) == list(fin)
        for k, v in sd.items():
            if v.is_floating_point() and float(fin[k].norm()) > 0:
                assert rel_err(v, fin[k]) < 1e-4, (name, k, rel_err(v, fin[k]))
        moved = max(rel_err(fin[k], g.group("sd/%s/" % name)[k]) for k in fin if fin[k].is_floating_point()
                    and float(fin[k].norm()) > 0)
        assert moved > 1e-3, (name, moved)
