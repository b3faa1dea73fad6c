"""Recurrent stacks whose layers differ - in width, LayerNorm, BatchNorm, dropout rate - so that neighbouring layers take
different routes (functional.rec_route): perf node -> general node -> perf node, persistent -> step-wise -> persistent,
the bf16 twin dropped and rebuilt, running statistics updated in-kernel by one layer and by _foreach_* in the next.  And
layers wider than 576, which take the step-wise kernels in both precisions.

Every case is compared with the CPU oracle on seeded inputs with injected drop masks, as
test_gpu_parity.py::test_per_step_layernorm_in_the_persistent_loop does: fp32 mode against the fp32 oracle at 1e-4, bf16
mode against the oracle's bf16-operand model at 5e-3 (outputs) / 2e-2 (gradients); ReLU candidates are differentiated on
the oracle run's own kink pattern (T <= 8).

Measured on an MI355X (norm-relative; worst over the stacks of a group; every kink report 0 flipped):

                          mixed stacks (a)                       one wide layer, H = 577 / 640 (b)
                  y        dx       gradient  running stat.     y        dx       gradient  running stat.
  liGRU      fp32 5.0e-07  8.6e-07  1.1e-06   1.7e-07           1.5e-07  4.0e-07  3.1e-07   1.1e-07
             bf16 2.7e-07  4.8e-03  5.4e-03   1.4e-07           1.2e-07  2.4e-03  2.6e-03   1.0e-07
  RNN        fp32 5.6e-07  5.3e-07  8.7e-07   3.6e-07           1.7e-07  4.2e-07  2.6e-07   1.1e-07
             bf16 8.6e-07  6.2e-03  6.5e-03   1.4e-07           1.5e-06  2.7e-03  2.5e-03   1.0e-07
  LSTM       fp32 4.8e-07  9.2e-07  1.2e-06   4.5e-07           1.2e-07  4.0e-07  2.5e-07   1.1e-07
             bf16 2.9e-07  6.6e-03  6.9e-03   2.4e-07           3.2e-07  2.5e-03  2.6e-03   1.0e-07
  GRU        fp32 3.7e-07  8.8e-07  1.3e-06   4.1e-07           1.2e-07  3.7e-07  5.3e-07   1.1e-07
             bf16 1.7e-04  5.1e-03  6.6e-03   1.4e-04           3.2e-05  2.2e-03  2.5e-03   1.0e-07
  minimalGRU fp32 4.6e-07  7.8e-07  1.3e-06   1.7e-07           1.2e-07  3.9e-07  2.7e-07   1.1e-07
             bf16 4.3e-06  5.6e-03  1.0e-02   1.4e-07           1.2e-07  2.5e-03  2.5e-03   1.0e-07

(c) every forward-only output within 6.5e-07 (fp32) / 6.3e-05 (bf16) of the oracle, and equal to the with-grad forward.  (d) flat gradients
inside and outside the training-step context: identical.  (e) 4.3e-07 and 2.9e-07 on the two calls."""
import contextlib
import importlib

import pytest
import torch

import pk_oracle as O
from golden_util import check_grads, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
TIGHT_OUT, TIGHT_GRAD = 5e-3, 2e-2   # bf16 mode against the bf16-operand model (test_gpu_reference_pins.py)
U_BF16 = 2.0 ** -9

CELLS = [("liGRU", "ligru", "relu"), ("RNN", "rnn", "relu"), ("LSTM", "lstm", "tanh"), ("GRU", "gru", "tanh"),
         ("minimalGRU", "minimalgru", "relu")]
TWO_PHASE = ("GRU", "minimalGRU")

# name -> lay, use_laynorm, use_batchnorm, drop, bidir, and the route of every layer in fp32 / bf16 mode while training:
# "perf" = RecLayerPerfFn; "persistent" / "stepwise" = the general node (RecLayerFn) with that algorithm
STACKS = {
    "narrow_wide_narrow": ([24, 580, 24], [False] * 3, [True] * 3, [0.2, 0.1, 0.3], True,
                           ["persistent", "stepwise", "persistent"], ["perf", "stepwise", "perf"]),
    "wide_first": ([580, 24], [False] * 2, [True] * 2, [0.2, 0.1], True,
                   ["stepwise", "persistent"], ["stepwise", "perf"]),
    "wide_last_uni": ([24, 580], [False] * 2, [True] * 2, [0.1, 0.2], False,
                      ["persistent", "stepwise"], ["perf", "stepwise"]),
    "ln_in_the_middle": ([40, 40, 40], [False, True, False], [True, False, True], [0.2, 0.0, 0.1], True,
                         ["persistent"] * 3, ["perf", "persistent", "perf"]),
    "ln_first": ([40, 40], [True, False], [False, False], [0.1, 0.2], True,
                 ["persistent"] * 2, ["persistent", "perf"]),
}
D, T, B = 13, 6, 3


@pytest.fixture(autouse=True)
def _restore_mode():
    F_ = importlib.import_module("pytorch-kaldi_amd.functional")
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")
    yield
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")
    F_.set_forced_kinks(None)


@contextlib.contextmanager
def _one_cpu_thread():
    """Seeded weights that are the same on every host (the orthogonal initialisation goes through a LAPACK QR whose last
    bits change with the number of CPU threads; see test_gpu_parity.py)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _stack_opts(pre, lay, act, ln, bn, drop, bidir, to_do="train"):
    j = lambda vals: ",".join(map(str, vals))  # noqa: E731
    return {pre + "_lay": j(lay), pre + "_drop": j(drop), pre + "_use_laynorm_inp": "False",
            pre + "_use_batchnorm_inp": "False", pre + "_use_laynorm": j(ln), pre + "_use_batchnorm": j(bn),
            pre + "_bidir": str(bidir), pre + "_act": j([act] * len(lay)), pre + "_orthinit": "True", "use_cuda": "True",
            "to_do": to_do}


def _route_names(F_, kind, lay, ln, bn, training):
    """The route of every layer in the precision / autograd mode that is current."""
    names, routes = [], []
    for H, l_, b_ in zip(lay, ln, bn):
        r = F_.rec_route(kind, H, bool(l_), bool(b_), training)
        routes.append(r)
        names.append("perf" if r.perf else ("persistent" if r.algo == F_.REC_PERSISTENT else "stepwise"))
    return names, routes


def _build(kind, opts, inp_dim, seed):
    """The module (on the CPU) with its normalisation parameters away from (1, 0), and its state dict."""
    from engine_util import nn_amd

    with _one_cpu_thread():
        torch.manual_seed(seed)
        net = getattr(nn_amd, kind)(opts, inp_dim)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, q in net.named_parameters():
                head, leaf = name.split(".")[0], name.split(".")[-1]
                if leaf == "gamma" or (head.startswith("bn") and leaf == "weight"):
                    q.mul_(1.0 + 0.3 * torch.randn(q.shape, generator=g))
                elif leaf == "beta" or (head.startswith("bn") and leaf == "bias"):
                    q.add_(0.2 * torch.randn(q.shape, generator=g))
    return net, {k: v.detach().clone() for k, v in net.state_dict().items()}


def _train_case(kind, pre, act, lay, ln, bn, drop, bidir, inp_dim, T_, B_, prec, want_routes, seed):
    """One training step of the stack, forward and backward, graded against the oracle."""
    from engine_util import F_amd

    F_amd.set_precision(prec)
    F_amd.set_rec_algo("auto")
    opts = _stack_opts(pre, lay, act, ln, bn, drop, bidir)
    names, routes = _route_names(F_amd, kind, lay, ln, bn, True)
    assert names == want_routes, (names, want_routes)
    if prec == "bf16":  # a general-node layer that normalises h_t runs the bf16 persistent LayerNorm kernels
        for r, l_ in zip(routes, ln):
            if l_:
                assert r.family == ("2p_bf16_ln" if kind in TWO_PHASE else "bf16_ln"), r
    net, sd = _build(kind, opts, inp_dim, 321)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T_, B_, inp_dim, generator=g)
    masks = O.make_drop_masks(kind, opts, B_, "train", generator=g)
    cot = torch.randn(T_, B_, net.out_dim, generator=g)
    osd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    log = [] if act == "relu" else None
    with (O.bf16_operands() if prec == "bf16" else contextlib.nullcontext()):
        yo = O.recurrent_forward(kind, opts, osd, xo, training=True, to_do="train", drop_masks=masks, kink_log=log)
        (yo * cot).sum().backward()
    ref = {k: v.grad for k, v in osd.items() if v.requires_grad and v.grad is not None}
    report = F_amd.set_forced_kinks(log) if log is not None else None
    try:
        net.cuda().train()
        xe = x.clone().cuda().requires_grad_(True)
        ye = net(xe, drop_masks=masks)
        (ye * cot.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        F_amd.set_forced_kinks(None)
    got = {k: (q.grad.detach().cpu() if q.grad is not None else None) for k, q in net.named_parameters()}
    otol, gtol = (TOL, TOL) if prec == "fp32" else (TIGHT_OUT, TIGHT_GRAD)
    e_y, e_x = rel_err(ye, yo), rel_err(xe.grad, xo.grad)
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for v in ref.values())))
    per = {k: float((got[k].double() - v.double()).norm()) / max(float(v.double().norm()), 1e-3 * total)
           for k, v in ref.items() if got[k] is not None}
    worst_k = max(per, key=per.get)
    stat_tol = 1e-5 if prec == "fp32" else 4 * U_BF16
    after = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    e_stat = max([rel_err(after[k], v) for k, v in osd.items() if "running" in k] or [0.0])
    print("\nmixed stack %s lay %s %s routes %s: y %.2e, dx %.2e, worst parameter gradient %.2e (%s), worst running statistic "
          "%.2e%s" % (kind, lay, prec, names, e_y, e_x, per[worst_k], worst_k, e_stat,
                      "" if report is None else "; kink report %s" % (report,)))
    assert e_y < otol, e_y
    assert e_x < gtol, e_x
    worst = check_grads(got, ref, None, gtol)
    assert worst < gtol
    # unused ln / bn parameters (the flag of their layer is off) have no gradient; the used ones have one
    unused = {id(q) for q in net.pk_unused_parameters()}
    n_unused = 0
    for k, q in net.named_parameters():
        if id(q) in unused:
            n_unused += 1
            assert k not in ref, k
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, k
        else:
            assert k in ref and got[k] is not None and float(got[k].abs().max()) > 0, k
    assert n_unused > 0
    # BatchNorm running statistics and counters after the step (a layer without BatchNorm leaves its modules untouched)
    n_counted = 0
    for k, v in osd.items():
        if "running" in k:
            assert rel_err(after[k], v) < stat_tol, (k, rel_err(after[k], v))
        elif "num_batches_tracked" in k:
            assert int(after[k]) == int(v), k
            n_counted += int(v)
    assert n_counted == sum(bn) * len(net._gates)
    if report is not None:  # the engine's own kink pattern differs from the oracle's only where a_t is rounding noise
        assert len(report) == len(lay)
        for flipped, total_k, worst_a in report:
            assert flipped < (2e-4 if prec == "fp32" else 2e-2) * total_k, report


# --------------------------------------------------------------------------------
# a. route changes inside a stack, training, forward + backward
# --------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,pre,act", CELLS)
@pytest.mark.parametrize("stack", list(STACKS))
def test_mixed_stack_training_step_against_the_oracle(stack, kind, pre, act, prec):
    lay, ln, bn, drop, bidir, routes_f32, routes_bf16 = STACKS[stack]
    _train_case(kind, pre, act, lay, ln, bn, drop, bidir, D, T, B, prec, routes_f32 if prec == "fp32" else routes_bf16, 321)


# --------------------------------------------------------------------------------
# b. layers wider than 576 on their own: the step-wise kernels in both precisions; 577 is odd (no 8- or 16-byte aligned
#    direction halves, gates re-pitched to 584 in the bf16 dU products), 640 a multiple of 128
# --------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,pre,act", CELLS)
@pytest.mark.parametrize("H,inp_dim,bidir", [(577, 13, True), (640, 16, False)])
def test_wide_layer_on_the_stepwise_kernels_against_the_oracle(H, inp_dim, bidir, kind, pre, act, prec):
    _train_case(kind, pre, act, [H], [False], [True], [0.2], bidir, inp_dim, 5, 3, prec, ["stepwise"], 654)


# --------------------------------------------------------------------------------
# c. forward-only chunks (module.eval(), torch.no_grad()): an inner perf layer leaves its fp32 output unwritten, which is
#    right only if the layer above reads the bf16 copy (functional.rec_keep_y)
# --------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,pre,act", CELLS)
@pytest.mark.parametrize("stack", list(STACKS))
def test_mixed_stack_forward_only_chunk(stack, kind, pre, act, prec):
    """The buffer an inner layer skips is uninitialised memory.  So that a recycled block which happens to hold the
    right values cannot make this pass: a with-grad forward on another input first, then NaN-filled blocks of every
    inner layer's output shape are allocated and freed, then the no_grad forward, and only then the with-grad forward
    of the same input it is compared with, bit for bit.

    Before functional.rec_keep_y (keep_y = "autograd on, or the last layer") the fifteen bf16 cases with a perf layer
    below a general one failed here - narrow_wide_narrow, wide_last_uni and ln_in_the_middle, all five cells: NaN outputs
    in seven of them, outputs 0.44 to 1.08 (norm-relative) away from the oracle in the other eight.

    With autograd on, an eval-mode layer with BatchNorm stays off the perf node (functional.perf_path_ok: backward through
    frozen statistics); the general node then runs the same persistent kernel as the no_grad forward - for GRU /
    minimalGRU too (functional.choose_rec_algo; they used to take the step-wise kernels there, which left the two
    forwards 3.6e-08 to 1.7e-07 apart in six of these cases) - so the comparison is bit for bit in every case."""
    from engine_util import F_amd

    lay, ln, bn, drop, bidir, _, _ = STACKS[stack]
    ndir = 2 if bidir else 1
    F_amd.set_precision(prec)
    F_amd.set_rec_algo("auto")
    opts = _stack_opts(pre, lay, act, ln, bn, drop, bidir, to_do="valid")
    net, _ = _build(kind, opts, D, 432)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():  # running statistics away from (0, 1)
        for b_ in net.buffers():
            if b_.dtype.is_floating_point:
                b_.add_(0.2 * torch.rand(b_.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x1, x2 = torch.randn(T, B, D, generator=g), torch.randn(T, B, D, generator=g)
    with (O.bf16_operands() if prec == "bf16" else contextlib.nullcontext()), torch.no_grad():
        yo = O.recurrent_forward(kind, opts, sd, x2, training=False, to_do="valid")
    net.cuda().eval()
    with torch.no_grad():
        names, routes = _route_names(F_amd, kind, lay, ln, bn, False)
    want = {"narrow_wide_narrow": ["perf", "stepwise", "perf"], "wide_first": ["stepwise", "perf"],
            "wide_last_uni": ["perf", "stepwise"], "ln_in_the_middle": ["perf", "persistent", "perf"],
            "ln_first": ["persistent", "perf"]}[stack]
    if prec == "bf16":
        assert names == want, (names, want)
    else:
        assert "perf" not in names, names
    names_grad, _ = _route_names(F_amd, kind, lay, ln, bn, False)  # (autograd on: frozen BatchNorm statistics keep a layer off the perf node)
    y1 = net(x1.cuda().requires_grad_(True))
    torch.cuda.synchronize()
    del y1
    poison = [torch.full((T, B, ndir * H), float("nan"), device="cuda") for H in lay[:-1] for _ in range(8)]
    torch.cuda.synchronize()
    del poison
    with torch.no_grad():
        y_fwd = net(x2.cuda())
    torch.cuda.synchronize()
    y_grad = net(x2.cuda().requires_grad_(True))
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(y_fwd).all())
    e_y = rel_err(y_fwd, yo) if finite else float("nan")
    same = torch.equal(y_fwd, y_grad.detach())
    print("\nforward-only chunk %s lay %s %s routes %s (autograd on: %s): finite %s, vs the oracle %.2e, equal to the "
          "with-grad forward %s (%.2e)" % (kind, lay, prec, names, names_grad, finite, e_y, same, rel_err(y_fwd, y_grad)))
    assert finite
    assert e_y < (TOL if prec == "fp32" else TIGHT_OUT), e_y
    # the bf16 copy of the output, which a perf-mode Linear behind the stack takes as its operand: there if the last layer
    # ran on the perf node (under no_grad; with autograd on, by its own route), and the same over the columns in use
    tw_a, tw_b = getattr(y_fwd, "_pk_twin", None), getattr(y_grad, "_pk_twin", None)
    assert (tw_a is not None) == (names[-1] == "perf")
    assert (tw_b is not None) == (names_grad[-1] == "perf")
    if tw_a is not None:
        Hp = (lay[-1] + 7) // 8 * 8
        assert tw_a[1] == (ndir, lay[-1], Hp)
        if tw_b is not None:
            assert torch.equal(tw_a[0][:, :ndir * Hp], tw_b[0][:, :ndir * Hp])
    assert same


@pytest.mark.parametrize("kind,pre,act", [c for c in CELLS if c[0] in TWO_PHASE])
def test_frozen_batchnorm_backward_of_the_two_phase_cells_on_the_general_node(kind, pre, act):
    """An eval-mode layer with BatchNorm and autograd on is handed back by the perf node (backward through frozen
    statistics).  For GRU / minimalGRU the general node runs it on the persistent two-phase bf16 kernels - the kernel of
    the no_grad forward, which is what makes the two forwards of test_mixed_stack_forward_only_chunk bit-identical.
    Forward and backward of that route against the oracle's bf16-operand model in eval mode, 5e-3 / 2e-2."""
    from engine_util import F_amd

    lay, ln, bn, drop = [24, 40], [False] * 2, [True] * 2, [0.2, 0.1]
    F_amd.set_precision("bf16")
    opts = _stack_opts(pre, lay, act, ln, bn, drop, True, to_do="valid")
    routes = [F_amd.rec_route(kind, H, False, True, False) for H in lay]
    assert all(r == (False, F_amd.REC_PERSISTENT, "2p_bf16") for r in routes), routes
    net, _ = _build(kind, opts, D, 543)
    g = torch.Generator().manual_seed(23)
    with torch.no_grad():
        for b_ in net.buffers():
            if b_.dtype.is_floating_point:
                b_.add_(0.2 * torch.rand(b_.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(T, B, D, generator=g)
    cot = torch.randn(T, B, net.out_dim, generator=g)
    osd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    log = [] if act == "relu" else None
    with O.bf16_operands():
        yo = O.recurrent_forward(kind, opts, osd, xo, training=False, to_do="valid", kink_log=log)
        (yo * cot).sum().backward()
    ref = {k: v.grad for k, v in osd.items() if v.requires_grad and v.grad is not None}
    report = F_amd.set_forced_kinks(log) if log is not None else None
    try:
        net.cuda().eval()
        xe = x.clone().cuda().requires_grad_(True)
        ye = net(xe)
        (ye * cot.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        F_amd.set_forced_kinks(None)
    got = {k: (q.grad.detach().cpu() if q.grad is not None else None) for k, q in net.named_parameters()}
    e_y, e_x = rel_err(ye, yo), rel_err(xe.grad, xo.grad)
    worst = check_grads(got, ref, None, TIGHT_GRAD)
    print("\nfrozen BatchNorm, %s bf16, general node on the two-phase kernels: y %.2e, dx %.2e, worst parameter gradient %.2e%s"
          % (kind, e_y, e_x, worst, "" if report is None else "; kink report %s" % (report,)))
    assert e_y < TIGHT_OUT, e_y
    assert e_x < TIGHT_GRAD, e_x
    after = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for k, v in sd.items():  # eval mode: the statistics stay where they were
        assert torch.equal(after[k], v), k
    if report is not None:
        for flipped, total_k, worst_a in report:
            assert flipped < 2e-2 * total_k, report


# --------------------------------------------------------------------------------
# d. the training step's context (functional.accumulating_backward) on a mixed stack: direct BatchNorm gradients and
#    side-stream weight gradients in the perf layers, autograd in the general layer between them
# --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,pre,act", [("liGRU", "ligru", "relu"), ("GRU", "gru", "tanh")])
def test_training_step_context_on_a_mixed_stack_leaves_the_gradients_of_the_autograd_path(kind, pre, act):
    """test_gpu_parity.py::test_training_step_context_leaves_the_gradients_of_the_autograd_path with a layer that
    normalises h_t (general node, gradients through autograd) between two BatchNorm layers on the perf node."""
    optim_ = importlib.import_module("pytorch-kaldi_amd.optim")
    F_ = importlib.import_module("pytorch-kaldi_amd.functional")
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    ln, bn = [False, True, False], [True, False, True]
    opts = _stack_opts(pre, [72, 72, 72], act, ln, bn, [0.2] * 3, True)
    T_, B_, D_ = 12, 8, 24
    F_.set_precision("bf16")
    assert _route_names(F_, kind, [72] * 3, ln, bn, True)[0] == ["perf", "persistent", "perf"]
    res = {}
    x = torch.randn(T_, B_, D_, generator=torch.Generator().manual_seed(6)).cuda()
    masks = [(torch.rand(2 * B_, 72, generator=torch.Generator().manual_seed(70 + i)) > 0.2).float() for i in range(3)]
    for inside in (False, True):
        with _one_cpu_thread():
            torch.manual_seed(5)
            net = getattr(nn_amd, kind)(dict(opts), D_).cuda().train()
        flat = optim_.FlatParams(net)
        snaps = []
        for _ in range(2):
            if inside:
                with F_.accumulating_backward():
                    y = net(x, drop_masks=masks)
                    flat.zero_grad()
                    y.square().mean().backward()
            else:
                y = net(x, drop_masks=masks)
                flat.zero_grad()
                y.square().mean().backward()
            F_.join_side()
            torch.cuda.synchronize()
            snaps.append(flat.grad.clone())
        res[inside] = (snaps, {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "tracked" in k})
    for step, (a, b) in enumerate(zip(res[True][0], res[False][0])):
        print("\ntraining-step context, mixed stack %s, step %d: flat gradient inside vs outside %.2e" % (kind, step, rel_err(a, b)))
        assert float(a.abs().max()) > 0 and rel_err(a, b) < 1e-6
    for k, v in res[False][1].items():
        assert torch.equal(v, res[True][1][k]), k


# --------------------------------------------------------------------------------
# e. the reference's mask stream with layers of unequal width and rate (one of them 0: the reference still draws)
# --------------------------------------------------------------------------------
def test_reference_masks_with_unequal_layers_against_the_oracles_own_draws():
    """test_gpu_parity.py::test_reference_masks_against_the_oracles_own_draws with three layers of different widths and
    dropout rates, 0.0 among them: torch.bernoulli consumes the generator for a mask of ones too."""
    from engine_util import F_amd, nn_amd

    F_amd.set_mask_rng("reference")  # (restored by conftest's settings fixture)
    lay, drop = [24, 40, 16], [0.25, 0.0, 0.4]
    opts = _stack_opts("ligru", lay, "relu", [False] * 3, [True] * 3, drop, True)
    T_, B_, D_ = 12, 5, 9
    torch.manual_seed(3)
    net = nn_amd.liGRU(opts, D_)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(T_, B_, D_, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(4711)
    want = []
    for _ in range(2):
        masks = O.make_drop_masks("liGRU", opts, B_, "train")  # the reference's call on the global CPU generator
        assert [tuple(m.shape) for m in masks] == [(2 * B_, H) for H in lay]
        assert all((0.0 < float(m.mean()) < 1.0) if p > 0 else bool((m == 1).all()) for m, p in zip(masks, drop))
        want.append(O.recurrent_forward("liGRU", opts, sd, x, training=True, to_do="train", drop_masks=masks))
    after = torch.get_rng_state().clone()
    net.cuda().train()
    torch.manual_seed(4711)
    try:
        with torch.no_grad():
            got = [net(x.cuda()).clone() for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        nn_amd.drain_mask_prefetch()
    for i, (g_, w) in enumerate(zip(got, want)):
        print("\nreference mask stream, lay %s drop %s, call %d: y %.2e" % (lay, drop, i, rel_err(g_, w)))
        assert rel_err(g_, w) < TOL
    assert rel_err(got[0], want[1]) > 1e-2  # (other masks give another output: the comparison above is not vacuous)
    assert torch.equal(torch.get_rng_state(), after)  # torch's CPU generator stands where the reference's would
