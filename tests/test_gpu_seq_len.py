"""Batched decoding on the GPU: pk_seq_pack_len / pk_seq_join_len against the host construction of seq_len_util.py
(torch.equal, guard bands), the recurrent classes under functional.sentence_lengths against each sentence alone - the CPU
oracle for the shared-weight classes, the class's own B = 1 forward for QLSTM / LSTM_cudnn / RNN_cudnn - and
core.run_nn_dp with PK_FORWARD_BATCH on the chunk fixture the reference's own run_nn wrote.

Tolerances are the project's (test_gpu_parity.py): norm-relative 1e-4 in fp32, 5e-3 in bf16 against the oracle's
bf16-operand model.  Every sentence is graded on its own rows.  Each test prints what it measured before it asserts.

Measured on an MI355X (worst sentence of a group; rec_algo auto and stepwise alike):

                                          fp32       bf16
  bidirectional, BatchNorm, H = 13 / 16   1.3e-07    6.4e-05
  bidirectional, LayerNorm, H = 16        1.2e-06    2.9e-03 (*)
  unidirectional, BatchNorm, H = 13       1.2e-07    6.3e-07
  QLSTM / LSTM_cudnn / RNN_cudnn          0          7.5e-08      (against their own B = 1 forward)
  run_nn_dp, n = 4 and 16                 3.1e-07                 (against the reference's ark; 3 and 1 forward_model calls)

(*) the RNN's two-frame sentence, 2.87e-03 with either algorithm - the size of an operand that rounds to the neighbouring
bf16 value (2^-9), spread by the per-step LayerNorm of 16 ReLU outputs; not traced further.  Every other sentence of the
group is below 2.5e-07.  Without the lengths block the short sentences are 0.45 to 1.1 away."""
import configparser
import contextlib
import ctypes
import importlib
import io

import numpy as np
import pytest
import torch

import pk_oracle as O
from golden_util import Golden, rel_err
from seq_len_util import LENS, T_MAX, host_join_len, host_pack_len, padded_batch

pytestmark = pytest.mark.gpu
TOL = {"fp32": 1e-4, "bf16": 5e-3}
SENTINEL = -777.0
GUARD = 64  # floats between and around the outputs (a multiple of 4: the aligned layouts stay 16-byte aligned)

F_ = importlib.import_module("pytorch-kaldi_amd.functional")
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
core = importlib.import_module("pytorch-kaldi_amd.core")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")


@pytest.fixture(autouse=True)
def _restore_mode():
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")
    yield
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")


# --------------------------------------------------------------------------------
# 1. the two kernels, torch.equal to the host construction
# --------------------------------------------------------------------------------
BATCHES = {"one_frame": (1, (1,)), "mixed": (T_MAX, LENS), "all_full": (T_MAX, (T_MAX,) * len(LENS))}
LAYOUTS = ("pitched", "separate", "first_only", "second_only", "offset")


def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _input(value, shift):
    """A device copy of `value` whose first element sits `shift` floats behind a 16-byte aligned address."""
    buf = torch.empty(value.numel() + shift, device="cuda")
    buf[shift:].copy_(value.reshape(-1))
    return buf, shift


def _arena(T, B, W, layout):
    """(arena size, [(offset, pitch) or None for the two outputs]) for outputs [T][B][W]."""
    step = B * W
    if layout == "pitched":  # both outputs in one [T][2B][W] tensor
        return GUARD + 2 * T * step + GUARD, [(GUARD, 2 * step), (GUARD + step, 2 * step)]
    shift = 1 if layout == "offset" else 0
    first = (GUARD + shift, step)
    second = (GUARD + shift + T * step + GUARD, step)
    size = second[0] + T * step + GUARD
    if layout == "first_only":
        return size, [first, None]
    if layout == "second_only":
        return size, [None, second]
    return size, [first, second]


def _check_arena(arena, places, wants, T, B, W):
    """The arena equals: the sentinel everywhere but the outputs, the host construction in them."""
    want = torch.full((arena.numel(),), SENTINEL)
    for place, value in zip(places, wants):
        if place is not None:
            torch.as_strided(want, (T, B, W), (place[1], W, 1), place[0]).copy_(value)
    got = arena.cpu()
    assert torch.equal(got, want), "%d elements differ (outputs or guard bands)" % int((got != want).sum())


def _lens_dev(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def _run_pack(x, lens, layout):
    T, B, D = x.shape
    lib = _lib.load()
    xbuf, xs = _input(x, 1 if layout == "offset" else 0)
    size, places = _arena(T, B, D, layout)
    arena = torch.full((size,), SENTINEL, device="cuda")
    ptrs = [None if p is None else _ptr(arena, p[0]) for p in places]
    ld = next(p[1] for p in places if p is not None)
    dlens = _lens_dev(lens)
    rc = lib.pk_seq_pack_len(_stream(), _ptr(xbuf, xs), _ptr(dlens), T, B, D, ptrs[0], ptrs[1], ld)
    torch.cuda.synchronize()
    assert rc == 0, lib.pk_last_error()
    _check_arena(arena, places, host_pack_len(x, lens), T, B, D)


def _run_join(hf, hb, lens, layout):
    T, B, H = hf.shape
    lib = _lib.load()
    if layout == "pitched":  # the directions as the halves of one [T][2B][H] tensor
        hbuf, _ = _input(torch.cat([hf, hb], 1), 0)
        pf, pb, ldi = _ptr(hbuf), _ptr(hbuf, B * H), 2 * B * H
    else:
        shift = 1 if layout == "offset" else 0
        fbuf, _ = _input(hf, shift)
        bbuf, _ = _input(hb, shift)
        pf, pb, ldi = _ptr(fbuf, shift), _ptr(bbuf, shift), B * H
    size, places = _arena(T, B, 2 * H, layout)
    arena = torch.full((size,), SENTINEL, device="cuda")
    ptrs = [None if p is None else _ptr(arena, p[0]) for p in places]
    ld = next(p[1] for p in places if p is not None)
    dlens = _lens_dev(lens)
    rc = lib.pk_seq_join_len(_stream(), pf, pb, ldi, _ptr(dlens), T, B, H, ptrs[0], ptrs[1], ld)
    torch.cuda.synchronize()
    assert rc == 0, lib.pk_last_error()
    _check_arena(arena, places, host_join_len(hf, hb, lens), T, B, 2 * H)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", [1, 5, 8])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_pack_kernel_equals_the_host_construction(batch, width, layout):
    T, lens = BATCHES[batch]
    x = torch.randn(T, len(lens), width, generator=torch.Generator().manual_seed(3)) + 3.0  # (no zeros among the frames)
    _run_pack(x, lens, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", [1, 5, 8])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_join_kernel_equals_the_host_construction(batch, width, layout):
    T, lens = BATCHES[batch]
    g = torch.Generator().manual_seed(4)
    hf = torch.randn(T, len(lens), width, generator=g) + 3.0
    hb = torch.randn(T, len(lens), width, generator=g) - 3.0
    _run_join(hf, hb, lens, layout)


@pytest.mark.parametrize("layout", ["pitched", "offset"])
def test_kernels_beyond_one_grid(layout):
    """More units than the bounded grid has threads (2048 x 256), so that the stride loop takes a second trip: 40 x 33
    x 408 elements in the scalar form ("offset"); the vector form ("pitched") covers 532 workgroups."""
    T, B, W = 40, 33, 408
    g = torch.Generator().manual_seed(5)
    lens = [int(v) for v in torch.randint(1, T + 1, (B,), generator=g)]
    lens[0], lens[1] = T, 1
    assert T * B * W > 2048 * 256
    _run_pack(torch.randn(T, B, W, generator=g) + 3.0, lens, layout)
    H = W // 2
    _run_join(torch.randn(T, B, H, generator=g) + 3.0, torch.randn(T, B, H, generator=g) - 3.0, lens, layout)


def test_wrappers_equal_the_host_construction():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(T_MAX, len(LENS), 8, generator=g) + 3.0
    hf, hb = torch.randn(T_MAX, len(LENS), 5, generator=g), torch.randn(T_MAX, len(LENS), 5, generator=g)
    wf, wr = host_pack_len(x, LENS)
    wy, wyr = host_join_len(hf, hb, LENS)
    with F_.sentence_lengths(LENS) as sl:
        f, r = F_.seq_pack_len(x.cuda())
        both = F_.seq_pack_len(x.cuda(), cat=True)
        only_r = F_.seq_pack_len(x.cuda(), want_f=False)
        y, yr = F_.seq_join_len(hf.cuda(), hb.cuda(), want_rev=True)
        y_halves = F_.seq_join_len(torch.cat([hf, hb], 1).cuda())
        y_cat = F_.seq_join_len(torch.cat([hf, hb], 1).cuda(), cat=True)
        assert sl.device_tensor(y.device).dtype == torch.int32 and sl.device_tensor(y.device).tolist() == list(LENS)
    explicit = F_.seq_pack_len(x.cuda(), LENS)  # lengths handed over, no block in force
    torch.cuda.synchronize()
    assert torch.equal(f.cpu(), wf) and torch.equal(r.cpu(), wr) and torch.equal(both.cpu(), torch.cat([wf, wr], 1))
    assert only_r[0] is None and torch.equal(only_r[1].cpu(), wr)
    assert torch.equal(explicit[0].cpu(), wf) and torch.equal(explicit[1].cpu(), wr)
    assert torch.equal(y.cpu(), wy) and torch.equal(yr.cpu(), wyr)
    assert torch.equal(y_halves[0].cpu(), wy) and y_halves[1] is None
    assert torch.equal(y_cat.cpu(), torch.cat([wy, wyr], 1))


# --------------------------------------------------------------------------------
# 2. the shared-weight classes against the oracle on each sentence alone
# --------------------------------------------------------------------------------
CELLS = [("liGRU", "ligru", "relu"), ("GRU", "gru", "tanh"), ("LSTM", "lstm", "tanh"), ("RNN", "rnn", "relu"),
         ("minimalGRU", "minimalgru", "relu")]
D_IN = 6


@contextlib.contextmanager
def _one_cpu_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _opts(pre, H, act, norm, bidir):
    """norm = "bn": BatchNorm in both layers; "ln": per-step LayerNorm in both layers plus LayerNorm of the input."""
    ln = norm == "ln"
    return {pre + "_lay": "%d,%d" % (H, H), pre + "_drop": "0.2,0.1", pre + "_use_laynorm_inp": str(ln),
            pre + "_use_batchnorm_inp": "False", pre + "_use_laynorm": "%s,%s" % (ln, ln),
            pre + "_use_batchnorm": "%s,%s" % (not ln, not ln), pre + "_bidir": str(bidir), pre + "_act": "%s,%s" % (act, act),
            pre + "_orthinit": "True", "use_cuda": "True", "to_do": "forward"}


_CASES = {}


def _case(kind, pre, act, H, norm, bidir, prec):
    """(module on the CPU, the padded batch, the oracle's output of every sentence alone): built once per configuration
    and shared by the tests that need it (the rec_algo settings), never changed."""
    key = (kind, H, norm, bidir, prec)
    if key in _CASES:
        return _CASES[key]
    opts = _opts(pre, H, act, norm, bidir)
    with _one_cpu_thread():
        torch.manual_seed(11)
        net = getattr(nn_amd, kind)(opts, D_IN)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():  # normalisation parameters away from (1, 0), running statistics away from (0, 1)
        for name, q in net.named_parameters():
            head, leaf = name.split(".")[0], name.split(".")[-1]
            if leaf == "gamma" or (head.startswith("bn") and leaf == "weight"):
                q.mul_(1.0 + 0.3 * torch.randn(q.shape, generator=g))
            elif leaf == "beta" or (head.startswith("bn") and leaf == "bias"):
                q.add_(0.2 * torch.randn(q.shape, generator=g))
        for name, b_ in net.named_buffers():
            if name.endswith("running_mean"):
                b_.add_(0.3 * torch.randn(b_.shape, generator=g))
            elif name.endswith("running_var"):
                b_.mul_(0.5 + torch.rand(b_.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    sentences = [torch.randn(n, D_IN, generator=g) for n in LENS]
    x, lens = padded_batch(sentences)
    with (O.bf16_operands() if prec == "bf16" else contextlib.nullcontext()), torch.no_grad():
        want = [O.recurrent_forward(kind, opts, sd, s.view(-1, 1, D_IN), training=False, to_do="forward")[:, 0] for s in sentences]
    _CASES[key] = (net, x, lens, want)
    return _CASES[key]


def _grade(tag, y, lens, want, tol, padding_is_zero):
    y = y.detach().cpu()
    errs = [rel_err(y[:n, b], want[b]) for b, n in enumerate(lens)]
    pad = max([float(y[n:, b].abs().max()) for b, n in enumerate(lens) if n < y.shape[0]] or [0.0])
    print("\n%s: per sentence %s, largest padding element %.1e" % (tag, " ".join("%.2e" % e for e in errs), pad))
    assert bool(torch.isfinite(y).all())
    assert max(errs) < tol, errs
    if padding_is_zero:
        assert pad == 0.0


def _run_class(kind, pre, act, H, norm, bidir, prec, algo):
    net, x, lens, want = _case(kind, pre, act, H, norm, bidir, prec)
    F_.set_precision(prec)
    F_.set_rec_algo(algo)
    net = net.cuda().eval()
    with torch.no_grad(), F_.sentence_lengths(lens):
        y = net(x.cuda())
    torch.cuda.synchronize()
    _lib.raise_if_persist_failed()
    assert tuple(y.shape) == (T_MAX, len(lens), (2 if bidir else 1) * H)
    assert getattr(y, "_pk_twin", None) is None or not bidir
    _grade("%s H=%d %s %s %s rec_algo=%s" % (kind, H, norm, "bidir" if bidir else "uni", prec, algo), y, lens, want,
           TOL[prec], bidir)


@pytest.mark.parametrize("algo", ["auto", "stepwise"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [13, 16])
@pytest.mark.parametrize("kind,pre,act", CELLS)
def test_bidirectional_batchnorm_stack_equals_each_sentence_alone(kind, pre, act, H, prec, algo):
    _run_class(kind, pre, act, H, "bn", True, prec, algo)


@pytest.mark.parametrize("algo", ["auto", "stepwise"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,pre,act", CELLS)
def test_bidirectional_layernorm_stack_equals_each_sentence_alone(kind, pre, act, prec, algo):
    _run_class(kind, pre, act, 16, "ln", True, prec, algo)


@pytest.mark.parametrize("algo", ["auto", "stepwise"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,pre,act", CELLS)
def test_unidirectional_stack_equals_each_sentence_alone(kind, pre, act, prec, algo):
    _run_class(kind, pre, act, 13, "bn", False, prec, algo)


def test_plain_time_reversal_is_not_each_sentence_alone():
    """The same batch WITHOUT the lengths block: the backward direction of a short sentence starts in the padding, and
    its rows are not what the sentence gives alone - the comparison above is not vacuous."""
    net, x, lens, want = _case("liGRU", "ligru", "relu", 16, "bn", True, "fp32")
    net = net.cuda().eval()
    with torch.no_grad():
        y = net(x.cuda()).cpu()
    errs = [rel_err(y[:n, b], want[b]) for b, n in enumerate(lens)]
    print("\nwithout sentence_lengths: per sentence %s" % " ".join("%.2e" % e for e in errs))
    assert all(e < 1e-4 for e, n in zip(errs, lens) if n == T_MAX)
    assert all(e > 1e-2 for e, n in zip(errs, lens) if n < T_MAX)


def test_lengths_block_with_autograd_on():
    """Parameters that require grad and autograd enabled (an input without grad): the same values; the result carries
    no autograd history (forward only)."""
    net, x, lens, want = _case("liGRU", "ligru", "relu", 16, "bn", True, "fp32")
    net = net.cuda().eval()
    with F_.sentence_lengths(lens):
        y = net(x.cuda())
    torch.cuda.synchronize()
    assert not y.requires_grad
    _grade("liGRU, autograd on", y, lens, want, TOL["fp32"], True)


# --------------------------------------------------------------------------------
# 3. QLSTM, LSTM_cudnn, RNN_cudnn against their own B = 1 forward
# --------------------------------------------------------------------------------
def _other(kind):
    if kind == "QLSTM":
        np.random.seed(21)
        net = nn_amd.QLSTM({"lstm_lay": "12,16", "lstm_drop": "0.2,0.1", "lstm_act": "tanh,tanh", "lstm_bidir": "True",
                            "autograd": "False", "use_cuda": "True", "to_do": "forward"}, 8)
        d_in = 8
    else:
        torch.manual_seed(22)
        opts = {"hidden_size": "13", "num_layers": "2", "bias": "True", "batch_first": "False", "dropout": "0.2",
                "bidirectional": "True", "nonlinearity": "relu", "use_cuda": "True", "to_do": "forward"}
        net = getattr(nn_amd, kind)(opts, D_IN)
        d_in = D_IN
    g = torch.Generator().manual_seed(23)
    with torch.no_grad():
        for name, q in net.named_parameters():
            if "bias" in name:
                q.copy_(0.2 * torch.randn(q.shape, generator=g))
    sentences = [torch.randn(n, d_in, generator=g) for n in LENS]
    return net.cuda().eval(), sentences


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["QLSTM", "LSTM_cudnn", "RNN_cudnn"])
def test_other_bidirectional_classes_equal_their_own_single_sentence_forward(kind, prec):
    net, sentences = _other(kind)
    x, lens = padded_batch(sentences)
    F_.set_precision(prec)
    with torch.no_grad():
        want = [net(s.view(len(s), 1, -1).cuda())[:, 0].cpu() for s in sentences]
        with F_.sentence_lengths(lens):
            y = net(x.cuda())
    torch.cuda.synchronize()
    _lib.raise_if_persist_failed()
    assert tuple(y.shape) == (T_MAX, len(lens), net.out_dim)
    _grade("%s %s against its own B = 1 forward" % (kind, prec), y, lens, want, TOL[prec], True)


# --------------------------------------------------------------------------------
# 4. run_nn_dp with PK_FORWARD_BATCH on the chunk the reference's run_nn decoded
# --------------------------------------------------------------------------------
def _chunk_setup(tmp_path):
    from test_core_chunk import CASE, checkpoint_from_fixture

    g = Golden(CASE)
    for i in (1, 2, 3):
        torch.save(checkpoint_from_fixture(g, "ck1", "architecture%d" % i), tmp_path / ("ck1_architecture%d.pkl" % i))
    with open(tmp_path / "counts", "w") as f:
        f.write("[ " + " ".join(str(int(c)) for c in g.arrays["counts"]) + " ]\n")
    return g


def _decode(g, cfg_text, out, arch_dict, monkeypatch, n):
    """One forward chunk with PK_FORWARD_BATCH = n: (forward_model calls, the info section, {ark name: records})."""
    from test_core_chunk import parse_ark

    meta = g.meta
    data, end = g.arrays["data_set"], g.arrays["data_end_index"]
    monkeypatch.setenv("PK_FORWARD_BATCH", str(n))
    calls = []
    real = core.forward_model

    def counting(*a, **kw):
        calls.append(tuple(a[6].shape))
        return real(*a, **kw)

    monkeypatch.setattr(core, "forward_model", counting)
    path = out / "forward.cfg"
    path.write_text(cfg_text)
    args = [meta["data_name"], torch.from_numpy(data).cuda(), end, {k: list(v) for k, v in meta["fea_dict"].items()},
            meta["lab_dict"], arch_dict]
    core.run_nn_dp(*args, str(path), False, str(path), reader=lambda *a: None)
    monkeypatch.setattr(core, "forward_model", real)
    info = configparser.ConfigParser()
    info.read(out / "forward.info")
    arks = {p.name: parse_ark(open(p, "rb").read()) for p in sorted(out.glob("forward_*.ark"))}
    return calls, info["results"], arks


@pytest.mark.parametrize("n,n_calls", [(4, 3), (16, 1)])
def test_run_nn_dp_decodes_the_reference_chunk_in_batches(tmp_path, monkeypatch, n, n_calls):
    from test_core_chunk import engine_cfg, parse_ark

    g = _chunk_setup(tmp_path)
    calls, res, arks = _decode(g, engine_cfg(g, "forward", tmp_path), tmp_path, g.meta["arch_dict"], monkeypatch, n)
    lens = np.diff(g.arrays["data_end_index"], prepend=0)
    assert len(calls) == n_calls, calls
    assert calls == [(int(max(lens[s:s + n])), len(lens[s:s + n]), g.arrays["data_set"].shape[1]) for s in range(0, len(lens), n)]
    assert "loss" not in res
    got = arks["forward_out_dnn2_to_decode.ark"]
    want = parse_ark(bytes(g.arrays["ark"]))
    assert [k for k, _ in got] == [k for k, _ in want] == g.meta["data_name"]
    errs = []
    for (_, a), (_, b) in zip(got, want):
        assert a.shape == b.shape
        errs.append(rel_err(torch.from_numpy(a.copy()), torch.from_numpy(b.copy())))
    print("\nPK_FORWARD_BATCH=%d: %d forward_model calls %s, worst sentence against the reference's ark %.2e" % (n, len(calls), calls, max(errs)))
    assert max(errs) < 1e-4, errs


def test_run_nn_dp_decodes_an_mlp_recipe_in_groups(tmp_path, monkeypatch):
    """The MLP-trunk variant of the recipe (test_core_chunk.py::test_run_nn_dp_hip_graph_replay_equals_eager builds it the
    same way), two forward outputs: the frames of four sentences back to back against sentence by sentence."""
    from test_core_chunk import engine_cfg

    g = _chunk_setup(tmp_path)
    cp = configparser.ConfigParser()
    cp.read_string(engine_cfg(g, "forward", tmp_path))
    a1 = cp["architecture1"]
    for k in [k for k in a1 if k.startswith("ligru_")]:
        del a1[k]
    a1["arch_class"], a1["arch_seq_model"] = "MLP", "False"
    a1.update({"dnn_lay": "32,32", "dnn_drop": "0.0,0.0", "dnn_use_laynorm_inp": "False", "dnn_use_batchnorm_inp": "False",
               "dnn_use_batchnorm": "True,True", "dnn_use_laynorm": "False,False", "dnn_act": "relu,relu"})
    for sec in ("architecture1", "architecture2", "architecture3"):  # (seeded initial weights: the checkpoints are the Li-GRU recipe's)
        cp[sec]["arch_pretrain_file"] = "none"
    cp["forward"].update({"forward_out": "out_dnn2,out_dnn3", "normalize_posteriors": "True,False",
                          "normalize_with_counts_from": "%s,none" % (tmp_path / "counts"), "require_decoding": "True,False"})
    arch_dict = {k: list(v) for k, v in g.meta["arch_dict"].items()}
    arch_dict["liGRU_layers"][2] = False
    buf = io.StringIO()
    cp.write(buf)
    runs = {}
    for n in (1, 4):
        out = tmp_path / ("n%d" % n)
        out.mkdir()
        text = buf.getvalue().replace(str(tmp_path) + "/forward.info", str(out) + "/forward.info")
        calls, _, arks = _decode(g, text, out, arch_dict, monkeypatch, n)
        runs[n] = (calls, arks)
    lens = np.diff(g.arrays["data_end_index"], prepend=0)
    assert [c[0] for c in runs[1][0]] == list(lens)
    assert [c[0] for c in runs[4][0]] == [int(lens[s:s + 4].sum()) for s in range(0, len(lens), 4)]
    assert sorted(runs[1][1]) == sorted(runs[4][1]) == ["forward_out_dnn2_to_decode.ark", "forward_out_dnn3.ark"]
    worst = 0.0
    for name, one in runs[1][1].items():
        four = runs[4][1][name]
        assert [k for k, _ in four] == [k for k, _ in one] == g.meta["data_name"]
        for (_, a), (_, b), n_frames in zip(four, one, lens):
            assert a.shape == b.shape and a.shape[0] == n_frames
            worst = max(worst, rel_err(torch.from_numpy(a.copy()), torch.from_numpy(b.copy())))
    print("\nMLP recipe, PK_FORWARD_BATCH=4 against 1: worst sentence %.2e" % worst)
    assert worst < 1e-4


# --------------------------------------------------------------------------------
# 5. refusals: PkError before anything is launched
# --------------------------------------------------------------------------------
class _NoLaunch:
    """Every stream-taking entry of the library raises while the block is open: a refusal must come before any launch."""

    def __enter__(self):
        self.lib = _lib.load()
        self.calls = []
        self.real = F_._lib.load
        outer = self

        class Spy:
            def __getattr__(self, name):
                fn = getattr(outer.lib, name)
                sig = _lib.SIGNATURES.get(name)
                if sig is None or not sig[1] or sig[1][0] is not _lib.P:
                    return fn

                def launched(*a):
                    outer.calls.append(name)
                    return fn(*a)

                return launched

        F_._lib.load = lambda: Spy()
        return self

    def __exit__(self, *exc):
        F_._lib.load = self.real
        return False


def _refused(net, x, lens):
    with _NoLaunch() as spy:
        with pytest.raises(_lib.PkError):
            with F_.sentence_lengths(lens):
                net(x)
    assert spy.calls == [], spy.calls
    assert F_.current_lengths() is None


@pytest.mark.parametrize("kind", ["liGRU", "liGRU_uni", "QLSTM", "LSTM_cudnn"])
def test_refusals(kind):
    if kind.startswith("liGRU"):
        bidir = kind == "liGRU"
        net = _case("liGRU", "ligru", "relu", 16, "bn", bidir, "fp32")[0].cuda().eval()
        x = torch.randn(T_MAX, len(LENS), D_IN, device="cuda")
    else:
        net, sentences = _other(kind)
        x = padded_batch(sentences)[0].cuda()
    torch.cuda.synchronize()
    try:
        net.train()
        _refused(net, x, LENS)  # training mode: batch statistics / dropout over padding
    finally:
        net.eval()
    _refused(net, x, (7, 0, 4, 7, 2))  # a length of 0
    _refused(net, x, (7, 1, 8, 7, 2))  # above T
    _refused(net, x, LENS[:4])  # a length count different from B
    _refused(net, x, LENS + (3,))
    _refused(net, x.clone().requires_grad_(True), LENS)  # a grad-requiring input with autograd on
    with torch.no_grad(), F_.sentence_lengths(LENS):  # ... which autograd off accepts
        y = net(x.clone().requires_grad_(True))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
