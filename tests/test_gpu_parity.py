"""GPU parity of the HIP engine (through the C-ABI) against (i) the golden fixtures
dumped from the reference's own classes and (ii) the CPU oracle on seeded inputs.

Tolerance: north_star asks for 1e-4 relative fp32 on posteriors / loss / gradients;
errors are norm-relative per tensor.  The engine runs in its
exact-fp32 mode here (v_mfma_f32_* MFMA); the bf16 perf mode has its own looser test.
"""
import contextlib
import importlib

import pytest
import torch

import pk_oracle as O
from golden_util import Golden, check_grads, list_cases, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
# every module fixture, the "ora_" option combinations included (per-step LayerNorm in the gated cells, input
# normalisations, eval mode of every cell, BatchNorm in SincNet / CNN)
_SKIP = ("e2e_", "chunk_", "io_", "train_", "scale_")
MODULE_CASES = [c for c in list_cases() if not c.startswith(_SKIP)]
PERSISTENT_OK = ("liGRU", "RNN", "LSTM", "GRU", "minimalGRU")  # (round 6: the fourth-generation fp32 kernels take the last three)


@pytest.fixture(autouse=True)
def _fp32_mode():
    F_ = importlib.import_module("pytorch-kaldi_amd.functional")
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")
    yield
    F_.set_precision("fp32")
    F_.set_rec_algo("auto")


def _check_case(case, algo):
    from engine_util import F_amd, build_engine, run_engine

    g = Golden(case)
    m = g.meta
    # (nothing skips any more: odd LSTM widths and per-step LayerNorm of LSTM / GRU / minimalGRU in exact fp32 run on the
    # fourth-generation kernels, which exchange 16-byte chunks at a padded pitch)
    F_amd.set_rec_algo(algo)
    net = build_engine(m, g.group("sd/"))
    has_bwd = "dx" in g.arrays
    y, dx, grads = run_engine(net, m, g.t("x"), g.masks(), g.t("cot") if has_bwd else None)
    assert rel_err(y, g.t("y")) < TOL, rel_err(y, g.t("y"))
    if has_bwd:
        assert rel_err(dx, g.t("dx")) < TOL, rel_err(dx, g.t("dx"))
        ref = g.group("grad/")
        worst = check_grads(grads, ref, m, TOL)
        # parameters the reference leaves without a gradient (unused ln/bn) must stay without one
        for k, v in grads.items():
            if k not in ref:
                assert v is None or float(v.abs().max()) == 0.0, k
        assert worst < TOL
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for k, ref in g.group("sd_after/").items():
        if ref.is_floating_point():
            assert rel_err(sd[k], ref) < 1e-5, k
        else:
            assert int(sd[k]) == int(ref), k


@pytest.mark.parametrize("case", MODULE_CASES)
def test_golden_module_stepwise(case):
    _check_case(case, "stepwise")


@pytest.mark.parametrize("case", [c for c in MODULE_CASES if Golden(c).meta["arch_class"] in PERSISTENT_OK])
def test_golden_module_persistent(case):
    _check_case(case, "persistent")


def test_golden_e2e_forward_model():
    """The shipped Li-GRU recipe (scaled down) through the forward_model mirror:
    out_dnn1/2/3, loss_final, err_final and every parameter gradient."""
    import configparser

    from engine_util import nn_amd  # noqa: F401

    U = importlib.import_module("pytorch-kaldi_amd.utils")
    g = Golden("e2e_ligru_two_heads")
    m = g.meta
    cfg = configparser.ConfigParser()
    cfg["exp"] = {"to_do": "train", "use_cuda": "True"}
    for sec, opts in m["options"].items():
        cfg[sec] = {k: v.replace("%", "%%") for k, v in opts.items()}
        cfg[sec]["arch_library"] = "pytorch-kaldi_amd.nn"
    nfea = m["nfea"]
    fea_dict = {"fmllr": ["fmllr", "lst", "opts", "0", "0", 0, nfea, nfea]}
    lab_dict = {"lab_cd": ["lab_cd", "f", "o", nfea], "lab_mono": ["lab_mono", "f", "o", nfea + 1]}
    arch_dict = {"liGRU_layers": ["architecture1", "liGRU_layers", True],
                 "MLP_layers": ["architecture2", "MLP_layers", False],
                 "MLP_layers2": ["architecture3", "MLP_layers2", False]}
    inp_out_dict = {"fmllr": fea_dict["fmllr"][5:]}
    nns, costs = U.model_init(inp_out_dict, m["model"], cfg, arch_dict, True, False, "train")
    for name, net in nns.items():
        net.load_state_dict(g.group("sd/%s/" % name))
        net.cuda()
    masks = g.masks()
    rec = nns["liGRU_layers"]
    orig_forward = rec.forward
    rec.forward = lambda x: orig_forward(x, drop_masks=masks)
    inp = g.t("inp").cuda()
    outs = U.forward_model(fea_dict, lab_dict, arch_dict, m["model"], nns, costs, inp, inp_out_dict, m["T"], m["B"],
                           "train", [])
    outs["loss_final"].backward()
    torch.cuda.synchronize()
    for k in ("out_dnn1", "out_dnn2", "out_dnn3"):
        assert rel_err(outs[k].reshape(g.t(k).shape), g.t(k)) < TOL, k
    assert abs(float(outs["loss_final"]) - float(g.t("loss_final"))) < TOL * abs(float(g.t("loss_final")))
    assert float(outs["err_final"]) == float(g.t("err_final"))
    for name, net in nns.items():
        ref = g.group("grad/%s/" % name)
        got = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in net.named_parameters()}
        meta = {"arch_class": "MLP" if name.startswith("MLP") else "liGRU", "options": m["options"][arch_dict[name][0]]}
        check_grads(got, ref, meta, TOL)


# --------------------------------------------------------------------------------
# oracle parity at the recipes' layer width (H = 550) on seeded inputs
# --------------------------------------------------------------------------------
def _rec_opts(pre, lay, act, bn=True, bidir=True, drop=0.2):
    n = len(lay)
    j = lambda v: ",".join([str(v)] * n)  # noqa: E731
    return {pre + "_lay": ",".join(map(str, lay)), pre + "_drop": j(drop), pre + "_use_laynorm_inp": "False",
            pre + "_use_batchnorm_inp": "False", pre + "_use_laynorm": j(False), pre + "_use_batchnorm": j(bn),
            pre + "_bidir": str(bidir), pre + "_act": j(act), pre + "_orthinit": "True", "use_cuda": "True",
            "to_do": "train"}


ORACLE_CASES = [
    # kind, prefix, act, layers, T, B, D, algo
    ("liGRU", "ligru", "relu", [550, 550], 12, 5, 40, "stepwise"),
    ("liGRU", "ligru", "relu", [550, 550], 12, 5, 40, "persistent"),
    ("liGRU", "ligru", "relu", [550], 40, 24, 40, "persistent"),
    ("LSTM", "lstm", "tanh", [550, 550], 12, 5, 40, "stepwise"),
    ("LSTM", "lstm", "tanh", [550], 30, 20, 40, "persistent"),
    ("GRU", "gru", "tanh", [550, 550], 12, 5, 40, "stepwise"),
    ("minimalGRU", "minimalgru", "relu", [96], 10, 3, 17, "stepwise"),
    # round 6: pk_rec_persist4_f32.hip - partial clusters, several clusters, odd widths, two launches (300 rows > 8 x 16 x 2)
    ("LSTM", "lstm", "tanh", [550, 550], 12, 5, 40, "persistent"),
    ("LSTM", "lstm", "tanh", [77], 9, 3, 13, "persistent"),
    ("GRU", "gru", "tanh", [550, 550], 12, 5, 40, "persistent"),
    ("GRU", "gru", "tanh", [550], 30, 20, 40, "persistent"),
    ("GRU", "gru", "relu", [61], 9, 3, 13, "persistent"),
    ("minimalGRU", "minimalgru", "relu", [96], 10, 3, 17, "persistent"),
    ("minimalGRU", "minimalgru", "tanh", [550], 16, 24, 40, "persistent"),
    ("LSTM", "lstm", "tanh", [550], 6, 150, 40, "persistent"),
    ("GRU", "gru", "tanh", [550], 6, 150, 40, "persistent"),
    ("RNN", "rnn", "relu", [130], 10, 33, 17, "persistent"),
    # pk_rec_persist2_f32.hip with two launches (400 rows > 24 clusters x 16)
    ("liGRU", "ligru", "relu", [550], 3, 200, 40, "persistent"),
]


@pytest.mark.parametrize("kind,pre,act,lay,T,B,D,algo", ORACLE_CASES)
def test_oracle_parity_h550(kind, pre, act, lay, T, B, D, algo):
    from engine_util import F_amd, nn_amd

    F_amd.set_rec_algo(algo)
    opts = _rec_opts(pre, lay, act)
    torch.manual_seed(1234)
    net = getattr(nn_amd, kind)(opts, D)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(99)
    x = torch.randn(T, B, D, generator=g)
    masks = O.make_drop_masks(kind, opts, B, "train", generator=g)
    cot = torch.randn(T, B, net.out_dim, generator=g)
    # oracle (CPU, fp32, autograd)
    osd = {k: v.clone() for k, v in sd.items()}
    for k in osd:
        if osd[k].is_floating_point() and "running" not in k:
            osd[k].requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    yo = O.recurrent_forward(kind, opts, osd, xo, training=True, to_do="train", drop_masks=masks)
    (yo * cot).sum().backward()
    # engine
    net.cuda().train()
    xe = x.clone().cuda().requires_grad_(True)
    ye = net(xe, drop_masks=masks)
    (ye * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert rel_err(ye, yo) < TOL
    # ReLU recurrences: the oracle's own gradient noise is ~4e-4 at T=100 because 1e-6 forward
    # differences flip ReLU kinks; these cases keep T short so 1e-4 holds
    gtol = TOL if T <= 16 else 3e-4
    assert rel_err(xe.grad, xo.grad) < gtol
    ref = {k: v.grad for k, v in osd.items() if v.requires_grad and v.grad is not None}
    got = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in net.named_parameters()}
    check_grads(got, ref, None, gtol)


def test_persistent_matches_stepwise_full_width():
    """Size-independent property at the BASELINE width/batch (2B = 256 rows, H = 550):
    the two recurrence algorithms evaluate the same fp32 expressions, so their outputs
    agree to rounding; and the bidirectional halves obey the time-reversal symmetry
    Y(x)[t, b, :H] == Y(flip x)[T-1-t, b, H:] when the two mask halves are swapped."""
    from engine_util import F_amd, nn_amd

    T, B, D, H = 64, 128, 40, 550
    opts = _rec_opts("ligru", [H], "relu")
    torch.manual_seed(7)
    net = nn_amd.liGRU(opts, D).cuda().train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, D, generator=g).cuda()
    mask = torch.bernoulli(torch.full((2 * B, H), 0.8), generator=g)
    outs = {}
    for algo in ("stepwise", "persistent"):
        F_amd.set_rec_algo(algo)
        with torch.no_grad():
            outs[algo] = net(x, drop_masks=[mask]).cpu()
    assert rel_err(outs["persistent"], outs["stepwise"]) < 1e-5
    swapped = torch.cat([mask[B:], mask[:B]], 0)
    with torch.no_grad():
        yf = net(torch.flip(x, dims=[0]), drop_masks=[swapped]).cpu()
    y = outs["persistent"]
    assert rel_err(torch.flip(yf[:, :, H:], dims=[0]), y[:, :, :H]) < 1e-5
    assert rel_err(torch.flip(yf[:, :, :H], dims=[0]), y[:, :, H:]) < 1e-5


@pytest.mark.parametrize("kind,pre,act,H", [("liGRU", "ligru", "relu", 550), ("LSTM", "lstm", "tanh", 550),
                                             ("GRU", "gru", "tanh", 550), ("minimalGRU", "minimalgru", "relu", 64),
                                             ("RNN", "rnn", "tanh", 128)])
def test_bf16_mode_is_close(kind, pre, act, H):
    """Perf mode: bf16 MFMA operands (bf16 copies of activations / gradients / weights in HBM,
    pk_gemm_bf16), fp32 accumulate / state / master weights.  Not the graded parity mode;
    documented tolerance: 3e-2 norm-relative on outputs, 1e-1 on gradients of a 2-layer net."""
    from engine_util import F_amd, nn_amd

    opts = _rec_opts(pre, [H, H], act)
    torch.manual_seed(11)
    net = getattr(nn_amd, kind)(opts, 40).cuda().train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(20, 8, 40, generator=g).cuda()
    masks = O.make_drop_masks(kind, opts, 8, "train", generator=g)
    res = {}
    for prec in ("fp32", "bf16"):
        F_amd.set_precision(prec)
        net.zero_grad()
        xe = x.clone().requires_grad_(True)
        y = net(xe, drop_masks=masks)
        y.square().sum().backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}
        res[prec] = (y.detach().cpu(), xe.grad.cpu(), grads)
    assert rel_err(res["bf16"][0], res["fp32"][0]) < 3e-2
    assert rel_err(res["bf16"][1], res["fp32"][1]) < 1e-1
    for k, v in res["fp32"][2].items():
        assert rel_err(res["bf16"][2][k], v) < 1e-1, k


@contextlib.contextmanager
def _one_cpu_thread():
    """Seeded inputs that are the same on every host.  The orthogonal initialisation goes through a LAPACK QR whose last
    bits change with the number of CPU threads, i.e. with the host and its OMP_NUM_THREADS; a test that compares two
    algorithms across activation kinks (one pre-activation that changes sign between them moves a gradient by per cent)
    must not draw different weights on different machines."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("kind,pre,act", [("liGRU", "ligru", "relu"), ("LSTM", "lstm", "tanh"), ("RNN", "rnn", "tanh"),
                                          ("GRU", "gru", "tanh"), ("minimalGRU", "minimalgru", "relu"),
                                          # the kernels are specialised for relu / tanh: these take the run-time switch
                                          ("liGRU", "ligru", "leaky_relu"), ("GRU", "gru", "sigmoid"), ("LSTM", "lstm", "elu")])
@pytest.mark.parametrize("H,T,B,bidir", [(550, 12, 5, True), (40, 9, 3, True), (20, 7, 4, False), (14, 5, 33, True),
                                         (129, 6, 2, True),
                                         (8, 1, 2, False),      # one step, two sequences
                                         (576, 3, 2, True),     # widest layer the register-resident U covers
                                         (24, 4, 300, True),    # 600 rows: ONE launch of 40 clusters, 15 rows each
                                         # 400 rows at 24 clusters of 16 (9 workgroups each): two launches of the cluster
                                         # grid, the second with one live cluster
                                         (550, 3, 200, True)])
@pytest.mark.parametrize("safe", [0, 1])
def test_bf16_persistent_matches_bf16_stepwise(kind, pre, act, H, T, B, bidir, safe):
    """The perf-mode persistent kernels (bf16 exchange through L2, MFMA B fragments in registers) and the
    step-wise algorithm in bf16 mode round the same operands (h_{t-1}, dgates_{t+1}, U) to bf16 and
    accumulate in fp32: they must agree far more tightly (5e-3) than bf16 vs fp32 does (3e-2)."""
    from engine_util import F_amd, nn_amd

    opts = _rec_opts(pre, [H, H], act, bidir=bidir)
    with _one_cpu_thread():
        torch.manual_seed(21)
        net = getattr(nn_amd, kind)(opts, 23).cuda().train()
        g = torch.Generator().manual_seed(13)
        x = torch.randn(T, B, 23, generator=g).cuda()
        masks = O.make_drop_masks(kind, opts, B, "train", generator=g)
        cot = torch.randn(T, B, net.out_dim, generator=g).cuda()
    F_amd.set_precision("bf16")
    lib = importlib.import_module("pytorch-kaldi_amd._lib").load()
    lib.pk_persist2_set_mode(safe)  # 1: placement-independent write-through exchange; 0: XCD-local fast path when possible
    res = {}
    for algo in ("stepwise", "persistent"):
        F_amd.set_rec_algo(algo)
        net.zero_grad()
        xe = x.clone().requires_grad_(True)
        y = net(xe, drop_masks=masks)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}
        res[algo] = (y.detach().cpu(), xe.grad.cpu(), grads)
    lib.pk_persist2_set_mode(0)
    assert rel_err(res["persistent"][0], res["stepwise"][0]) < 5e-3
    assert rel_err(res["persistent"][1], res["stepwise"][1]) < 2e-2
    for k, v in res["stepwise"][2].items():
        assert rel_err(res["persistent"][2][k], v) < 2e-2, k


@pytest.mark.parametrize("kind,pre,act", [("liGRU", "ligru", "relu"), ("RNN", "rnn", "tanh"), ("LSTM", "lstm", "tanh"),
                                          ("GRU", "gru", "tanh"), ("minimalGRU", "minimalgru", "relu")])
@pytest.mark.parametrize("H,T,B,bidir", [(550, 40, 9, True), (72, 3, 4, True), (40, 64, 3, False), (24, 9, 300, True)])
@pytest.mark.parametrize("safe", [0, 1])
def test_self_filled_exchange_on_a_dirty_buffer(kind, pre, act, H, T, B, bidir, safe):
    """The bf16 persistent kernels write the "not written yet" pattern of their exchange buffers themselves, a few
    steps ahead of their own publishes (prefilled = 2).  Run twice in a row on different inputs, so that the second
    run's buffers are the allocator's recycled blocks holding the FIRST run's perfectly valid-looking data: outputs and
    gradients must equal, bit for bit, what the whole-buffer fill (PK_EXPERIMENT rec_self_fill=0 path) gives on the second input -
    a poll that accepted a stale chunk would show up here."""
    from engine_util import F_amd, nn_amd

    opts = _rec_opts(pre, [H, H], act, bidir=bidir)
    torch.manual_seed(5)
    net = getattr(nn_amd, kind)(opts, 23).cuda().train()
    g = torch.Generator().manual_seed(17)
    xs = [torch.randn(T, B, 23, generator=g).cuda() for _ in range(4)]  # the same recycled blocks, step after step
    masks = O.make_drop_masks(kind, opts, B, "train", generator=g)
    cot = torch.randn(T, B, net.out_dim, generator=g).cuda()
    lib = importlib.import_module("pytorch-kaldi_amd._lib").load()
    assert lib.pk_rec_self_fill(F_amd.CELL[kind]) == 1
    F_amd.set_precision("bf16")
    F_amd.set_rec_algo("persistent")
    lib.pk_persist2_set_mode(safe)
    res = {}
    try:
        for self_fill in (True, False):
            F_amd.settings.self_fill = self_fill
            for x in (xs if self_fill else xs[-1:]):  # the self-filled run sees a dirty allocator
                net.zero_grad()
                xe = x.clone().requires_grad_(True)
                y = net(xe, drop_masks=masks)
                (y * cot).sum().backward()
                torch.cuda.synchronize()
                out = (y.detach().clone(), xe.grad.clone(),
                       {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
                del y, xe
            res[self_fill] = out
    finally:
        F_amd.settings.self_fill = True
        F_amd.set_rec_algo("auto")
        F_amd.set_precision("fp32")
        lib.pk_persist2_set_mode(0)
    assert lib.pk_persist2_error_count() == 0
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    for k, v in res[False][2].items():
        assert torch.equal(res[True][2][k], v), k


# --------------------------------------------------------------------------------
# BASELINE configs[1] at FULL size (Li-GRU 5x550 bidirectional + 1938/48 heads, T=500, B=128):
# the oracle needs ~400 s and 37 GB per step there, so parity is checked through
# size-independent properties of the same computation.
# --------------------------------------------------------------------------------
def _full_trainer(prec):
    from engine_util import F_amd

    R = importlib.import_module("pytorch-kaldi_amd.recipes")
    U = importlib.import_module("pytorch-kaldi_amd.utils")
    F_amd.set_precision(prec)
    F_amd.set_rec_algo("auto")
    rcp = R.recipe("timit_ligru")
    iod = {"fea": rcp["fea_dict"]["fea"][5:]}
    torch.manual_seed(2234)
    nns, costs = U.model_init(iod, rcp["model"], rcp["cfg"], rcp["arch_dict"], True, False, "train")
    return R, U, rcp, iod, nns, costs


def _fwd(U, rcp, iod, nns, costs, inp, T, B, masks):
    rec = nns[rcp["first"]]
    orig = rec.forward
    rec.forward = lambda x: orig(x, drop_masks=masks)
    try:
        return U.forward_model(rcp["fea_dict"], rcp["lab_dict"], rcp["arch_dict"], rcp["model"], nns, costs, inp, iod,
                               T, B, "train", [])
    finally:
        rec.forward = orig


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_full_size_properties(prec):
    import math

    T, B, H = 500, 128, 550
    R, U, rcp, iod, nns, costs = _full_trainer(prec)
    inp = R.synthetic_batch(rcp, T, B, 4234, "cuda")
    g = torch.Generator().manual_seed(9)
    masks = [torch.bernoulli(torch.full((2 * B, H), 0.8), generator=g).cuda() for _ in range(5)]
    outs = _fwd(U, rcp, iod, nns, costs, inp, T, B, masks)
    # (1) fresh network, uniform labels: loss_final = ln(1938) + ln(48) up to the spread of a random init
    loss0 = float(outs["loss_final"])
    assert abs(loss0 - (math.log(1938) + math.log(48))) < 0.05
    # log-posteriors are normalised: sum(exp) == 1 for every frame
    p = outs["out_dnn2"].exp().sum(1)
    assert float((p - 1).abs().max()) < 1e-3
    # (2) time-reversal symmetry of a bidirectional layer at full T and B: flipping the input in time and swapping
    #     the mask halves swaps the two direction halves of the output (the reference's cat/flip identity; it
    #     holds per layer - the next layer sees the halves in swapped feature positions)
    rec1 = nns[rcp["first"]]
    x1 = inp[:, :, :rcp["nfea"]]
    saved_lay = rec1._n_lay
    rec1._n_lay = 1
    try:
        with torch.no_grad():
            y = rec1(x1, drop_masks=masks[:1])
            yf = rec1(torch.flip(x1, dims=[0]), drop_masks=[torch.cat([masks[0][B:], masks[0][:B]], 0)])
    finally:
        rec1._n_lay = saved_lay
    tol = 1e-4 if prec == "fp32" else 3e-2
    assert rel_err(torch.flip(yf[:, :, H:], dims=[0]), y[:, :, :H]) < tol
    assert rel_err(torch.flip(yf[:, :, :H], dims=[0]), y[:, :, H:]) < tol
    # (3) backward against a central finite difference of the loss along a random direction in the top
    #     recurrent layer's input weights and the senone head (gradients are what training consumes)
    outs["loss_final"].backward()
    rec, head = nns[rcp["first"]], nns["MLP_layers"]
    params = [rec.wh[4].weight, rec.wz[4].weight, rec.uh[4].weight, head.wx[0].weight]
    dirs = [torch.randn(q.shape, generator=g).cuda() for q in params]
    for d in dirs:
        d /= d.norm()
    analytic = sum(float((q.grad * d).sum()) for q, d in zip(params, dirs))
    eps = 2e-2
    vals = []
    for sgn in (+1, -1):
        with torch.no_grad():
            for q, d in zip(params, dirs):
                q.add_(d, alpha=sgn * eps)
            vals.append(float(_fwd(U, rcp, iod, nns, costs, inp, T, B, masks)["loss_final"]))
            for q, d in zip(params, dirs):
                q.add_(d, alpha=-sgn * eps)
    numeric = (vals[0] - vals[1]) / (2 * eps)
    assert abs(numeric - analytic) < (2e-2 if prec == "fp32" else 1e-1) * max(abs(numeric), abs(analytic), 1e-3), (numeric, analytic)
    importlib.import_module("pytorch-kaldi_amd.functional").set_precision("fp32")


def test_side_stream_weight_gradients_equal_the_autograd_path():
    """Perf mode: dW / dU GEMMs on the second stream accumulating into the flat .grad buffer (FlatParams) give the
    same gradients as the plain autograd path, step after step (zero_grad / optimizer step join the side stream)."""
    optim_ = importlib.import_module("pytorch-kaldi_amd.optim")
    F_ = importlib.import_module("pytorch-kaldi_amd.functional")
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    opts = {"ligru_lay": "72,72", "ligru_drop": "0.0,0.0", "ligru_use_laynorm_inp": "False", "ligru_use_batchnorm_inp": "False",
            "ligru_use_laynorm": "False,False", "ligru_use_batchnorm": "True,True", "ligru_bidir": "True",
            "ligru_act": "relu,relu", "ligru_orthinit": "True", "use_cuda": "True", "to_do": "train"}
    old_prec, old_side = F_.settings.precision, F_.settings.wgrad_side
    F_.set_precision("bf16")
    try:
        grads = {}
        for side in (False, True):
            F_.settings.wgrad_side = side
            torch.manual_seed(5)
            net = nn_amd.liGRU(dict(opts), 24).cuda().train()
            head = nn_amd.MLP({"dnn_lay": "37", "dnn_drop": "0.0", "dnn_use_laynorm_inp": "False",
                               "dnn_use_batchnorm_inp": "False", "dnn_use_batchnorm": "False", "dnn_use_laynorm": "False",
                               "dnn_act": "softmax", "use_cuda": "True", "to_do": "train"}, 144).cuda().train()
            flat, hflat = optim_.FlatParams(net), optim_.FlatParams(head)
            x = torch.randn(300, 16, 24, generator=torch.Generator().manual_seed(6)).cuda()  # 4800 rows: Linear takes the side path too
            for _ in range(2):  # second pass: accumulation on top of a zeroed buffer again
                flat.zero_grad()
                hflat.zero_grad()
                head(net(x).reshape(4800, 144)).square().mean().backward()
                F_.join_side()
            grads[side] = torch.cat((flat.grad, hflat.grad)).clone()
        assert float(grads[True].abs().max()) > 0
        assert rel_err(grads[True], grads[False]) < 1e-6
    finally:
        F_.set_precision(old_prec)
        F_.settings.wgrad_side = old_side


@pytest.mark.parametrize("kind,pre,act", [("liGRU", "ligru", "relu"), ("GRU", "gru", "tanh"), ("LSTM", "lstm", "tanh")])
def test_training_step_context_leaves_the_gradients_of_the_autograd_path(kind, pre, act):
    """Inside functional.accumulating_backward (what run_nn's step wraps forward and backward in) a recurrent layer takes
    its BatchNorm scales / shifts as views of the flat buffer - no concatenation, one draw for all layers' masks - and the
    BatchNorm backward adds d gamma / d beta to the flat .grad itself (pk_bn_bwd_bf16's acc arguments).  Same gradients
    and running statistics as the step outside the context, where they travel through torch.cat and AccumulateGrad; two
    steps (the second accumulates on a zeroed buffer again), two layers, dropout masks injected."""
    optim_ = importlib.import_module("pytorch-kaldi_amd.optim")
    F_ = importlib.import_module("pytorch-kaldi_amd.functional")
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    opts = _rec_opts(pre, [72, 72], act, drop=0.2)
    T, B, D = 40, 16, 24
    old_prec = F_.settings.precision
    F_.set_precision("bf16")
    try:
        res = {}
        x = torch.randn(T, B, D, generator=torch.Generator().manual_seed(6)).cuda()
        masks = [(torch.rand(2 * B, 72, generator=torch.Generator().manual_seed(70 + i)) > 0.2).float() for i in range(2)]
        for inside in (False, True):
            torch.manual_seed(5)
            net = getattr(nn_amd, kind)(dict(opts), D).cuda().train()
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
        for a, b in zip(res[True][0], res[False][0]):
            assert float(a.abs().max()) > 0 and rel_err(a, b) < 1e-6
        for k, v in res[False][1].items():
            assert torch.equal(v, res[True][1][k]), k
    finally:
        F_.set_precision(old_prec)


def test_hip_graph_replay_trains_like_eager_steps():
    """graphs.GraphedStep: an MLP training step (forward, NLL, backward, fused RMSprop) captured once and replayed on
    new batches ends with the same parameters, optimizer state and step count as the eager loop."""
    optim_ = importlib.import_module("pytorch-kaldi_amd.optim")
    graphs = importlib.import_module("pytorch-kaldi_amd.graphs")
    F_ = importlib.import_module("pytorch-kaldi_amd.functional")
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    opts = {"dnn_lay": "64,48,11", "dnn_drop": "0.0,0.0,0.0", "dnn_use_laynorm_inp": "False", "dnn_use_batchnorm_inp": "False",
            "dnn_use_batchnorm": "True,True,False", "dnn_use_laynorm": "False,False,False", "dnn_act": "relu,relu,softmax",
            "use_cuda": "True", "to_do": "train"}
    g = torch.Generator().manual_seed(9)
    batches = [torch.randn(32, 20, generator=g).cuda() for _ in range(7)]
    labels = [torch.randint(0, 11, (32,), generator=g).cuda() for _ in range(7)]
    packed = [torch.cat((b, l.float()[:, None]), 1) for b, l in zip(batches, labels)]
    old = F_.settings.precision
    F_.set_precision("bf16")
    try:
        results = []
        for use_graph in (False, True):
            torch.manual_seed(4)
            net = nn_amd.MLP(dict(opts), 20).cuda().train()
            opt = optim_.FusedOptimizer(optim_.FlatParams(net), "rmsprop", 1e-3, alpha=0.95, eps=1e-8)

            def step(inp):
                opt.zero_grad()
                loss = torch.nn.functional.nll_loss(net(inp[:, :20]), inp[:, 20].long())
                loss.backward()
                opt.step()
                return loss.detach()

            losses = [step(packed[i]) for i in range(3)]
            if use_graph:
                gs = graphs.GraphedStep(step, [opt]).capture(packed[3])
                losses += [gs(packed[i]).clone() for i in range(3, 7)]
            else:
                losses += [step(packed[i]) for i in range(3, 7)]
            torch.cuda.synchronize()
            results.append((opt.flat.flat.clone(), opt.bufs["square_avg"].clone(), opt.steps, torch.stack(losses),
                            net.bn[0].num_batches_tracked.item()))
        (p0, s0, n0, l0, t0), (p1, s1, n1, l1, t1) = results
        assert n0 == n1 == 7 and t0 == t1 == 7
        assert torch.equal(l0, l1) and torch.equal(p0, p1) and torch.equal(s0, s1)
        with pytest.raises(Exception):
            graphs.GraphedStep(step, [optim_.FusedOptimizer(optim_.FlatParams(nn_amd.MLP(dict(opts), 20).cuda()), "adam", 1e-3)])
    finally:
        F_.set_precision(old)


def test_single_row_batchnorm_training_raises_like_torch():
    """T = B = 1 with BatchNorm in training mode: torch's BatchNorm1d (the reference) raises ValueError."""
    from engine_util import nn_amd

    net = nn_amd.liGRU(_rec_opts("ligru", [8], "relu", bidir=False), 5).cuda().train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(torch.randn(1, 1, 5).cuda())
    ref = torch.nn.BatchNorm1d(8).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ref(torch.randn(1, 8))


@pytest.mark.parametrize("kind,pre,act", [("liGRU", "ligru", "relu"), ("GRU", "gru", "tanh"), ("LSTM", "lstm", "tanh")])
def test_bf16_eval_forward_is_close(kind, pre, act):
    """Validation / forward chunks (to_do != train, module.eval(), no_grad): the perf pipeline folds the running
    BatchNorm statistics and the (1 - p) dropout scalar and must stay within the bf16 tolerance of the fp32 path."""
    from engine_util import F_amd, nn_amd

    opts = _rec_opts(pre, [72, 72], act)
    opts["to_do"] = "valid"
    torch.manual_seed(17)
    net = getattr(nn_amd, kind)(opts, 30).cuda()
    with torch.no_grad():
        for b in net.buffers():
            if b.dtype.is_floating_point:
                b.add_(0.2 * torch.rand_like(b))
    net.eval()
    x = torch.randn(31, 6, 30, generator=torch.Generator().manual_seed(2)).cuda()
    outs = {}
    for prec in ("fp32", "bf16"):
        F_amd.set_precision(prec)
        with torch.no_grad():
            outs[prec] = net(x).cpu()
    assert rel_err(outs["bf16"], outs["fp32"]) < 3e-2


# --------------------------------------------------------------------------------
# the FULL launch geometry, value for value: 2B = 256 rows x H = 550 (16 clusters live), both precisions
# --------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [20, 50])
@pytest.mark.parametrize("kind,pre,act", [("liGRU", "ligru", "relu"), ("LSTM", "lstm", "tanh"), ("GRU", "gru", "tanh")])
def test_full_geometry_value_for_value(kind, pre, act, T, prec):
    """The recurrent kernels at the geometry bench.py times - batch 128 bidirectional = 256 rows, H = 550, every one of
    the 16 clusters live, two layers so that the layer-to-layer hand-over of the bf16 copy is on the path too - compared
    VALUE FOR VALUE with the oracle on the host CPU: fp32 mode against the fp32 oracle at 1e-4, bf16 mode (the
    persistent bf16 kernels: liGRU, the 8-wave LSTM, the two-phase GRU) against the oracle's bf16-operand model at
    5e-3 (outputs) / 2e-2 (gradients).  The Li-GRU's ReLU recurrence is differentiated on the oracle run's own kink
    pattern on both sides (kink-forced backward), so that the gradient comparison measures arithmetic at any T."""
    import contextlib

    from engine_util import F_amd, nn_amd

    B, D, H = 128, 40, 550
    opts = _rec_opts(pre, [H, H], act)
    torch.manual_seed(4321)
    net = getattr(nn_amd, kind)(opts, D)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(17)
    x = torch.randn(T, B, D, generator=g)
    masks = O.make_drop_masks(kind, opts, B, "train", generator=g)
    cot = torch.randn(T, B, net.out_dim, generator=g)
    osd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    log = [] if act == "relu" else None
    with (O.bf16_operands() if prec == "bf16" else contextlib.nullcontext()):
        yo = O.recurrent_forward(kind, opts, osd, xo, training=True, to_do="train", drop_masks=masks, kink_log=log)
        (yo * cot).sum().backward()
    F_amd.set_precision(prec)
    F_amd.set_rec_algo("auto")
    report = F_amd.set_forced_kinks(log) if log is not None else None
    try:
        net.cuda().train()
        xe = x.clone().cuda().requires_grad_(True)
        ye = net(xe, drop_masks=masks)
        (ye * cot.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        F_amd.set_forced_kinks(None)
    otol, gtol = (TOL, TOL) if prec == "fp32" else (5e-3, 2e-2)
    e_y, e_x = rel_err(ye, yo), rel_err(xe.grad, xo.grad)
    ref = {k: v.grad for k, v in osd.items() if v.requires_grad and v.grad is not None}
    got = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in net.named_parameters()}
    worst = check_grads(got, ref, None, gtol)
    print("\nfull geometry %s T=%d %s: y %.2e, dx %.2e, worst parameter gradient %.2e%s"
          % (kind, T, prec, e_y, e_x, worst, "" if report is None else "; kink report %s" % (report,)))
    assert e_y < otol, e_y
    assert e_x < gtol, e_x
    if report is not None:  # the engine's own pattern differs from the oracle's only where a_t is rounding noise
        for flipped, total, worst_a in report:
            assert flipped < (2e-4 if prec == "fp32" else 2e-2) * total, report


# --------------------------------------------------------------------------------
# per-step LayerNorm of h_t inside the persistent time loop (the row statistics cross the 9 workgroups of a cluster)
# --------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,pre,act,bidir,B,T", [("liGRU", "ligru", "relu", True, 24, 12), ("RNN", "rnn", "tanh", False, 37, 9),
                                                     ("LSTM", "lstm", "tanh", True, 11, 10), ("liGRU", "ligru", "relu", True, 128, 6),
                                                     ("GRU", "gru", "tanh", True, 19, 8), ("minimalGRU", "minimalgru", "tanh", False, 40, 7)])
def test_per_step_layernorm_in_the_persistent_loop(kind, pre, act, bidir, B, T, prec):
    """`*_use_laynorm=True` (neural_networks.py:466-467, :1138-1139, :1444-1445) at the recipes' width H = 550: every
    cluster is 9 workgroups whose waves exchange the rows' partial sums inside each step.  Compared with the oracle
    (fp32 at 1e-4; perf mode against the oracle's bf16-operand model at 5e-3 / 2e-2) and - fp32 - with the engine's own
    step-wise algorithm, which the reference-generated `*_ln*` fixtures grade."""
    import contextlib

    from engine_util import F_amd, nn_amd

    D, H = 40, 550
    opts = _rec_opts(pre, [H, H], act, bn=False, bidir=bidir)
    opts[pre + "_use_laynorm"] = "True,True"
    torch.manual_seed(99)
    net = getattr(nn_amd, kind)(opts, D)
    with torch.no_grad():  # LayerNorm parameters away from (1, 0)
        for name, q in net.named_parameters():
            if name.startswith("ln.") and name.endswith("gamma"):
                q.mul_(1.0 + 0.3 * torch.randn_like(q))
            if name.startswith("ln.") and name.endswith("beta"):
                q.add_(0.2 * torch.randn_like(q))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, D, generator=g)
    masks = O.make_drop_masks(kind, opts, B, "train", generator=g)
    cot = torch.randn(T, B, net.out_dim, generator=g)
    osd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    log = [] if act == "relu" else None
    with (O.bf16_operands() if prec == "bf16" else contextlib.nullcontext()):
        yo = O.recurrent_forward(kind, opts, osd, xo, training=True, to_do="train", drop_masks=masks, kink_log=log)
        (yo * cot).sum().backward()
    ref = {k: v.grad for k, v in osd.items() if v.requires_grad and v.grad is not None}
    F_amd.set_precision(prec)
    net.cuda().train()
    runs = {}
    for algo in (("persistent", "stepwise") if prec == "fp32" else ("persistent",)):
        F_amd.set_rec_algo(algo)
        report = F_amd.set_forced_kinks(log) if log is not None else None
        try:
            net.zero_grad(set_to_none=True)
            xe = x.clone().cuda().requires_grad_(True)
            ye = net(xe, drop_masks=masks)
            (ye * cot.cuda()).sum().backward()
            torch.cuda.synchronize()
        finally:
            F_amd.set_forced_kinks(None)
        runs[algo] = (ye.detach().cpu(), xe.grad.cpu(),
                      {k: (q.grad.detach().cpu() if q.grad is not None else None) for k, q in net.named_parameters()})
    otol, gtol = (TOL, TOL) if prec == "fp32" else (5e-3, 2e-2)
    ye, dxe, got = runs["persistent"]
    e_y, e_x = rel_err(ye, yo), rel_err(dxe, xo.grad)
    worst = check_grads(got, ref, None, gtol)
    print("\nper-step LayerNorm, persistent, %s %s: y %.2e, dx %.2e, worst parameter gradient %.2e" % (kind, prec, e_y, e_x, worst))
    assert e_y < otol, e_y
    assert e_x < gtol, e_x
    assert any(k.startswith("ln.") and v is not None and float(v.abs().max()) > 0 for k, v in got.items())
    if "stepwise" in runs:
        ys, dxs, gs = runs["stepwise"]
        assert rel_err(ye, ys) < 2e-5 and rel_err(dxe, dxs) < 2e-5
        for k, v in gs.items():
            if v is not None:
                assert rel_err(got[k], v) < 5e-5, k


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,pre", [("liGRU", "ligru"), ("RNN", "rnn"), ("GRU", "gru")])
def test_per_step_layernorm_first_step_with_a_large_common_offset(kind, pre, prec):
    """LayerNorm is a two-pass mean / variance in the reference (neural_networks.py:23-33).  The persistent loops use a
    one-pass variance pivoted on the previous step's mean; at t = 0 there is none, and a pivot of 0 loses
    eps_fp32 * (mean / std)^2 of relative accuracy - invisible on N(0,1) states, 1e-3 when every unit of a row sits at
    ~30 +- 0.3.  The first step therefore takes one more exchange (the row's own mean first).  Here: no dropout, an input
    with a large common level, averaging candidate weights -> first-step states with mean / std >> 1; the normalised first step must match the
    fp64 two-pass evaluation to 2e-5 (fp32 kernels; the pivot-0 form is 50 x off)."""
    from engine_util import F_amd, nn_amd

    D, H, T, B = 40, 550, 3, 16
    opts = _rec_opts(pre, [H], "relu" if kind != "GRU" else "tanh", bn=False, bidir=True, drop=0.0)
    opts[pre + "_use_laynorm"] = "True"
    torch.manual_seed(7)
    net = getattr(nn_amd, kind)(opts, D)
    level = 30.0 if kind != "GRU" else 0.3  # (GRU: tanh keeps the candidate in range)
    with torch.no_grad():  # (a layer with per-step LayerNorm has no projection bias: the offset comes through the input)
        for name, q in net.named_parameters():
            if name.startswith("wh.") and name.endswith("weight"):
                q.copy_(torch.full_like(q, 1.0 / D) + 0.002 * torch.randn_like(q))   # a = mean(x) + small
            if name.endswith("weight") and name.startswith(("wz.", "wr.")):
                q.mul_(0.001)                                                         # gates ~ 0.5 with a small spread
    x = level + 0.01 * level * torch.randn(T, B, D, generator=torch.Generator().manual_seed(3))
    F_amd.set_precision(prec)
    F_amd.set_rec_algo("persistent")
    net.cuda().train()
    with torch.no_grad():
        y = net(x.cuda()).cpu().double()
    # fp64 evaluation of the first step of direction 0 (h_{-1} = 0): pre-LN state, then the reference's LayerNorm
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    xd = x[0].double()
    rnd = (lambda t: t.to(torch.bfloat16).double()) if prec == "bf16" else (lambda t: t)
    a = rnd(xd) @ rnd(sd["wh.0.weight"]).t()
    if kind == "liGRU":
        z = torch.sigmoid(rnd(xd) @ rnd(sd["wz.0.weight"]).t())
        h = (1 - z) * a.clamp_min(0)
    elif kind == "RNN":
        h = a.clamp_min(0)
    else:
        z = torch.sigmoid(rnd(xd) @ rnd(sd["wz.0.weight"]).t())
        h = (1 - z) * torch.tanh(a)
    mu, sdv = h.mean(1, keepdim=True), h.std(1, keepdim=True)
    ratio = float((mu.abs() / sdv).median())
    ref = sd["ln.0.gamma"] * (h - mu) / (sdv + 1e-6) + sd["ln.0.beta"]
    err = rel_err(y[0, :, :H], ref)
    print("\nfirst-step LayerNorm, %s %s: mean / std of the pre-LN state %.0f, first step vs fp64 two-pass: %.2e" % (kind, prec, ratio, err))
    assert ratio > 20
    assert err < (2e-5 if prec == "fp32" else 2e-3), err


# --------------------------------------------------------------------------------
# the small-batch (launch-bound) MLP step: one-launch layers, one-launch BatchNorm / activation backward, gradients
# accumulated into the flat .grad by the kernels that produce them
# --------------------------------------------------------------------------------
def test_small_batch_mlp_step_direct_gradients(monkeypatch):
    """TIMIT_MLP at its batch size (128 frames, 440 -> 1024 x 4 -> softmax head) in perf mode with flat parameters: the
    backward pass with its small-batch shortcuts on (one launch for activation / BatchNorm backward, PK_EXPERIMENT mlp_fused_bwd;
    weight and BatchNorm gradients accumulated into the flat .grad by the kernels that produce them, PK_EXPERIMENT direct_grads)
    must leave the gradients of the node-by-node backward through autograd's AccumulateGrad - same forward, same saved
    tensors; the fp32 operation order inside the BatchNorm backward differs, which flips the bf16 rounding of a few
    entries of dz per layer (measured 7e-4 at the bottom layer; two different forward kernels are 2e-2 apart, the bf16
    noise floor of this stack) - twice in a row (the second step lands on zeroed gradients again)."""
    from engine_util import F_amd, nn_amd

    optim_ = importlib.import_module("pytorch-kaldi_amd.optim")
    opts = {"dnn_lay": "1024,1024,1024,1024,200", "dnn_drop": "0.15,0.15,0.15,0.15,0.0", "dnn_use_laynorm_inp": "False",
            "dnn_use_batchnorm_inp": "False", "dnn_use_batchnorm": "True,True,True,True,False",
            "dnn_use_laynorm": "False,False,False,False,False", "dnn_act": "relu,relu,relu,relu,softmax"}
    g = torch.Generator().manual_seed(8)
    xs = [torch.randn(128, 440, generator=g).cuda() for _ in range(2)]
    labs = [torch.randint(0, 200, (128,), generator=g).cuda() for _ in range(2)]
    F_amd.set_precision("bf16")
    results = {}
    for mode in ("plain", "direct"):
        monkeypatch.setenv("PK_EXPERIMENT", "mlp_fused_bwd=0,direct_grads=0" if mode == "plain" else "mlp_fused_bwd=1,direct_grads=1")
        torch.manual_seed(3)
        net = nn_amd.MLP(opts, 440).cuda().train()
        flat = optim_.FlatParams(net)
        grads = []
        for x, lab in zip(xs, labs):
            masks = [(torch.rand(128, 1024, generator=torch.Generator().manual_seed(50 + i)) > 0.15).float() for i in range(4)]
            F_amd.set_forced_dropout([m.cuda() for m in masks])
            try:
                flat.zero_grad()
                loss = torch.nn.functional.nll_loss(net(x), lab)
                with F_amd.accumulating_backward():  # (the engine's step says so; without it nothing bypasses autograd)
                    loss.backward()
                torch.cuda.synchronize()
            finally:
                F_amd.set_forced_dropout(None)
            grads.append({k: q.grad.detach().clone() for k, q in net.named_parameters()})
        results[mode] = grads
    for step in range(2):
        for k, ref in results["plain"][step].items():
            if float(ref.abs().max()) < 1e-6:  # (the bias in front of a BatchNorm: its gradient is rounding noise around 0)
                continue
            got = results["direct"][step][k]
            assert rel_err(got, ref) < 4e-3, (step, k, rel_err(got, ref))


@pytest.mark.gpu
def test_reference_mask_stream_device_equals_host_call():
    """PK_MASK_RNG=reference (masks from the device mirror of torch's CPU generator) against reference_host (the reference's
    own torch.bernoulli call on the host, neural_networks.py:1102-1107): same seed -> the same three-layer Li-GRU outputs,
    bit for bit, over two consecutive forward calls, and the CPU generator ends in the same state."""
    from engine_util import F_amd, nn_amd

    opts = {"ligru_lay": "48,48,48", "ligru_drop": "0.2,0.3,0.2", "ligru_use_laynorm_inp": "False", "ligru_use_batchnorm_inp": "False",
            "ligru_use_laynorm": "False,False,False", "ligru_use_batchnorm": "True,True,True", "ligru_bidir": "True",
            "ligru_act": "relu,relu,relu", "ligru_orthinit": "True", "use_cuda": "True", "to_do": "train"}
    x = torch.randn(20, 6, 13, generator=torch.Generator().manual_seed(2)).cuda()
    old = F_amd.settings.mask_rng
    res = {}
    try:
        for mode in ("reference_host", "reference"):
            F_amd.set_mask_rng(mode)
            torch.manual_seed(11)
            net = nn_amd.liGRU(opts, 13).cuda().train()
            torch.manual_seed(99)
            with torch.no_grad():
                ys = [net(x).clone(), net(x).clone()]
            torch.cuda.synchronize()
            nn_amd.drain_mask_prefetch()
            res[mode] = (ys, torch.get_rng_state().clone())
    finally:
        F_amd.set_mask_rng(old)
        nn_amd.drain_mask_prefetch()
    for a, b in zip(res["reference"][0], res["reference_host"][0]):
        assert torch.equal(a, b)
    assert not torch.equal(res["reference"][0][0], res["reference"][0][1])  # (the second call drew new masks)
    assert torch.equal(res["reference"][1], res["reference_host"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,pre", [("liGRU", "ligru"), ("LSTM", "lstm"), ("GRU", "gru")])
def test_reference_masks_against_the_oracles_own_draws(kind, pre):
    """PK_MASK_RNG=reference, nothing injected: after torch.manual_seed(s) the engine's forward gives what
    the oracle gives with the masks the reference's own call draws after torch.manual_seed(s) (neural_networks.py:1102-1107,
    :430-441, :604-615) - in fp32 mode to 1e-4, over two consecutive forward calls (the stream goes on, it does not restart)."""
    from engine_util import F_amd, nn_amd

    F_amd.set_mask_rng("reference")  # (restored by conftest's settings fixture)
    opts = _rec_opts(pre, [40, 40], "relu" if kind == "liGRU" else "tanh")
    opts[pre + "_drop"] = "0.25,0.15"
    T, B, D = 12, 5, 9
    torch.manual_seed(3)
    net = getattr(nn_amd, kind)(opts, D)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(T, B, D, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(4711)
    want = []
    for _ in range(2):
        masks = O.make_drop_masks(kind, opts, B, "train")  # the reference's call on the global CPU generator
        assert all(0.0 < float(m.mean()) < 1.0 for m in masks)
        want.append(O.recurrent_forward(kind, opts, sd, x, training=True, to_do="train", drop_masks=masks))
    after = torch.get_rng_state().clone()
    net.cuda().train()
    torch.manual_seed(4711)
    with torch.no_grad():
        got = [net(x.cuda()).clone() for _ in range(2)]
    torch.cuda.synchronize()
    nn_amd.drain_mask_prefetch()
    for g_, w in zip(got, want):
        assert rel_err(g_, w) < TOL
    assert rel_err(got[0], want[1]) > 1e-2  # (other masks give another output: the comparison above is not vacuous)
    assert torch.equal(torch.get_rng_state(), after)  # torch's CPU generator stands where the reference's would
