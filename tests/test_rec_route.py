"""functional.rec_route - the one place that decides where a recurrent layer runs - against the functions it is composed
from (perf_path_ok, choose_rec_algo, as they stand) and against the table of library entry families below, over every
setting that any of them reads.  Host logic only: no GPU, no library."""
import importlib
import itertools

import pytest

F_ = importlib.import_module("pytorch-kaldi_amd.functional")

CELLS = ("liGRU", "RNN", "LSTM", "GRU", "minimalGRU")
WIDTHS = (1, 12, 13, 550, 576, 577)
EXPERIMENTS = (None, "rec_ln_persist=0", "rec_f32_gen4=0", "rec_f32_gen=1")

# The entry family of a layer, as the two autograd nodes used to pick it with their own `if` ladders:
#   (perf node, bf16 mode, persistent algorithm, per-step LayerNorm, two-phase cell) -> family
# The perf node runs only in bf16 mode, only persistent kernels and no layer that normalises h_t; the general node takes
# a bf16 persistent kernel when both hold and otherwise the generic entry, which takes algorithm and precision as arguments.
FAMILY = {}
for _bf, _pers, _ln, _2p in itertools.product((False, True), repeat=4):
    FAMILY[(False, _bf, _pers, _ln, _2p)] = "generic"
FAMILY[(False, True, True, False, False)] = "bf16"
FAMILY[(False, True, True, False, True)] = "2p_bf16"  # (a two-phase layer the perf node hands back: frozen BatchNorm statistics with autograd on)
FAMILY[(False, True, True, True, False)] = "bf16_ln"
FAMILY[(False, True, True, True, True)] = "2p_bf16_ln"
FAMILY[(True, True, True, False, False)] = "bf16"
FAMILY[(True, True, True, False, True)] = "2p_bf16"


@pytest.mark.parametrize("experiment", EXPERIMENTS)
@pytest.mark.parametrize("rec_algo", ["auto", "stepwise"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rec_route_is_the_old_decisions_in_one_place(monkeypatch, precision, rec_algo, experiment):
    if experiment is None:
        monkeypatch.delenv("PK_EXPERIMENT", raising=False)
    else:
        monkeypatch.setenv("PK_EXPERIMENT", experiment)
    old_prec, old_algo = F_.settings.precision, F_.settings.rec_algo
    seen = set()
    try:
        F_.set_precision(precision)
        F_.set_rec_algo(rec_algo)
        for cell, H, use_ln, use_bn, training in itertools.product(CELLS, WIDTHS, *[(False, True)] * 3):
            what = (cell, H, use_ln, use_bn, training)
            route = F_.rec_route(*what)
            assert route.perf == F_.perf_path_ok(*what), what
            if route.perf:  # this node has persistent kernels only and never asked choose_rec_algo
                assert route.algo == F_.REC_PERSISTENT, what
            else:
                assert route.algo == F_.choose_rec_algo(cell, H, use_ln), what
            key = (route.perf, precision == "bf16", route.algo == F_.REC_PERSISTENT, use_ln, cell in ("GRU", "minimalGRU"))
            assert route.family == FAMILY[key], (what, key)
            assert route.family == "generic" or route.family in F_._REC_BF16, what
            seen.add(route.family)
    finally:
        F_.set_precision(old_prec)
        F_.set_rec_algo(old_algo)
    if precision == "bf16" and rec_algo == "auto" and experiment != "rec_ln_persist=0":
        assert seen == {"generic", "bf16", "bf16_ln", "2p_bf16", "2p_bf16_ln"}
    elif precision == "bf16" and rec_algo == "auto":
        assert seen == {"generic", "bf16", "2p_bf16"}
    else:
        assert seen == {"generic"}


def _every_route(monkeypatch):
    """Every distinct RecRoute that rec_route gives over the settings enumerated above."""
    routes = set()
    old_prec, old_algo = F_.settings.precision, F_.settings.rec_algo
    try:
        for precision, rec_algo, experiment in itertools.product(("fp32", "bf16"), ("auto", "stepwise"), EXPERIMENTS):
            if experiment is None:
                monkeypatch.delenv("PK_EXPERIMENT", raising=False)
            else:
                monkeypatch.setenv("PK_EXPERIMENT", experiment)
            F_.set_precision(precision)
            F_.set_rec_algo(rec_algo)
            for what in itertools.product(CELLS, WIDTHS, *[(False, True)] * 3):
                routes.add(F_.rec_route(*what))
    finally:
        F_.set_precision(old_prec)
        F_.set_rec_algo(old_algo)
    return sorted(routes)


def test_rec_keep_y_skips_the_fp32_output_only_between_two_perf_layers(monkeypatch):
    """functional.rec_keep_y over every pair and triple of routes: an inner layer of a forward-only chunk leaves its fp32
    output unwritten only when it is a perf layer AND the layer above is one too (that one reads the bf16 copy).  The
    general node reads the fp32 tensor: a perf layer below it must write it (it used to hand over uninitialised memory
    whenever the next layer had per-step LayerNorm or H > 576).  A uniform perf stack keeps the saving on every inner
    layer - forward-only chunks at the benchmark shape depend on it."""
    routes = _every_route(monkeypatch)
    perf = [r for r in routes if r.perf]
    assert perf and len(perf) < len(routes)
    assert {r.family for r in routes} == {"generic", "bf16", "bf16_ln", "2p_bf16", "2p_bf16_ln"}
    n_false = 0
    for n in (2, 3):
        for stack in itertools.product(routes, repeat=n):
            for i in range(n):
                assert F_.rec_keep_y(stack, i, True) is True, (stack, i)
                keep = F_.rec_keep_y(stack, i, False)
                want = not (i < n - 1 and stack[i].perf and stack[i + 1].perf)
                assert keep is want, (stack, i)
                n_false += not keep
    assert n_false > 0
    for n in (1, 2, 3, 5):
        for r in perf:
            assert [F_.rec_keep_y([r] * n, i, False) for i in range(n)] == [False] * (n - 1) + [True], (r, n)
            assert all(F_.rec_keep_y([r] * n, i, True) for i in range(n)), (r, n)


def test_forced_persistent_still_raises_for_the_layers_it_cannot_cover(monkeypatch):
    """PK_REC_ALGO=persistent: rec_route raises what choose_rec_algo raises, for the layers of the general node only."""
    monkeypatch.delenv("PK_EXPERIMENT", raising=False)
    old_prec, old_algo = F_.settings.precision, F_.settings.rec_algo
    try:
        F_.set_rec_algo("persistent")
        F_.set_precision("fp32")
        with pytest.raises(F_._lib.PkError, match="persistent recurrence does not cover cell=liGRU H=577 laynorm=False"):
            F_.rec_route("liGRU", 577, False, True, True)
        assert F_.rec_route("GRU", 550, False, True, True) == (False, F_.REC_PERSISTENT, "generic")
        F_.set_precision("bf16")
        assert F_.rec_route("GRU", 550, False, True, True) == (True, F_.REC_PERSISTENT, "2p_bf16")  # (perf node: not asked)
        with pytest.raises(F_._lib.PkError, match="cell=GRU H=577"):
            F_.rec_route("GRU", 577, False, True, True)
    finally:
        F_.set_precision(old_prec)
        F_.set_rec_algo(old_algo)
