"""PK_PRECISION=bf16x3 end to end: reference-produced module fixtures under set_precision("bf16x3"), graded like the fp32
mode's (tests/test_gpu_parity.py): outputs, input gradient and parameter gradients against the reference's arrays."""
import importlib

import pytest

from golden_util import Golden, check_grads, rel_err

pytestmark = pytest.mark.gpu
# measured (worst of y, dx and the parameter gradients): mlp_bn_relu_softmax 7.4e-6, ligru_bidir_bn 7.3e-6, lstm_bidir_bn
# 1.4e-5 - all at or below 5e-5, so the bar is the parity mode's own
TOL = 1e-4


@pytest.mark.parametrize("case", ["mlp_bn_relu_softmax", "ligru_bidir_bn", "lstm_bidir_bn"])
def test_reference_fixture_in_bf16x3_mode(case):
    from engine_util import F_amd, build_engine, run_engine

    g = Golden(case)
    m = g.meta
    F_amd.set_precision("bf16x3")  # (conftest's settings fixture restores the mode)
    net = build_engine(m, g.group("sd/"))
    y, dx, grads = run_engine(net, m, g.t("x"), g.masks(), g.t("cot"))
    e_y, e_x = rel_err(y, g.t("y")), rel_err(dx, g.t("dx"))
    worst = check_grads(grads, g.group("grad/"), m, float("inf"))
    print("\nbf16x3 mode, %s: y %.2e, dx %.2e, worst parameter gradient %.2e" % (case, e_y, e_x, worst))
    assert e_y < TOL and e_x < TOL and worst < TOL, (e_y, e_x, worst)


def test_routes_are_the_fp32_modes():
    F_ = importlib.import_module("pytorch-kaldi_amd.functional")
    routes = {}
    for prec in ("fp32", "bf16x3"):
        F_.set_precision(prec)
        routes[prec] = F_.rec_route("liGRU", 550, False, True, True)
    assert routes["bf16x3"] == routes["fp32"]
