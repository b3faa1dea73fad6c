"""Host side of the quaternion linear layers: the reference's initial values under one numpy seed, state-dict layout,
refusals, and the argument checks of the pk_quat_linear_* entries (no GPU)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from golden_util import Golden

nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
G = Golden("e2e_quat_linear_ref")
NAMES = ["r_weight", "i_weight", "j_weight", "k_weight", "bias"]
ENTRIES = {"pk_quat_linear_work_floats": 3, "pk_quat_linear_fwd": 10, "pk_quat_linear_bwd_x": 9, "pk_quat_linear_bwd_w": 12}


@pytest.mark.parametrize("cls,winit,crit", [(c, w, k) for c, ws in G.meta["inits"].items() for w in ws for k in G.meta["criteria"]])
def test_same_seed_same_initial_values_as_the_reference(cls, winit, crit):
    np.random.seed(G.meta["seed"])
    net = getattr(nn_amd, cls)(G.meta["in"], G.meta["out"], init_criterion=crit, weight_init=winit)
    ref = G.group("init/%s/%s/%s/" % (cls, winit, crit))
    sd = net.state_dict()
    assert list(sd) == list(ref) == NAMES
    for k in NAMES:
        assert sd[k].shape == ref[k].shape and torch.allclose(sd[k], ref[k], rtol=1e-6, atol=1e-7), k


def test_state_dict_loads_strictly_and_bias_forms():
    net = nn_amd.QuaternionLinear(G.meta["in"], G.meta["out"])
    net.load_state_dict(G.group("sd/"), strict=True)
    assert "seed=" in repr(net) and repr(net).startswith("QuaternionLinear(in_features=5, out_features=3, bias=True")
    off = nn_amd.QuaternionLinear(8, 8, bias=False)
    assert off.bias is None and list(off.state_dict()) == NAMES[:4]
    auto = nn_amd.QuaternionLinearAutograd(8, 8, bias=False, weight_init="random", seed=3)
    assert list(auto.state_dict()) == NAMES[:4] and not bool(auto.bias.any()) and auto.seed == 3


def test_constructor_refusals():
    with pytest.raises(ValueError):
        nn_amd.QuaternionLinear(8, 8, weight_init="random")
    with pytest.raises(ValueError):
        nn_amd.QuaternionLinearAutograd(8, 8, init_criterion="xavier")


def test_cpu_tensor_and_wrong_width_are_refused():
    net = nn_amd.QuaternionLinear(8, 8)
    with pytest.raises(_lib.PkError):
        net(torch.randn(3, 8))
    with pytest.raises(_lib.PkError, match="4 \\* 2"):
        net(torch.randn(3, 12))
    with pytest.raises(NotImplementedError):
        net(torch.randn(2, 2, 2, 8))


def test_abi_declares_and_binds_the_entries():
    text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pk_amd.h")).read()
    lib = _lib.load()
    for n, nargs in ENTRIES.items():
        assert re.search(r"\b%s\s*\(" % n, text) and hasattr(lib, n) and len(_lib.SIGNATURES[n][1]) == nargs, n


def test_bad_arguments_return_an_error_before_any_device_call():
    lib = _lib.load()
    f = 4096  # never dereferenced: the checks come first
    fwd = lambda *a: lib.pk_quat_linear_fwd(None, *a)  # noqa: E731  (prec, N, I, O, X, comps, base, bias, Y)
    bwx = lambda *a: lib.pk_quat_linear_bwd_x(None, *a)  # noqa: E731  (prec, N, I, O, dY, comps, base, dX)
    bww = lambda *a: lib.pk_quat_linear_bwd_w(None, *a)  # noqa: E731  (prec, N, I, O, X, dY, beta, dcomps, dbase, dbias, ws)
    bad = [(fwd, b"pk_quat_linear_fwd", [(0, 4, 2, 2, None, None, f, None, f), (0, 4, 2, 2, f, None, f, None, None),
                                         (0, 4, 2, 2, f, None, None, None, f), (0, 4, 2, 2, f, f, f, None, f),
                                         (0, 0, 2, 2, f, None, f, None, f), (0, 4, 0, 2, f, None, f, None, f),
                                         (0, 4, 2, 1 << 21, f, None, f, None, f), (2, 4, 2, 2, f, None, f, None, f)]),
           (bwx, b"pk_quat_linear_bwd_x", [(0, 4, 2, 2, None, None, f, f), (0, 4, 2, 2, f, None, f, None),
                                           (0, 4, 2, 2, f, None, None, f), (0, 4, 2, -1, f, None, f, f),
                                           (7, 4, 2, 2, f, None, f, f)]),
           (bww, b"pk_quat_linear_bwd_w", [(0, 4, 2, 2, None, f, 0.0, None, f, None, f), (0, 4, 2, 2, f, None, 0.0, None, f, None, f),
                                           (0, 4, 2, 2, f, f, 0.0, None, f, None, None), (0, 4, 2, 2, f, f, 0.0, None, None, None, f),
                                           (0, 4, 2, 2, f, f, 0.0, f, f, None, f), (0, 4, 2, 2, f, f, 0.5, None, f, None, f),
                                           (0, -4, 2, 2, f, f, 0.0, None, f, None, f), (3, 4, 2, 2, f, f, 0.0, None, f, None, f)])]
    for fn, name, calls in bad:
        for args in calls:
            assert fn(*args) != 0 and name in lib.pk_last_error(), (name, args)
    assert lib.pk_quat_linear_work_floats(2500, 4, 4) == 10 * (4 * 16 + 16) and lib.pk_quat_linear_work_floats(0, 4, 4) == 0


def test_qlstm_parameters_are_what_they_were():
    """QLSTM's containers now share the initialiser code: the same seed gives the fixture the parent commit passed."""
    g = Golden("e2e_qlstm_bidir_train")
    np.random.seed(g.meta["seed"])
    net = nn_amd.QLSTM(dict(g.meta["options"]), g.meta["inp_dim"])
    for k, v in g.group("init/").items():
        assert torch.allclose(net.state_dict()[k], v, rtol=1e-6, atol=1e-7), k
