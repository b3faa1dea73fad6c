"""QLSTM without a GPU: the class against the fixtures the reference's quaternion_neural_networks.QLSTM wrote
(tools/make_golden_qlstm.py) - checkpoint layout, initialisation stream, refusals, flat layout - and the C ABI of the two
pk_quat_* entries."""
import builtins
import importlib
import re
import sys

import numpy as np
import pytest
import torch

from golden_util import Golden

nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
optim_amd = importlib.import_module("pytorch-kaldi_amd.optim")
F_amd = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

FIXTURES = ["e2e_qlstm_bidir_train", "e2e_qlstm_uni_eval"]
ORDER = ["wfx", "ufh", "wix", "uih", "wox", "uoh", "wcx", "uch"]


def _build(g):
    np.random.seed(g.meta["seed"])
    return nn_amd.QLSTM(dict(g.meta["options"]), g.meta["inp_dim"])


@pytest.mark.parametrize("case", FIXTURES)
def test_state_dict_layout_is_the_references(case):
    g = Golden(case)
    net = _build(g)
    ref, sd = g.group("sd/"), net.state_dict()
    assert list(sd) == list(ref)  # names AND order: parameters() order indexes torch optimizer state
    for k in ref:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
    assert [k for k, _ in net.named_parameters()] == list(ref)
    assert net.out_dim == g.meta["out_dim"] == g.t("y").shape[-1]
    # registration order of the reference: gate by gate w then u, components then bias inside
    n_lay = len(g.meta["options"]["lstm_lay"].split(","))
    want = ["%s.%d.%s" % (m, i, c) for m in ORDER for i in range(n_lay)
            for c in ["r_weight", "i_weight", "j_weight", "k_weight"] + (["bias"] if m.startswith("w") else [])]
    assert list(sd) == want
    # and a reference state_dict loads strictly
    res = net.load_state_dict({k: v.clone() for k, v in ref.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def _check_init(case):
    g = Golden(case)
    sd = _build(g).state_dict()
    init = g.group("init/")
    assert list(init) == list(sd)
    for k, v in init.items():
        assert torch.allclose(sd[k], v, rtol=1e-5, atol=1e-6), (case, k, float((sd[k] - v).abs().max()))
        if not k.endswith("bias"):
            assert float(v.abs().max()) > 0  # (the comparison is not one of zeros)


@pytest.mark.parametrize("case", FIXTURES)
def test_init_reproduces_the_reference_with_scipy(case):
    from scipy.stats import chi  # noqa: F401  (what the reference draws the moduli with)

    _check_init(case)


@pytest.mark.parametrize("case", FIXTURES)
def test_init_reproduces_the_reference_without_scipy(case, monkeypatch):
    """The numpy form of the chi(4) draw: every import of scipy fails for the duration of the construction (an import
    statement goes through builtins.__import__ also when the module is already loaded)."""
    real_import = builtins.__import__
    blocked = []

    def no_scipy(name, *a, **k):
        if name == "scipy" or name.startswith("scipy."):
            blocked.append(name)
            raise ImportError("scipy is blocked in this test")
        return real_import(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    _check_init(case)
    assert blocked, "the constructor never tried scipy: the test did not exercise the fallback"


def test_training_fixture_starts_from_the_constructor():
    """The training fixture's QLSTM (the first thing its generator constructed after np.random.seed)."""
    g = Golden("train_qlstm_3steps")
    np.random.seed(g.meta["seed"])
    opts = dict(g.meta["options"]["architecture1"], use_cuda="True", to_do="train")
    sd = nn_amd.QLSTM(opts, g.meta["nfea"]).state_dict()
    ref = g.group("sd/QLSTM/")
    assert list(sd) == list(ref)
    for k, v in ref.items():
        assert torch.allclose(sd[k], v, rtol=1e-5, atol=1e-6), k


def _opts(**kw):
    o = {"lstm_lay": "16,8", "lstm_drop": "0.2,0.0", "lstm_act": "tanh,relu", "lstm_bidir": "True", "autograd": "False",
         "quaternion_init": "quaternion", "use_cuda": "True", "to_do": "train"}
    o.update(kw)
    return o


def test_refusals_at_construction():
    with pytest.raises(_lib.PkError):
        nn_amd.QLSTM(_opts(lstm_lay="18,8"), 12)
    with pytest.raises(_lib.PkError):
        nn_amd.QLSTM(_opts(lstm_lay="16,18"), 12)
    with pytest.raises(_lib.PkError):
        nn_amd.QLSTM(_opts(), 10)
    with pytest.raises(_lib.PkError):
        nn_amd.QLSTM(_opts(lstm_act="tanh,prelu"), 12)
    with pytest.raises(_lib.PkError):
        nn_amd.QLSTM(_opts(lstm_act="hardtanh,tanh"), 12)
    nn_amd.QLSTM(_opts(), 12)  # (and the options themselves are fine)
    del_q = _opts()
    del del_q["quaternion_init"]
    nn_amd.QLSTM(del_q, 12)  # quaternion_init is optional, and ignored when present


def test_autograd_option_changes_nothing():
    np.random.seed(5)
    a = nn_amd.QLSTM(_opts(autograd="False"), 12)
    np.random.seed(5)
    b = nn_amd.QLSTM(_opts(autograd="True"), 12)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_cpu_tensor_is_refused():
    net = nn_amd.QLSTM(_opts(), 12)
    with pytest.raises(_lib.PkError):
        net(torch.randn(5, 2, 12))
    comps = [torch.randn(3, 5) for _ in range(4)]
    with pytest.raises(_lib.PkError):
        F_amd.QuatMatrixFn.apply(*comps, 1, 3, 5)


def test_flat_groups_name_every_parameter_once_and_pack_the_components():
    net = nn_amd.QLSTM(_opts(lstm_lay="16,8,12", lstm_drop="0.2,0.0,0.1", lstm_act="tanh,relu,tanh"), 12)
    groups = net.pk_flat_groups()
    named = [id(q) for grp in groups for q in grp]
    assert sorted(named) == sorted(id(p) for p in net.parameters())
    assert len(named) == len(set(named))
    assert net.pk_unused_parameters() == []
    assert len(groups) == 3 * 3 and [len(grp) for grp in groups] == [16, 16, 4] * 3
    flat = optim_amd.FlatParams(net)
    assert flat.n_active == flat.numel  # nothing parked behind the active range
    for i in range(3):
        ws, us, bs = groups[3 * i:3 * i + 3]
        for grp in (ws, us):
            view = F_amd.adjacent_view([q.detach() for q in grp])
            assert view is not None, i  # one contiguous block: pk_quat_assemble's base-pointer form
            I, O = grp[0].shape
            assert tuple(view.shape) == (16 * I, O)
            assert F_amd.adjacent_view([q.grad for q in grp]) is not None
        # gate order f, i, o, c and r, i, j, k inside a gate - the order forward hands the components over in
        want = [getattr(getattr(net, m)[i], c) for m in ("wfx", "wix", "wox", "wcx")
                for c in ("r_weight", "i_weight", "j_weight", "k_weight")]
        assert [id(q) for q in ws] == [id(q) for q in want]
        assert [id(q) for q in ws] == [id(q) for q in net._layer_params(i)[0]]
        assert [id(q) for q in us] == [id(q) for q in net._layer_params(i)[1]]
        assert [id(q) for q in bs] == [id(getattr(net, m)[i].bias) for m in ("wfx", "wix", "wox", "wcx")]
    # the parameters are views of the flat buffer now, values kept
    assert all(getattr(p, "_pk_flat", False) for p in net.parameters())


def test_abi_declares_and_binds_both_entries():
    names = _lib.declared_symbols()
    for n in ("pk_quat_assemble", "pk_quat_fold"):
        assert n in names and n in _lib.SIGNATURES
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert re.search(r"int\s+pk_quat_assemble\s*\(\s*void\s*\*\s*stream", text)
    assert re.search(r"int\s+pk_quat_fold\s*\(\s*void\s*\*\s*stream", text)
    assert len(_lib.SIGNATURES["pk_quat_assemble"][1]) == 7 and len(_lib.SIGNATURES["pk_quat_fold"][1]) == 8
    lib = _lib.load()
    assert hasattr(lib, "pk_quat_assemble") and hasattr(lib, "pk_quat_fold")


def test_bad_arguments_return_an_error_before_any_device_call():
    lib = _lib.load()
    fake = 4096  # never dereferenced: the checks come first
    assert lib.pk_quat_assemble(None, None, None, 1, 2, 2, fake) != 0 and b"pk_quat_assemble" in lib.pk_last_error()
    assert lib.pk_quat_assemble(None, None, fake, 1, 2, 2, None) != 0
    assert lib.pk_quat_assemble(None, None, fake, 1, 0, 2, fake) != 0
    assert lib.pk_quat_assemble(None, None, fake, 0, 2, 2, fake) != 0
    assert lib.pk_quat_fold(None, None, 1, 2, 2, 0.0, None, fake) != 0
    assert lib.pk_quat_fold(None, fake, 1, 2, 2, 0.0, None, None) != 0
    assert lib.pk_quat_fold(None, fake, 1, 2, 0, 0.0, None, fake) != 0
    assert lib.pk_quat_fold(None, fake, 1, 2, 2, 0.5, None, fake) != 0 and b"beta" in lib.pk_last_error()
