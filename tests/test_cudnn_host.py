"""LSTM_cudnn / RNN_cudnn / GRU_cudnn without a GPU: parameter names, order, shapes and initial values against
torch.nn.LSTM / nn.RNN built and re-initialised the way the reference's classes do it (neural_networks.py:153-297; only
torch is needed), checkpoints of the reference fixtures, refusals, the flat-parameter layout and the C ABI's argument
checks (which come before any device call)."""
import importlib
import itertools
import re

import pytest
import torch

from golden_util import Golden

nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_amd = importlib.import_module("pytorch-kaldi_amd.functional")
optim_amd = importlib.import_module("pytorch-kaldi_amd.optim")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

ENTRIES = ("pk_gates_pack", "pk_gates_unpack", "pk_seq_join_fwd", "pk_seq_join_bwd")


def _opts(**kw):
    o = {"hidden_size": "8", "num_layers": "2", "bias": "True", "batch_first": "True", "dropout": "0.0", "bidirectional": "True",
         "nonlinearity": "tanh", "use_cuda": "True", "to_do": "train"}
    o.update({k: str(v) for k, v in kw.items()})
    return o


def _reference_way(cls, D, H, L, bias, batch_first, bidir, nonlinearity):
    """What the reference's constructor leaves behind, from torch alone."""
    if cls == "LSTM_cudnn":
        m = torch.nn.LSTM(D, H, L, bias=bias, dropout=0.0, bidirectional=bidir)
        for name, param in m.named_parameters():
            if "weight_hh" in name:
                if batch_first:
                    torch.nn.init.orthogonal_(param)
            elif "bias" in name:
                torch.nn.init.zeros_(param)
        return m
    return torch.nn.RNN(D, H, L, nonlinearity=nonlinearity, bias=bias, dropout=0.0, bidirectional=bidir)


@pytest.mark.parametrize("cls,pre", [("LSTM_cudnn", "lstm.0."), ("RNN_cudnn", "rnn.0.")])
@pytest.mark.parametrize("bidir,bias,batch_first", list(itertools.product([False, True], repeat=3)))
@pytest.mark.parametrize("L", [1, 3])
def test_same_seed_same_state_dict_as_torch(cls, pre, bidir, bias, batch_first, L):
    D, H, seed = 6, 8, 17 + L
    torch.manual_seed(seed)
    net = getattr(nn_amd, cls)(_opts(num_layers=L, bias=bias, batch_first=batch_first, bidirectional=bidir,
                                     nonlinearity="relu"), D)
    torch.manual_seed(seed)
    ref = _reference_way(cls, D, H, L, bias, batch_first, bidir, "relu")
    sd, rsd = net.state_dict(), ref.state_dict()
    assert list(sd) == [pre + k for k in rsd]
    assert [k for k, _ in net.named_parameters()] == [pre + k for k, _ in ref.named_parameters()]
    for k, v in rsd.items():
        assert sd[pre + k].shape == v.shape and torch.equal(sd[pre + k], v), k
    assert net.out_dim == (2 * H if bidir else H)
    assert ("bias_ih_l0" in "".join(sd)) == bias
    # and the other way round: the reference's module takes this one's checkpoint
    res = ref.load_state_dict({k[len(pre):]: v for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


@pytest.mark.parametrize("case", ["e2e_lstm_cudnn_bidir_train", "e2e_lstm_cudnn_uni_eval", "e2e_rnn_cudnn_tanh_bidir_train",
                                  "e2e_rnn_cudnn_relu_uni_train"])
def test_reference_checkpoints_load_strictly(case):
    g = Golden(case)
    net = getattr(nn_amd, g.meta["arch_class"])(dict(g.meta["options"], use_cuda="True"), g.meta["inp_dim"])
    sd = g.group("sd/")
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(net.state_dict()) == list(sd)
    assert net.out_dim == g.meta["out_dim"]
    # the same seed gives the reference's initial values
    torch.manual_seed(g.meta["seed"])
    fresh = getattr(nn_amd, g.meta["arch_class"])(dict(g.meta["options"], use_cuda="True"), g.meta["inp_dim"])
    for k, v in g.group("init/").items():
        assert torch.equal(fresh.state_dict()[k], v), k
    if case == "e2e_rnn_cudnn_relu_uni_train":
        assert g.meta["min_abs_preactivation"] >= 1e-3


def test_gru_cudnn_is_refused_with_the_reason():
    with pytest.raises(_lib.PkError) as e:
        nn_amd.GRU_cudnn(_opts(), 6)
    msg = str(e.value)
    assert "r * (U_n h + b_hn)" in msg and "GRU" in msg and "cell" in msg


def test_refusals_at_construction():
    for cls in ("LSTM_cudnn", "RNN_cudnn"):
        with pytest.raises(_lib.PkError):
            getattr(nn_amd, cls)(_opts(dropout="1.0"), 6)
        with pytest.raises(_lib.PkError):
            getattr(nn_amd, cls)(_opts(dropout="1.5"), 6)
        getattr(nn_amd, cls)(_opts(dropout="0.99"), 6)
    with pytest.raises(_lib.PkError):
        nn_amd.RNN_cudnn(_opts(nonlinearity="sigmoid"), 6)
    assert nn_amd.RNN_cudnn(_opts(nonlinearity="relu"), 6).nonlinearity == "relu"


@pytest.mark.parametrize("cls", ["LSTM_cudnn", "RNN_cudnn"])
def test_cpu_tensor_is_refused(cls):
    net = getattr(nn_amd, cls)(_opts(), 6)
    with pytest.raises(_lib.PkError):
        net(torch.randn(5, 2, 6))
    with pytest.raises(_lib.PkError):
        F_amd.gates_pack(torch.randn(32, 6), torch.randn(32, 8), None, None, F_amd.GATE_PERM["LSTM"])
    with pytest.raises(_lib.PkError):
        F_amd.seq_join(torch.randn(3, 2, 4), torch.randn(3, 2, 4))


@pytest.mark.parametrize("cls", ["LSTM_cudnn", "RNN_cudnn"])
@pytest.mark.parametrize("bidir,bias", [(True, True), (False, True), (True, False)])
def test_flat_groups_cover_every_parameter_once(cls, bidir, bias):
    net = getattr(nn_amd, cls)(_opts(num_layers=3, bidirectional=bidir, bias=bias), 6)
    groups = net.pk_flat_groups()
    named = [id(q) for grp in groups for q in grp]
    assert sorted(named) == sorted(id(p) for p in net.parameters())
    assert len(named) == len(set(named))
    assert net.pk_unused_parameters() == []
    ndir = 2 if bidir else 1
    assert [len(grp) for grp in groups] == [1, 1, 2 if bias else 0] * (3 * ndir)
    params = dict(net.named_parameters())
    pre = "lstm.0." if cls == "LSTM_cudnn" else "rnn.0."
    at = 0
    for k in range(3):
        for sfx in ("", "_reverse")[:ndir]:
            want = [[params[pre + "weight_ih_l%d%s" % (k, sfx)]], [params[pre + "weight_hh_l%d%s" % (k, sfx)]],
                    [params[pre + "%s_l%d%s" % (n, k, sfx)] for n in ("bias_ih", "bias_hh")] if bias else []]
            assert [[id(q) for q in grp] for grp in groups[at:at + 3]] == [[id(q) for q in grp] for grp in want]
            at += 3


def test_flat_params_put_the_two_biases_back_to_back():
    torch.manual_seed(1)
    net = nn_amd.LSTM_cudnn(_opts(num_layers=2), 6)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    flat = optim_amd.FlatParams(net)
    assert flat.n_active == flat.numel
    assert all(getattr(p, "_pk_flat", False) for p in net.parameters())
    for grp in net.pk_flat_groups()[2::3]:
        view = F_amd.adjacent_view([q.detach() for q in grp])
        assert view is not None and tuple(view.shape) == (2 * 4 * 8,)
        assert F_amd.adjacent_view([q.grad for q in grp]) is not None
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_abi_declares_and_binds_the_entries():
    names = _lib.declared_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    lib = _lib.load()
    for n in ENTRIES:
        assert n in names and n in _lib.SIGNATURES
        assert re.search(r"int\s+%s\s*\(\s*void\s*\*\s*stream" % n, text)
        assert hasattr(lib, n)
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [12, 12, 11, 11]


def test_bad_arguments_return_an_error_before_any_device_call():
    lib = _lib.load()
    fake = 4096  # never dereferenced: the checks come first
    perm = F_amd._perm_arg((1, 0, 3, 2))
    bad = F_amd._perm_arg((1, 1, 3, 2))
    assert lib.pk_gates_pack(None, fake, fake, None, None, 4, -1, 4, perm, fake, fake, None) != 0
    assert b"pk_gates_pack" in lib.pk_last_error()
    assert lib.pk_gates_pack(None, fake, fake, None, None, 4, 4, 0, perm, fake, fake, None) != 0
    assert lib.pk_gates_pack(None, fake, fake, None, None, 0, 4, 4, perm, fake, fake, None) != 0
    assert lib.pk_gates_pack(None, fake, fake, None, None, 9, 4, 4, perm, fake, fake, None) != 0
    assert lib.pk_gates_pack(None, fake, fake, None, None, 4, 4, 4, bad, fake, fake, None) != 0   # not a permutation
    assert lib.pk_gates_pack(None, fake, fake, None, None, 4, 4, 4, None, fake, fake, None) != 0
    assert lib.pk_gates_pack(None, fake, fake, None, None, 4, 4, 4, perm, None, fake, None) != 0   # a matrix without its target
    assert lib.pk_gates_pack(None, None, None, None, None, 4, 4, 4, perm, None, None, fake) != 0   # nothing to move
    assert lib.pk_gates_unpack(None, fake, fake, None, 4, 4, -3, perm, fake, fake, None, None) != 0
    assert b"pk_gates_unpack" in lib.pk_last_error()
    assert lib.pk_gates_unpack(None, fake, None, None, 4, 4, 4, perm, fake, fake, None, None) != 0
    assert lib.pk_seq_join_fwd(None, fake, None, None, 1.0, -1, 2, 4, 1, fake, None) != 0
    assert b"pk_seq_join_fwd" in lib.pk_last_error()
    assert lib.pk_seq_join_fwd(None, fake, None, None, 1.0, 3, 2, 4, 1, None, None) != 0   # both outputs NULL
    assert lib.pk_seq_join_fwd(None, fake, None, None, 1.0, 3, 2, 4, 2, fake, None) != 0   # two directions, one tensor
    assert lib.pk_seq_join_fwd(None, fake, fake, None, 1.0, 3, 2, 4, 1, fake, None) != 0
    assert lib.pk_seq_join_fwd(None, None, None, None, 1.0, 3, 2, 4, 1, fake, None) != 0
    assert lib.pk_seq_join_fwd(None, fake, None, None, 1.0, 3, 2, 4, 3, fake, None) != 0
    assert lib.pk_seq_join_bwd(None, None, None, None, 1.0, 3, 2, 4, 1, fake, None) != 0   # both gradients NULL
    assert b"pk_seq_join_bwd" in lib.pk_last_error()
    assert lib.pk_seq_join_bwd(None, fake, None, None, 1.0, 3, 0, 4, 1, fake, None) != 0
    assert lib.pk_seq_join_bwd(None, fake, None, None, 1.0, 3, 2, 4, 2, fake, None) != 0
