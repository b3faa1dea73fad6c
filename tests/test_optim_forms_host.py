"""optim.FusedOptimizer in the forms torch.optim.RMSprop / SGD accept beyond the plain ones (RMSprop momentum / centered,
SGD dampening / nesterov): everything that happens on the host - which forms are accepted, which flat state buffers they
keep, and torch's own state_dict format both ways.  The kernels themselves: test_gpu_optim_forms.py."""
import importlib

import pytest
import torch

OPT = importlib.import_module("pytorch-kaldi_amd.optim")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

FORMS = [("rmsprop", dict(alpha=0.95, eps=1e-8, momentum=0.9), ("square_avg", "momentum_buffer")),
         ("rmsprop", dict(alpha=0.95, eps=1e-8, centered=True), ("square_avg", "grad_avg")),
         ("rmsprop", dict(alpha=0.95, eps=1e-8, momentum=0.9, centered=True, weight_decay=1e-4),
          ("square_avg", "momentum_buffer", "grad_avg")),
         ("sgd", dict(momentum=0.9, nesterov=True, weight_decay=1e-4), ("momentum_buffer",)),
         ("sgd", dict(momentum=0.9, dampening=0.3), ("momentum_buffer",)),
         ("sgd", dict(momentum=0.0, dampening=0.3), ())]
TORCH = {"rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5))


@pytest.mark.parametrize("kind,kw,keys", FORMS)
def test_new_forms_construct_and_write_torchs_param_groups(kind, kw, keys):
    net = _net()
    opt = OPT.FusedOptimizer(OPT.FlatParams(net), kind, 0.01, **kw)
    assert tuple(opt.bufs) == keys
    for b in opt.bufs.values():
        assert b.shape == opt.flat.flat.shape and float(b.abs().max()) == 0.0
    sd = opt.state_dict()
    ref = TORCH[kind](list(_net().parameters()), lr=0.01, **kw).state_dict()
    assert sd["param_groups"] == ref["param_groups"]
    for k in ("momentum", "centered") if kind == "rmsprop" else ("momentum", "dampening", "nesterov"):
        assert sd["param_groups"][0][k] == kw.get(k, ref["param_groups"][0][k])
    assert sd["state"] == {} == ref["state"]
    with pytest.raises(_lib.PkError):  # no CPU fallback for the new forms either
        opt.step()


@pytest.mark.parametrize("kw", [dict(momentum=0.0, nesterov=True), dict(momentum=0.9, dampening=0.1, nesterov=True)])
def test_nesterov_needs_a_momentum_and_zero_dampening_like_torch(kw):
    with pytest.raises(ValueError):
        torch.optim.SGD(list(_net().parameters()), lr=0.01, **kw)
    with pytest.raises(Exception, match="Nesterov momentum requires a momentum and zero dampening"):
        OPT.FusedOptimizer(OPT.FlatParams(_net()), "sgd", 0.01, **kw)


def test_load_state_dict_adopts_the_form_of_a_torch_checkpoint():
    """A torch RMSprop(momentum, centered) state loaded into an optimizer built plain: the optimizer takes the form, with
    every buffer of it at torch's values; and a plain state loaded back releases the two buffers again."""
    ref = _net()
    topt = torch.optim.RMSprop(list(ref.parameters()), lr=4e-4, alpha=0.95, eps=1e-8, momentum=0.9, centered=True)
    x = torch.randn(64, 33, generator=torch.Generator().manual_seed(1))
    for _ in range(2):
        topt.zero_grad()
        ref(x).pow(2).mean().backward()
        topt.step()
    opt = OPT.FusedOptimizer(OPT.FlatParams(_net()), "rmsprop", 0.01)
    assert tuple(opt.bufs) == ("square_avg",)
    opt.load_state_dict(topt.state_dict())
    assert opt.momentum == 0.9 and opt.centered is True and opt.alpha == 0.95 and opt.param_groups[0]["lr"] == 4e-4
    assert sorted(opt.bufs) == ["grad_avg", "momentum_buffer", "square_avg"] and opt.steps == 2
    for i, (p, o) in enumerate(zip(opt.flat.params, opt.flat.offsets)):
        for k in ("square_avg", "momentum_buffer", "grad_avg"):
            assert torch.equal(opt.bufs[k][o:o + p.numel()].view(p.shape), topt.state[topt.param_groups[0]["params"][i]][k]), (i, k)
    sd = opt.state_dict()
    assert sd["param_groups"] == topt.state_dict()["param_groups"]
    assert sorted(sd["state"]) == sorted(topt.state_dict()["state"])
    assert set(sd["state"][0]) == set(topt.state_dict()["state"][0])
    # entries without the keys of the loaded form: zeros, torch's initial value of all three buffers
    plain = torch.optim.RMSprop(list(ref.parameters()), lr=4e-4).state_dict()
    mixed = {"state": {i: {"step": e["step"], "square_avg": e["square_avg"]} for i, e in sd["state"].items()},
             "param_groups": sd["param_groups"]}
    opt.load_state_dict(mixed)
    assert float(opt.bufs["momentum_buffer"].abs().max()) == 0.0 and float(opt.bufs["grad_avg"].abs().max()) == 0.0
    assert float(opt.bufs["square_avg"].abs().max()) > 0.0 and opt.steps == 2
    opt.load_state_dict(plain)
    assert tuple(opt.bufs) == ("square_avg",) and opt.momentum == 0.0 and opt.centered is False and opt.steps == 0


def test_load_state_dict_rechecks_the_nesterov_rule():
    net = _net()
    opt = OPT.FusedOptimizer(OPT.FlatParams(net), "sgd", 0.1, momentum=0.9, nesterov=True)
    sd = opt.state_dict()
    sd["param_groups"][0]["dampening"] = 0.2
    with pytest.raises(Exception, match="Nesterov"):
        opt.load_state_dict(sd)
