"""The fused optimizer forms behind pk_fused_step_ex - RMSprop with momentum / centered, SGD with dampening / nesterov -
against torch.optim on the GPU: the kernels through the C ABI, FusedOptimizer on a real module, checkpoints both ways,
HIP-graph replay and the recipe path.  (Host-side behaviour: test_optim_forms_host.py.)

Tolerances: 1e-6 norm-relative at the C ABI is the bound the project holds its other optimizer kernels to; a plain fp32
evaluation of the same formulas is 1e-9 .. 6e-9 from torch.optim on the parameters and at most 8e-8 on the state for the
inputs used here, so FMA contraction and evaluation order have more than 10x room.  Gradients are independent draws per
step: that keeps sq - ga^2 of the centered form far from cancellation, the one regime where torch itself turns to NaN."""
import ctypes
import importlib

import pytest
import torch

from golden_util import rel_err

pytestmark = pytest.mark.gpu
_lib = importlib.import_module("pytorch-kaldi_amd._lib")
OPT = importlib.import_module("pytorch-kaldi_amd.optim")
CENTERED, NESTEROV = 1, 2

# (kind, torch arguments, state keys in the order of the entry's s0, s1, s2)
ABI_FORMS = [
    (0, dict(lr=4e-4, alpha=0.95, eps=1e-8, momentum=0.9), ("square_avg", "momentum_buffer", None)),
    (0, dict(lr=4e-4, alpha=0.95, eps=1e-8, centered=True), ("square_avg", None, "grad_avg")),
    (0, dict(lr=4e-4, alpha=0.95, eps=1e-8, momentum=0.9, centered=True, weight_decay=1e-4),
     ("square_avg", "momentum_buffer", "grad_avg")),
    (1, dict(lr=0.08, momentum=0.9, nesterov=True, weight_decay=1e-4), ("momentum_buffer", None, None)),
    (1, dict(lr=0.08, momentum=0.9, dampening=0.3), ("momentum_buffer", None, None)),
    (1, dict(lr=0.08, momentum=0.0, dampening=0.3), (None, None, None)),
]


def _ids(forms):
    return ["-".join([["rmsprop", "sgd"][f[0]] if isinstance(f[0], int) else f[0]] +
                     ["%s=%s" % kv for kv in f[1].items() if kv[0] not in ("lr", "alpha", "eps")]) for f in forms]


def _ex_step(lib, kind, kw, pe, ge, bufs, keys, step, zero, segs=None, nseg=0, shadow=None):
    h = (kw["alpha"], kw["eps"], kw.get("momentum", 0.0)) if kind == 0 else (kw["momentum"], kw.get("dampening", 0.0), 0.0)
    flags = (CENTERED if kw.get("centered") else 0) | (NESTEROV if kw.get("nesterov") else 0)
    s = [bufs[k].data_ptr() if k else None for k in keys]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.pk_fused_step_ex(st, kind, pe.data_ptr(), ge.data_ptr(), s[0], s[1], s[2], pe.numel(), kw["lr"], h[0], h[1],
                                    h[2], kw.get("weight_decay", 0.0), flags, step, int(zero),
                                    segs.data_ptr() if nseg else None, nseg, shadow.data_ptr() if nseg else None), "fused step ex")


def _check_against_torch(pe, bufs, pr, opt):
    err = rel_err(pe, pr)
    print("rel_err p %.3e" % err)
    assert err < 1e-6, err
    for k, b in bufs.items():
        err = rel_err(b, opt.state[pr][k])
        print("rel_err %s %.3e" % (k, err))
        assert err < 1e-6, (k, err)


@pytest.mark.parametrize("kind,kw,keys", ABI_FORMS, ids=_ids(ABI_FORMS))
def test_fused_step_ex_matches_torch_zeroes_the_gradient_and_refreshes_the_bf16_copies(kind, kw, keys):
    lib = _lib.load()
    g = torch.Generator().manual_seed(14)
    n = 64 * 300
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(5)]
    # two "weights" inside the bucket: [40 x 100] at element 128 (pitch 128) and [7 x 64] at element 6400 (pitch 64)
    segs = torch.tensor([[128, 40, 100, 128, 0], [6400, 7, 64, 64, 40 * 128]], dtype=torch.int64).cuda()
    pr = p0.clone().requires_grad_(True)
    opt = (torch.optim.RMSprop if kind == 0 else torch.optim.SGD)([pr], **kw)
    pe = p0.clone().cuda()
    bufs = {k: torch.zeros(n).cuda() for k in keys if k}
    shadow = torch.zeros(40 * 128 + 7 * 64 + 64, dtype=torch.bfloat16).cuda()
    shadow[-64:] = 3.0
    for i, gr in enumerate(grads):
        pr.grad = gr.clone()
        opt.step()
        ge = gr.cuda()
        _ex_step(lib, kind, kw, pe, ge, bufs, keys, i + 1, i != 1, segs, 2, shadow)
        torch.cuda.synchronize()
        assert float(ge.abs().max()) == 0.0 if i != 1 else torch.equal(ge.cpu(), gr)
    _check_against_torch(pe, bufs, pr, opt)
    w1 = pe[128:128 + 4000].view(40, 100)
    c1 = shadow[:40 * 128].view(40, 128)
    assert torch.equal(c1[:, :100], w1.to(torch.bfloat16)) and float(c1[:, 100:].float().abs().max()) == 0.0
    w2 = pe[6400:6400 + 448].view(7, 64)
    assert torch.equal(shadow[40 * 128:40 * 128 + 448].view(7, 64), w2.to(torch.bfloat16))
    assert float((shadow[-64:].float() - 3.0).abs().max()) == 0.0


def test_fused_step_ex_grid_stride_loop():
    """More quads than the grid has threads (4096 blocks of 256), and not a multiple of them: the loop's second trip."""
    lib = _lib.load()
    kind, kw, keys = ABI_FORMS[2]
    g = torch.Generator().manual_seed(15)
    n = 4 * (4096 * 256 + 3)
    p0 = torch.randn(n, generator=g)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.RMSprop([pr], **kw)
    pe = p0.clone().cuda()
    bufs = {k: torch.zeros(n).cuda() for k in keys}
    for i in range(2):
        gr = torch.randn(n, generator=g)
        pr.grad = gr.clone()
        opt.step()
        ge = gr.cuda()
        _ex_step(lib, kind, kw, pe, ge, bufs, keys, i + 1, i == 0)
        torch.cuda.synchronize()
        assert float(ge.abs().max()) == 0.0 if i == 0 else torch.equal(ge.cpu(), gr)
    _check_against_torch(pe, bufs, pr, opt)


def test_fused_step_ex_refuses_what_it_cannot_run():
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, g, s = (torch.zeros(64).cuda() for _ in range(3))

    def call(kind, s0, s1, s2, h0, h1, h2, flags, n=64, step=1):
        return lib.pk_fused_step_ex(st, kind, p.data_ptr(), g.data_ptr(), s0, s1, s2, n, 0.1, h0, h1, h2, 0.0, flags, step, 0,
                                    None, 0, None)

    sp = s.data_ptr()
    assert call(0, sp, None, None, 0.95, 1e-8, 0.9, 0) != 0 and b"buffer" in lib.pk_last_error()         # momentum, no buffer
    assert call(0, sp, None, None, 0.95, 1e-8, 0.0, CENTERED) != 0 and b"average" in lib.pk_last_error()  # centered, no grad_avg
    assert call(0, None, None, None, 0.95, 1e-8, 0.0, 0) != 0
    assert call(1, None, None, None, 0.9, 0.0, 0.0, 0) != 0 and b"buffer" in lib.pk_last_error()
    assert call(1, sp, None, None, 0.0, 0.0, 0.0, NESTEROV) != 0 and b"Nesterov" in lib.pk_last_error()
    assert call(1, sp, None, None, 0.9, 0.1, 0.0, NESTEROV) != 0 and b"Nesterov" in lib.pk_last_error()
    assert call(2, sp, sp, None, 0.9, 0.999, 1e-8, 0) != 0                                                # Adam stays with pk_fused_step
    assert call(1, sp, None, None, 0.9, 0.0, 0.0, 0, n=62) != 0 and call(1, sp, None, None, 0.9, 0.0, 0.0, 0, step=0) != 0
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0


# ---- FusedOptimizer on a real module ---------------------------------------------------------------------------------
MODULE_FORMS = [("rmsprop", dict(momentum=0.9, centered=True, weight_decay=0.05)),
                ("sgd", dict(momentum=0.9, nesterov=True, weight_decay=0.05))]


@pytest.mark.parametrize("kind,kw", MODULE_FORMS, ids=_ids(MODULE_FORMS))
def test_fused_optimizer_new_forms_skip_never_used_parameters_like_torch(kind, kw):
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    opts = {"ligru_lay": "24,16", "ligru_drop": "0.0,0.0", "ligru_use_laynorm_inp": "False", "ligru_use_batchnorm_inp": "False",
            "ligru_use_laynorm": "False,True", "ligru_use_batchnorm": "True,False", "ligru_bidir": "True",
            "ligru_act": "relu,relu", "ligru_orthinit": "True", "use_cuda": "True", "to_do": "train"}
    torch.manual_seed(3)
    net_e = nn_amd.liGRU(dict(opts), 9).cuda().train()
    net_t = nn_amd.liGRU(dict(opts), 9).cuda().train()
    net_t.load_state_dict(net_e.state_dict())
    x = torch.randn(7, 3, 9, generator=torch.Generator().manual_seed(1)).cuda()
    lr = 0.01
    opt_t = {"rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}[kind](net_t.parameters(), lr=lr, **kw)
    opt_e = OPT.FusedOptimizer(OPT.FlatParams(net_e), kind, lr, **kw)
    unused = {n for n, p in net_e.named_parameters() if any(p is q for q in net_e.pk_unused_parameters())}
    assert len(unused) == 6
    before = {n: p.detach().clone() for n, p in net_e.named_parameters()}
    for _ in range(3):
        for net, opt in ((net_t, opt_t), (net_e, opt_e)):
            opt.zero_grad()
            net(x).square().mean().backward()
            opt.step()
    torch.cuda.synchronize()
    for (n, pe), (_, pt) in zip(net_e.named_parameters(), net_t.named_parameters()):
        if n in unused:
            assert pt.grad is None and torch.equal(pe, before[n]) and torch.equal(pt, before[n]), n
        else:
            assert rel_err(pe, pt) < 1e-5, (n, rel_err(pe, pt))
    sd_e, sd_t = opt_e.state_dict(), opt_t.state_dict()
    assert sorted(sd_e["state"]) == sorted(sd_t["state"])
    k = sorted(sd_t["state"])[0]
    assert set(sd_e["state"][k]) == set(sd_t["state"][k])
    assert sd_e["param_groups"] == sd_t["param_groups"]


CKPT_FORMS = [("rmsprop", dict(lr=4e-4, alpha=0.95, eps=1e-8, momentum=0.9, centered=True)),
              ("sgd", dict(lr=0.08, momentum=0.9, dampening=0.3)),
              ("sgd", dict(lr=0.08, momentum=0.9, nesterov=True))]


@pytest.mark.parametrize("kind,kw", CKPT_FORMS, ids=_ids(CKPT_FORMS))
def test_fused_optimizer_new_forms_continue_a_torch_checkpoint(kind, kw):
    mk = lambda ps: {"rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}[kind](ps, **kw)
    torch.manual_seed(3)
    ref = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5)).cuda()
    eng = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5)).cuda()
    x = torch.randn(64, 33).cuda()
    ropt = mk(list(ref.parameters()))

    def rstep(net, opt):
        opt.zero_grad()
        net(x).pow(2).mean().backward()
        opt.step()

    for _ in range(2):
        rstep(ref, ropt)
    eng.load_state_dict(ref.state_dict())
    fkw = {k: v for k, v in kw.items() if k != "lr"}
    fopt = OPT.FusedOptimizer(OPT.FlatParams(eng), kind, kw["lr"], **fkw)
    fopt.load_state_dict(ropt.state_dict())
    for _ in range(2):
        rstep(ref, ropt)
        rstep(eng, fopt)
    for a, b in zip(eng.parameters(), ref.parameters()):
        assert rel_err(a, b) < 1e-5, rel_err(a, b)
    # and back: torch continues from the fused optimizer's state
    back = mk(list(ref.parameters()))
    back.load_state_dict(fopt.state_dict())
    rstep(ref, back)
    rstep(eng, fopt)
    for a, b in zip(eng.parameters(), ref.parameters()):
        assert rel_err(a, b) < 1e-5, rel_err(a, b)


GRAPH_FORMS = [("rmsprop", dict(alpha=0.95, eps=1e-8, momentum=0.9, centered=True)), ("sgd", dict(momentum=0.9, nesterov=True))]


@pytest.mark.parametrize("kind,kw", GRAPH_FORMS, ids=_ids(GRAPH_FORMS))
def test_hip_graph_replay_of_the_new_forms_trains_like_eager_steps(kind, kw):
    """bf16 mode: the replayed forward reads the weight copies the captured step refreshes, so a form that skipped the
    refresh (or the gradient zeroing zero_in_step promises) ends elsewhere than the eager loop."""
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
            opt = OPT.FusedOptimizer(OPT.FlatParams(net), kind, 1e-3, **kw)
            opt.zero_in_step = True

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
            results.append((opt.flat.flat.clone(), {k: b.clone() for k, b in opt.bufs.items()}, opt.steps, torch.stack(losses)))
        (p0, s0, n0, l0), (p1, s1, n1, l1) = results
        assert n0 == n1 == 7
        assert torch.equal(l0, l1) and torch.equal(p0, p1)
        assert sorted(s0) == sorted(s1) == sorted(opt._state_keys())
        for k in s0:
            assert torch.equal(s0[k], s1[k]) and float(s0[k].abs().max()) > 0.0, k
    finally:
        F_.set_precision(old)


def test_recipe_fields_reach_the_fused_optimizer():
    recipes = importlib.import_module("pytorch-kaldi_amd.recipes")
    utils = importlib.import_module("pytorch-kaldi_amd.utils")
    sec = dict(recipes._rms("0.002"), opt_momentum="0.9", opt_centered="True")
    torch.manual_seed(5)
    ref = torch.nn.Sequential(torch.nn.Linear(20, 12), torch.nn.ReLU(), torch.nn.Linear(12, 4)).cuda()
    eng = torch.nn.Sequential(torch.nn.Linear(20, 12), torch.nn.ReLU(), torch.nn.Linear(12, 4)).cuda()
    eng.load_state_dict(ref.state_dict())
    config, arch = {"architecture1": sec}, {"net": ["architecture1"]}
    topt = utils.optimizer_init({"net": ref}, config, arch)["net"]
    fopt = OPT.fused_optimizer_init({"net": eng}, config, arch)["net"]
    assert isinstance(fopt, OPT.FusedOptimizer) and fopt.momentum == 0.9 and fopt.centered is True
    assert sorted(fopt.bufs) == ["grad_avg", "momentum_buffer", "square_avg"]
    x = torch.randn(16, 20, generator=torch.Generator().manual_seed(2)).cuda()
    for net, opt in ((ref, topt), (eng, fopt)):
        opt.zero_grad()
        net(x).pow(2).mean().backward()
        opt.step()
    torch.cuda.synchronize()
    assert fopt.steps == 1
    for a, b in zip(eng.parameters(), ref.parameters()):
        assert rel_err(a, b) < 1e-5, rel_err(a, b)
    bad = dict(recipes._sgd(), opt_nesterov="True", opt_momentum="0.0")
    with pytest.raises(Exception, match="Nesterov"):
        OPT.fused_optimizer_init({"net": eng}, {"architecture1": bad}, arch)
