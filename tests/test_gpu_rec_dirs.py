"""Both directions of a torch-layout layer in one recurrence launch (pk_rec_persist2_dirs.hip; LSTM_cudnn / RNN_cudnn).

Kernel level: pk_rec_fwd_bf16_dirs / pk_rec_bwd_bf16_dirs with two different weight sets against two calls of
pk_rec_fwd_bf16 / pk_rec_bwd_bf16 at bidir = 0 (direction 1 on time-reversed P and dY), placed into the bidirectional
layouts on the host: torch.equal on Y, S, dP2 and the valid columns of Yb and dGb - per-row arithmetic is the same, only
the split into clusters differs.  Against an fp64 loop with U and the exchanged h rounded to bf16 the bound is 1e-2, the
figure tests/test_gpu_kernels.py uses for every bf16-operand comparison.  Class level: the new path against the same module
under PK_EXPERIMENT cudnn_dirs=0: y and dx bit-equal; the parameter gradients of the reversed direction sum their rows in
the opposite time order and take tests/test_gpu_cudnn.py's bf16 bound max(1e-5, 2 d0), d0 the run-to-run distance.

The plan gives direction d its own clusters: B = 3 runs 3 + 3 clusters of one row (2B = 6 rows would fit one tile), B = 16
4 + 4 of four rows, B = 17 3 + 3 of 6, 6, 5 rows."""
import importlib

import pytest
import torch

from golden_util import rel_err

pytestmark = pytest.mark.gpu
nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

CELLS = [("LSTM", "tanh"), ("RNN", "tanh"), ("RNN", "relu")]
SHAPES = [(H, B, T) for H in (8, 13, 80) for B in (3, 16, 17) for T in (1, 2, 7)]


@pytest.fixture(autouse=True)
def _bf16():
    F_.set_precision("bf16")
    F_.set_rec_algo("auto")
    yield
    F_.set_precision("fp32")


def test_the_entries_resolve():
    lib = _lib.load()
    for name in ("pk_rec_fwd_bf16_dirs", "pk_rec_bwd_bf16_dirs", "pk_rec_dirs_covered"):
        assert getattr(lib, name) is not None


def _inputs(cell, H, B, T):
    G = 4 if cell == "LSTM" else 1
    g = torch.Generator().manual_seed(1000 * H + 10 * B + T)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"P": r(2, T, B, G * H).cuda(), "psh": (0.1 * r(2, G * H)).cuda(), "U": (r(2, G * H, H) / H ** 0.5).cuda(),
            "dY": r(T, B, 2 * H).cuda(), "G": G}


def _launch(lib, entry, cell, act, T, B, bidir, H, P, psh, U, dY, save=True):
    """One forward and (save) one backward call of `entry` ("" or "_dirs"): Y, S, Yb, dP2, dGb, exchange buffers NaN-free
    only where written (they start as the 0xFF pattern)."""
    G, NS = lib.pk_rec_num_gates(F_.CELL[cell]), lib.pk_rec_num_saved(F_.CELL[cell])
    nd, Hp, p = 1 + bidir, F_._up(H, 8), F_._p
    yp, gp = F_._up(nd * Hp, 64), F_._up(G * Hp, 64)
    Y = torch.full((T, B, nd * H), float("nan"), device="cuda")
    S = torch.full((nd, T * B, NS * H), float("nan"), device="cuda") if save else None
    Yb = torch.empty(T * B, yp, device="cuda", dtype=torch.bfloat16)
    psc = torch.ones_like(psh)
    head = (F_._stream(), F_.CELL[cell], F_.ACT[act], T, B, bidir, H)
    _lib.check(getattr(lib, "pk_rec_fwd_bf16" + entry)(*head, p(P), p(psc), p(psh), p(U), None, 1.0, p(Y), p(S), p(Yb), yp, 2), "fwd")
    out = {"Y": Y, "S": S, "Yb": Yb}
    if save:
        dP2 = torch.full((nd, T * B, G * H), float("nan"), device="cuda")
        dGb = torch.empty(nd * T * B, gp, device="cuda", dtype=torch.bfloat16)
        _lib.check(getattr(lib, "pk_rec_bwd_bf16" + entry)(*head, p(U), None, 1.0, p(Y), p(S), p(dY.contiguous()), p(dP2), p(dGb), gp, 2),
                   "bwd")
        out.update(dP2=dP2, dGb=dGb)
    torch.cuda.synchronize()
    _lib.raise_if_persist_failed()
    return out


def _two_single_launches(lib, cell, act, H, B, T, x, save):
    """The parent's kernels, one direction per launch, in the bidirectional layouts."""
    rev = lambda t: t.view(T, B, -1).flip(0)
    f = _launch(lib, "", cell, act, T, B, 0, H, x["P"][0].contiguous(), x["psh"][0], x["U"][0], x["dY"][:, :, :H], save)
    b = _launch(lib, "", cell, act, T, B, 0, H, x["P"][1].flip(0).contiguous(), x["psh"][1], x["U"][1], x["dY"][:, :, H:].flip(0), save)
    Hp, G = F_._up(H, 8), x["G"]
    out = {"Y": torch.cat([f["Y"], b["Y"].flip(0)], 2),
           "Yb": torch.cat([f["Yb"][:, :H], rev(b["Yb"]).reshape(T * B, -1)[:, :H]], 1)}
    if save:
        out["S"] = torch.stack([f["S"][0], rev(b["S"][0]).reshape(T * B, -1)])
        out["dP2"] = torch.stack([f["dP2"][0], rev(b["dP2"][0]).reshape(T * B, -1)])
        cols = torch.cat([torch.arange(g * Hp, g * Hp + H) for g in range(G)]).cuda()
        out["dGb"] = torch.cat([f["dGb"][:, cols], rev(b["dGb"]).reshape(T * B, -1)[:, cols]], 0)
    return out


@pytest.mark.parametrize("save", [True, False], ids=["train", "forward_only"])
@pytest.mark.parametrize("H,B,T", SHAPES)
@pytest.mark.parametrize("cell,act", CELLS)
def test_one_launch_equals_two_single_direction_launches(cell, act, H, B, T, save):
    lib = _lib.load()
    assert lib.pk_rec_dirs_covered(F_.CELL[cell], F_.ACT[act], T, B, H) == 1
    x = _inputs(cell, H, B, T)
    want = _two_single_launches(lib, cell, act, H, B, T, x, save)
    got = _launch(lib, "_dirs", cell, act, T, B, 1, H, x["P"], x["psh"], x["U"], x["dY"], save)
    Hp, G = F_._up(H, 8), x["G"]
    got["Yb"] = torch.cat([got["Yb"][:, :H], got["Yb"][:, Hp:Hp + H]], 1)
    if save:
        cols = torch.cat([torch.arange(g * Hp, g * Hp + H) for g in range(G)]).cuda()
        got["dGb"] = got["dGb"][:, cols]
    for k, w in want.items():
        assert bool(torch.isfinite(w.float()).all()), k
        assert torch.equal(got[k], w), (k, float((got[k].float() - w.float()).abs().max()))


def _fp64_loop(cell, act, x, T, B, H):
    """Both directions in fp64, U and the h that is fed back rounded to bf16: (Y, dL/dP for L = sum(Y * dY))."""
    bf = lambda t: t.float().bfloat16().double()
    P = x["P"].double().cpu().requires_grad_(True)
    psh, U, fn = x["psh"].double().cpu(), bf(x["U"].cpu()), torch.tanh if act == "tanh" else torch.relu
    ys = []
    for d in range(2):
        h, c, out = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64), [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            # (straight-through rounding: the kernels round the copy that is exchanged, the state itself stays fp32)
            hb = h + (bf(h.detach()) - h.detach())
            pre = P[d, t] + psh[d] + hb @ U[d].t()
            if cell == "LSTM":
                f, i, o, g = pre.split(H, 1)
                c = torch.sigmoid(i) * fn(g) + torch.sigmoid(f) * c
                h = torch.sigmoid(o) * fn(c)
            else:
                h = fn(pre)
            out[t] = h
        ys.append(torch.stack(out))
    Y = torch.cat(ys, 2)
    (Y * x["dY"].double().cpu()).sum().backward()
    return Y.detach(), P.grad.reshape(2, T * B, -1)


@pytest.mark.parametrize("cell,act,H,B,T", [("LSTM", "tanh", 80, 17, 7), ("RNN", "tanh", 13, 16, 7)])
def test_against_an_fp64_loop(cell, act, H, B, T):
    x = _inputs(cell, H, B, T)
    got = _launch(_lib.load(), "_dirs", cell, act, T, B, 1, H, x["P"], x["psh"], x["U"], x["dY"])
    Y, dP = _fp64_loop(cell, act, x, T, B, H)
    e_y, e_dp = rel_err(got["Y"].cpu(), Y), rel_err(got["dP2"].cpu(), dP)
    print("%s H%d B%d T%d: Y %.2e dP2 %.2e" % (cell, H, B, T, e_y, e_dp))
    assert e_y < 1e-2 and e_dp < 1e-2, (e_y, e_dp)


def _run(net, x_cpu, cot_cpu, masks):
    net.zero_grad()
    x = x_cpu.clone().cuda().requires_grad_(True)
    with _lib.Profiler() as prof:
        y = net(x, drop_masks=masks)
        n_fwd = len(prof.events)
        (y * cot_cpu.cuda()).sum().backward()
    torch.cuda.synchronize()
    calls = [name for name, _, _ in prof.events]
    rec = lambda names, way: sum(n.startswith("pk_rec_%s_bf16" % way) for n in names)
    grads = {k: q.grad.detach().cpu().clone() for k, q in net.named_parameters()}
    return y.detach().cpu(), x.grad.detach().cpu(), grads, (rec(calls[:n_fwd], "fwd"), rec(calls[n_fwd:], "bwd"))


@pytest.mark.parametrize("H", [13, 80])
@pytest.mark.parametrize("cls", ["LSTM_cudnn", "RNN_cudnn"])
def test_class_equals_the_one_launch_per_direction_path(cls, H, monkeypatch):
    T, B, D, L, p = 5, 3, 6, 2, 0.25
    torch.manual_seed(7 + H)
    opts = {"hidden_size": str(H), "num_layers": str(L), "bias": "True", "batch_first": "False", "dropout": str(p),
            "bidirectional": "True", "nonlinearity": "tanh", "use_cuda": "True", "to_do": "train"}
    net = getattr(nn_amd, cls)(opts, D)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for k, q in net.named_parameters():
            if "bias" in k:
                q.copy_(0.1 * torch.randn(q.shape, generator=g))
    net.cuda().train()
    x, cot = torch.randn(T, B, D, generator=g), torch.randn(T, B, 2 * H, generator=g)
    masks = [torch.bernoulli(torch.full((T, B, 2 * H), 1 - p), generator=g) for _ in range(L - 1)]
    monkeypatch.setenv("PK_EXPERIMENT", "cudnn_dirs=0")
    y0, dx0, g0, n0 = _run(net, x, cot, masks)
    _, _, g0b, _ = _run(net, x, cot, masks)
    monkeypatch.delenv("PK_EXPERIMENT")
    y1, dx1, g1, n1 = _run(net, x, cot, masks)
    # one recurrence launch per bidirectional layer and pass (two on the old path)
    assert n0 == (2 * L, 2 * L) and n1 == (L, L), (n0, n1)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    d0 = max(rel_err(g0b[k], g0[k]) for k in g0)
    e = {k: rel_err(g1[k], g0[k]) for k in g0}
    print("%s H%d: d0 %.2e, worst gradient %.2e" % (cls, H, d0, max(e.values())))
    for k, v in e.items():
        assert v <= max(1e-5, 2 * d0), (k, v, d0)
    net.eval()  # forward-only equals the grad-mode forward
    ya = net(x.cuda().requires_grad_(True)).detach()
    with torch.no_grad():
        yn = net(x.cuda())
    assert torch.equal(yn, ya)
