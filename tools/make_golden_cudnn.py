"""Generate the LSTM_cudnn / RNN_cudnn fixtures of tests/golden/ from a checkout of the reference (PyTorch-Kaldi).

    python tools/make_golden_cudnn.py /path/to/pytorch-kaldi

TEST INFRASTRUCTURE ONLY, never run by a test.  Imports the reference's ``neural_networks.py`` unmodified, runs its
classes (thin wrappers over torch.nn.LSTM / nn.RNN) on the CPU in fp32 on seeded inputs and stores options, input, state
dict, output, input gradient and parameter gradients:

  e2e_lstm_cudnn_bidir_train      LSTM_cudnn 3 x 8 bidirectional, D 6, T 12, B 3, bias, batch_first=True (the orthogonal
                                  path of the reference's initialisation), dropout 0.0, training
  e2e_lstm_cudnn_uni_eval         LSTM_cudnn 2 x 13 unidirectional, D 7, T 9, B 2, no bias, batch_first=False, dropout 0.2,
                                  .eval() (dropout is the identity)
  e2e_rnn_cudnn_tanh_bidir_train  RNN_cudnn 2 x 8 bidirectional, tanh, D 6, T 12, B 3, training
  e2e_rnn_cudnn_relu_uni_train    RNN_cudnn 2 x 10 unidirectional, relu, D 5, T 8, B 2, training; the seed is the first one
                                  for which no pre-activation of the reference run is closer than 1e-3 to the kink
  train_lstm_cudnn_3steps         LSTM_cudnn 2 x 8 bidirectional -> softmax MLP head of 10 classes, NLL cost, RMSprop with
                                  the hyper-parameters of cfg/TIMIT_baselines/TIMIT_LSTM_fmllr_cudnn.cfg, 3 steps on one
                                  batch

The names start with ``e2e_`` / ``train_`` so that the tests which take every other ``tests/golden/*.npz`` as a module
case of ``neural_networks.py`` leave them alone.
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
RELU_MARGIN = 1e-3


def _import_reference(path):
    try:
        import distutils.util  # noqa: F401  (the reference takes strtobool from it; gone from python 3.12)
    except ImportError:
        def strtobool(s):
            s = str(s).strip().lower()
            if s in ("y", "yes", "t", "true", "on", "1"):
                return 1
            if s in ("n", "no", "f", "false", "off", "0"):
                return 0
            raise ValueError("invalid truth value %r" % (s,))

        pkg, util = types.ModuleType("distutils"), types.ModuleType("distutils.util")
        util.strtobool = strtobool
        pkg.util = util
        sys.modules["distutils"], sys.modules["distutils.util"] = pkg, util
    sys.path.insert(0, path)
    import neural_networks
    return neural_networks


def _save(name, meta, arrays):
    os.makedirs(OUT, exist_ok=True)
    meta = dict(meta, torch=torch.__version__, numpy=np.__version__)
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def _perturb_biases(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "bias" in k:
                p.add_(0.1 * torch.randn(p.shape, generator=g))


def _rnn_min_preact(net, x):
    """Smallest |pre-activation| of an RNN_cudnn run on x (float64, from the module's own parameters): W x_t + b_ih +
    U h_(t-1) + b_hh over all layers, directions, steps, rows and units."""
    rnn = net.rnn[0]
    act = torch.relu if net.nonlinearity == "relu" else torch.tanh
    inp, low = x.detach().double(), float("inf")
    for k in range(net.num_layers):
        outs = []
        for sfx in ("", "_reverse")[:2 if net.bidirectional else 1]:
            w, u = (getattr(rnn, "%s_l%d%s" % (n, k, sfx)).detach().double() for n in ("weight_ih", "weight_hh"))
            b = sum(getattr(rnn, "%s_l%d%s" % (n, k, sfx)).detach().double() for n in ("bias_ih", "bias_hh")) if net.bias else 0.0
            seq = inp.flip(0) if sfx else inp
            h, ys = torch.zeros(seq.shape[1], w.shape[0], dtype=torch.float64), []
            for t in range(seq.shape[0]):
                pre = seq[t] @ w.t() + h @ u.t() + b
                low = min(low, float(pre.abs().min()))
                h = act(pre)
                ys.append(h)
            y = torch.stack(ys)
            outs.append(y.flip(0) if sfx else y)
        inp = torch.cat(outs, 2)
    return low, inp


def module_case(rnn, name, cls, options, inp_dim, T, B, seed, training, relu_margin=False):
    options = dict(options, use_cuda="False", to_do="train" if training else "valid")
    while True:
        torch.manual_seed(seed)
        net = getattr(rnn, cls)(options, inp_dim)
        arrays = {"init/" + k: v.clone() for k, v in net.state_dict().items()}
        if cls == "LSTM_cudnn":
            _perturb_biases(net, seed + 1)  # (the reference's initialisation leaves them zero)
        net.train() if training else net.eval()
        g = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(T, B, inp_dim, generator=g).requires_grad_(True)
        extra = {}
        if not relu_margin:
            break
        low, y64 = _rnn_min_preact(net, x)
        if low >= RELU_MARGIN:
            extra = {"min_abs_preactivation": low}
            break
        seed += 1
    arrays.update({"sd/" + k: v.clone() for k, v in net.state_dict().items()})
    torch.manual_seed(seed + 3)
    y = net(x)
    if relu_margin:
        assert low >= RELU_MARGIN and float((y.detach().double() - y64).abs().max()) < 1e-5, (low, "the float64 replay differs")
    cot = torch.randn(y.shape, generator=g)
    (y * cot).sum().backward()
    arrays.update({"x": x, "y": y, "cot": cot, "dx": x.grad})
    for k, p in net.named_parameters():
        arrays["grad/" + k] = p.grad
    meta = dict({"arch_class": cls, "options": options, "inp_dim": inp_dim, "to_do": options["to_do"], "training": training,
                 "seed": seed, "n_masks": 0, "out_dim": net.out_dim, "T": T, "B": B}, **extra)
    _save(name, meta, arrays)
    if extra:
        print("  seed %d, smallest |pre-activation| %.3e" % (seed, low))


def train_case(rnn, name, seed, T=8, B=4, D=12, n_cls=10, n_steps=3):
    opt = {"arch_opt": "rmsprop", "opt_momentum": "0.0", "opt_alpha": "0.95", "opt_eps": "1e-8", "opt_centered": "False",
           "opt_weight_decay": "0.0", "arch_freeze": "False"}
    rec = dict(opt, arch_class="LSTM_cudnn", hidden_size="8", num_layers="2", bias="True", batch_first="True", dropout="0.0",
               bidirectional="True", arch_lr="0.0016")
    head = dict(opt, arch_class="MLP", dnn_lay=str(n_cls), dnn_drop="0.0", dnn_use_laynorm_inp="False",
                dnn_use_batchnorm_inp="False", dnn_use_batchnorm="False", dnn_use_laynorm="False", dnn_act="softmax",
                arch_lr="0.0016")
    inject = {"use_cuda": "False", "to_do": "train"}
    torch.manual_seed(seed)
    nets = {"LSTM_cudnn_layers": rnn.LSTM_cudnn(dict(rec, **inject), D)}
    nets["MLP_layers"] = rnn.MLP(dict(head, **inject), nets["LSTM_cudnn_layers"].out_dim)
    arrays = {}
    for n, net in nets.items():
        net.train()
        arrays.update({"sd/%s/%s" % (n, k): v.clone() for k, v in net.state_dict().items()})
    optims = [torch.optim.RMSprop(nets[n].parameters(), lr=float(o["arch_lr"]), alpha=float(o["opt_alpha"]),
                                  eps=float(o["opt_eps"]), momentum=0.0, centered=False, weight_decay=0.0)
              for n, o in (("LSTM_cudnn_layers", rec), ("MLP_layers", head))]
    g = torch.Generator().manual_seed(seed + 2)
    inp = torch.randn(T, B, D + 1, generator=g)
    inp[:, :, D] = torch.randint(0, n_cls, (T, B), generator=g).float()
    cost = torch.nn.NLLLoss()
    losses = []
    for _ in range(n_steps):
        out = nets["MLP_layers"](nets["LSTM_cudnn_layers"](inp[:, :, :D]).view(T * B, -1))
        loss = cost(out, inp[:, :, D].reshape(-1).long())
        for o in optims:
            o.zero_grad()
        loss.backward()
        for o in optims:
            o.step()
        losses.append(float(loss.detach()))
    arrays.update({"inp": inp, "loss": np.array(losses, dtype=np.float64)})
    for n, net in nets.items():
        arrays.update({"sd_final/%s/%s" % (n, k): v.clone() for k, v in net.state_dict().items()})
    model = ["out_dnn1=compute(LSTM_cudnn_layers,fea)", "out_dnn2=compute(MLP_layers,out_dnn1)",
             "loss_final=cost_nll(out_dnn2,lab_cd)", "err_final=cost_err(out_dnn2,lab_cd)"]
    meta = {"options": {"architecture1": rec, "architecture2": head}, "model": model, "nfea": D, "T": T, "B": B, "seed": seed,
            "n_cls": n_cls, "n_steps": n_steps, "n_masks": 0}
    _save(name, meta, arrays)
    print("  loss", losses)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rnn = _import_reference(sys.argv[1])
    torch.set_num_threads(1)
    module_case(rnn, "e2e_lstm_cudnn_bidir_train", "LSTM_cudnn",
                {"hidden_size": "8", "num_layers": "3", "bias": "True", "batch_first": "True", "dropout": "0.0",
                 "bidirectional": "True"}, 6, 12, 3, 5101, True)
    module_case(rnn, "e2e_lstm_cudnn_uni_eval", "LSTM_cudnn",
                {"hidden_size": "13", "num_layers": "2", "bias": "False", "batch_first": "False", "dropout": "0.2",
                 "bidirectional": "False"}, 7, 9, 2, 5202, False)
    module_case(rnn, "e2e_rnn_cudnn_tanh_bidir_train", "RNN_cudnn",
                {"hidden_size": "8", "num_layers": "2", "nonlinearity": "tanh", "bias": "True", "batch_first": "False",
                 "dropout": "0.0", "bidirectional": "True"}, 6, 12, 3, 5303, True)
    module_case(rnn, "e2e_rnn_cudnn_relu_uni_train", "RNN_cudnn",
                {"hidden_size": "10", "num_layers": "2", "nonlinearity": "relu", "bias": "True", "batch_first": "False",
                 "dropout": "0.0", "bidirectional": "False"}, 5, 8, 2, 5404, True, relu_margin=True)
    train_case(rnn, "train_lstm_cudnn_3steps", 5505)


if __name__ == "__main__":
    main()
