"""Generate the QLSTM fixtures of tests/golden/ from a checkout of the reference (PyTorch-Kaldi).

    python tools/make_golden_qlstm.py /path/to/pytorch-kaldi

TEST INFRASTRUCTURE ONLY, never run by a test.  Imports the reference's ``quaternion_neural_networks.py`` and
``neural_networks.py`` unmodified, runs its classes on the CPU in fp32 on seeded inputs and stores inputs, parameters,
drop masks, outputs and gradients:

  e2e_qlstm_bidir_train   QLSTM 16,8 bidirectional, drop 0.2,0.0, tanh,relu, autograd=False, training
  e2e_qlstm_uni_eval      QLSTM 20 unidirectional, drop 0.3, tanh, autograd=True, to_do=valid (components are 1 x 5)
  train_qlstm_3steps      QLSTM 16,16 bidirectional -> softmax MLP head of 10 classes, NLL cost, RMSprop with the
                          hyper-parameters of cfg/DIRHA_baselines/DIRHA_QLSTM_MFCC.cfg, 3 steps on one batch

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
    import quaternion_neural_networks
    return quaternion_neural_networks, neural_networks


class _MaskTap:
    """Records every torch.bernoulli() result the reference draws in forward (its train-mode drop masks)."""

    def __init__(self):
        self.masks = []

    def __enter__(self):
        self._bern = torch.bernoulli

        def bern(*a, **k):
            m = self._bern(*a, **k)
            self.masks.append(m.clone())
            return m

        torch.bernoulli = bern
        return self

    def __exit__(self, *exc):
        torch.bernoulli = self._bern


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
            if k.endswith(".bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))


def module_case(qnn, name, options, inp_dim, T, B, seed):
    options = dict(options, use_cuda="False")
    np.random.seed(seed)
    net = qnn.QLSTM(options, inp_dim)
    arrays = {"init/" + k: v.clone() for k, v in net.state_dict().items()}
    _perturb_biases(net, seed + 1)  # (the initialiser leaves them zero)
    training = options["to_do"] == "train"
    net.train() if training else net.eval()
    arrays.update({"sd/" + k: v.clone() for k, v in net.state_dict().items()})
    g = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(T, B, inp_dim, generator=g).requires_grad_(True)
    torch.manual_seed(seed + 3)
    with _MaskTap() as tap:
        y = net(x)
    cot = torch.randn(y.shape, generator=g)
    (y * cot).sum().backward()
    arrays.update({"x": x, "y": y, "cot": cot, "dx": x.grad})
    for k, p in net.named_parameters():
        arrays["grad/" + k] = p.grad
    masks = tap.masks
    if not training:  # test mode: the 1-element scalar 1 - p the reference multiplies with (:126)
        masks = [torch.FloatTensor([1 - p]) for p in net.lstm_drop]
    for i, m in enumerate(masks):
        arrays["mask/%d" % i] = m
    meta = {"arch_class": "QLSTM", "options": options, "inp_dim": inp_dim, "to_do": options["to_do"], "training": training,
            "seed": seed, "n_masks": len(masks), "out_dim": net.out_dim, "T": T, "B": B}
    _save(name, meta, arrays)


def train_case(qnn, rnn, name, seed, T=8, B=4, D=12, n_cls=10, n_steps=3):
    opt = {"arch_opt": "rmsprop", "opt_momentum": "0.0", "opt_alpha": "0.95", "opt_eps": "1e-8", "opt_centered": "False",
           "opt_weight_decay": "0.0", "arch_freeze": "False"}
    rec = dict(opt, arch_class="QLSTM", lstm_lay="16,16", lstm_drop="0.0,0.0", lstm_bidir="True", lstm_act="tanh,tanh",
               quaternion_init="quaternion", autograd="False", arch_lr="0.0016")
    head = dict(opt, arch_class="MLP", dnn_lay=str(n_cls), dnn_drop="0.0", dnn_use_laynorm_inp="False",
                dnn_use_batchnorm_inp="False", dnn_use_batchnorm="False", dnn_use_laynorm="False", dnn_act="softmax",
                arch_lr="0.0004")
    inject = {"use_cuda": "False", "to_do": "train"}
    np.random.seed(seed)
    torch.manual_seed(seed)
    nets = {"QLSTM": qnn.QLSTM(dict(rec, **inject), D)}
    nets["MLP_layers"] = rnn.MLP(dict(head, **inject), nets["QLSTM"].out_dim)
    arrays = {}
    for n, net in nets.items():
        net.train()
        arrays.update({"sd/%s/%s" % (n, k): v.clone() for k, v in net.state_dict().items()})
    optims = [torch.optim.RMSprop(nets[n].parameters(), lr=float(o["arch_lr"]), alpha=float(o["opt_alpha"]),
                                  eps=float(o["opt_eps"]), momentum=0.0, centered=False, weight_decay=0.0)
              for n, o in (("QLSTM", rec), ("MLP_layers", head))]
    g = torch.Generator().manual_seed(seed + 2)
    inp = torch.randn(T, B, D + 1, generator=g)
    inp[:, :, D] = torch.randint(0, n_cls, (T, B), generator=g).float()
    cost = torch.nn.NLLLoss()
    losses = []
    for _ in range(n_steps):
        out = nets["MLP_layers"](nets["QLSTM"](inp[:, :, :D]).view(T * B, -1))
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
    model = ["out_dnn1=compute(QLSTM,fea)", "out_dnn2=compute(MLP_layers,out_dnn1)", "loss_final=cost_nll(out_dnn2,lab_cd)",
             "err_final=cost_err(out_dnn2,lab_cd)"]
    meta = {"options": {"architecture1": rec, "architecture2": head}, "model": model, "nfea": D, "T": T, "B": B, "seed": seed,
            "n_cls": n_cls, "n_steps": n_steps, "n_masks": 0}
    _save(name, meta, arrays)
    print("  loss", losses)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    qnn, rnn = _import_reference(sys.argv[1])
    torch.set_num_threads(1)
    module_case(qnn, "e2e_qlstm_bidir_train",
                {"lstm_lay": "16,8", "lstm_drop": "0.2,0.0", "lstm_act": "tanh,relu", "lstm_bidir": "True",
                 "quaternion_init": "quaternion", "autograd": "False", "to_do": "train"}, 12, 7, 3, 4101)
    module_case(qnn, "e2e_qlstm_uni_eval",
                {"lstm_lay": "20", "lstm_drop": "0.3", "lstm_act": "tanh", "lstm_bidir": "False",
                 "quaternion_init": "quaternion", "autograd": "True", "to_do": "valid"}, 4, 5, 2, 4202)
    train_case(qnn, rnn, "train_qlstm_3steps", 4303)


if __name__ == "__main__":
    main()
