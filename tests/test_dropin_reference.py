"""The drop-in, checked against what the REFERENCE's own caller builds.

A PyTorch-Kaldi user switches engines by editing one cfg line per architecture (arch_library).  The caller then
instantiates ``arch_class(options, inp_dim)`` through importlib (utils.model_init, utils.py:2047-2057), builds torch
optimizers over ``.parameters()`` (utils.optimizer_init, utils.py:2106-2164) and loads the previous chunk's ``.pkl`` into
both (core.py:523-535).  tests/golden/dropin_model_init.json holds what the reference's model_init + optimizer_init built
from the shipped cfg files with its own neural_networks (oracle/make_golden.py::dropin_case: every name, out_dim, shape,
dtype, optimizer group and the SHA-256 of every initial value at seed 1234 - with a float64 fingerprint of the
orthogonally initialised matrices, whose LAPACK QR may round differently on another host) and the cfg files themselves; these tests run
the package's model_init / optimizer_init (pytorch-kaldi_amd/utils.py, the same importlib dispatch) on those cfg files
with ``arch_library = pytorch-kaldi_amd.nn`` and require the same result.
"""
import configparser
import hashlib
import importlib
import json
import os

import pytest
import torch

from golden_util import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "dropin_model_init.json")))


@pytest.fixture(scope="module")
def ref_utils():
    """The caller: the package's model_init / optimizer_init (they dispatch on arch_library as the reference's do)."""
    return importlib.import_module("pytorch-kaldi_amd.utils")


def _cfg(text, library, n_out):
    cfg = configparser.ConfigParser()
    cfg.read_string(text)
    cfg["exp"]["to_do"] = "train"
    cfg["exp"]["use_cuda"] = "False"  # construction only: the engine's forward needs the GPU
    for sec in cfg.sections():
        if sec.startswith("architecture"):
            cfg[sec]["arch_library"] = library
            for k, v in cfg[sec].items():
                if v in n_out:
                    cfg[sec][k] = str(n_out[v])
    return cfg


RECIPES = [
    ("cfg/TIMIT_baselines/TIMIT_liGRU_fmllr.cfg", 40),
    ("cfg/TIMIT_baselines/TIMIT_LSTM_fmllr.cfg", 40),
    ("cfg/TIMIT_baselines/TIMIT_MLP_fmllr.cfg", 440),
    ("cfg/TIMIT_baselines/TIMIT_SincNet_raw.cfg", 3200),
    ("cfg/Librispeech_baselines/libri_GRU_fmllr.cfg", 40),
]


def _build(ref_utils, path, library, feat_dim):
    n_out = {"N_out_lab_cd": 1938, "N_out_lab_mono": 48}
    cfg = _cfg(GOLD[path]["cfg"], library, n_out)
    model = cfg["model"]["model"].split("\n")
    arch_dict = {}
    for sec in cfg.sections():
        if sec.startswith("architecture"):
            arch_dict[cfg[sec]["arch_name"]] = [sec, cfg[sec]["arch_name"], bool(ref_utils.strtobool(cfg[sec]["arch_seq_model"]))]
    fea = [ln for ln in model if "compute" in ln][0].split(",")[1].strip(" )")
    inp_out_dict = {fea: [0, feat_dim, feat_dim]}
    nns, costs = ref_utils.model_init(inp_out_dict, model, cfg, arch_dict, False, False, "train")
    opts = ref_utils.optimizer_init(nns, cfg, arch_dict)
    return cfg, nns, costs, opts, inp_out_dict


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("path,feat_dim", RECIPES)
def test_reference_model_init_builds_the_engine_classes(ref_utils, path, feat_dim):
    """model_init + optimizer_init on the SHIPPED cfg with arch_library switched: same architectures, out_dims,
    parameter names / shapes / order, optimizer types and hyper-parameters as the reference's caller built with the
    reference's own neural_networks - and, with the same seed, the same initial weights."""
    nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
    want = GOLD[path]
    assert want["feat_dim"] == feat_dim
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (as the fixture was recorded: the orthogonal initialisation's QR, bit for bit)
    try:
        torch.manual_seed(1234)
        _, nns_e, costs_e, opts_e, iod_e = _build(ref_utils, path, "pytorch-kaldi_amd.nn", feat_dim)
    finally:
        torch.set_num_threads(threads)
    assert list(nns_e) == want["nns"] and list(costs_e) == want["costs"]
    assert {k: list(v) for k, v in iod_e.items()} == want["inp_out_dict"]  # every out_dim the interpreter derived
    for name, r in want["nets"].items():
        e = nns_e[name]
        assert type(e).__module__ == nn_amd.__name__ and type(e).__name__ == r["class"]
        assert e.out_dim == r["out_dim"] and e.training == r["training"]
        assert [k for k, _ in e.named_parameters()] == r["parameters"]  # the order indexes torch optimizer state
        sde = e.state_dict()
        assert list(sde) == [k for k, _, _, _ in r["state_dict"]]
        for k, shape, dtype, sha in r["state_dict"]:
            assert list(sde[k].shape) == shape and str(sde[k].dtype) == dtype, (name, k)
            if _sha(sde[k]) != sha:  # same seed -> same initialisation
                # (only where LAPACK's QR is involved may another host's last bits differ from the recorded ones)
                fp = r["orthogonal"].get(k)
                assert fp is not None, (name, k)
                # (fp32 QR rounding: up to ~2e-6 per element, of either sign - a sum of n of them grows as sqrt(n))
                w = sde[k].double().reshape(-1)
                assert abs(float(w.sum()) - fp["sum"]) < 1e-5 * w.numel() ** 0.5, (name, k)
                assert abs(float((w * w).sum()) - fp["sumsq"]) < 1e-5 * fp["sumsq"], (name, k)
                assert torch.allclose(w[fp["idx"]], torch.tensor(fp["values"], dtype=torch.float64), rtol=1e-5, atol=1e-5), (name, k)
        assert type(opts_e[name]).__name__ == r["optimizer"] and type(opts_e[name]).__module__.startswith("torch.optim")
        assert json.loads(json.dumps(opts_e[name].state_dict()["param_groups"])) == r["param_groups"]
        # a checkpoint of this architecture in the reference's layout loads into the engine's module and its optimizer
        ck = {"model_par": {k: v.clone() for k, v in sde.items()}, "optimizer_par": opts_e[name].state_dict()}
        e.load_state_dict(ck["model_par"])
        opts_e[name].load_state_dict(ck["optimizer_par"])


def test_reference_written_checkpoint_loads_through_the_reference_caller(ref_utils, tmp_path):
    """core.py:523-535 with a REAL reference checkpoint: tests/golden/chunk_ligru_run_nn.npz holds the .pkl contents
    the reference's run_nn wrote after its first training chunk (model_par + RMSprop state after several steps)."""
    g = Golden("chunk_ligru_run_nn")
    m = g.meta
    cfg = configparser.ConfigParser()
    cfg.read_string(m["cfgs"]["ck1"].replace("{OUT}", str(tmp_path)))
    arch_dict = m["arch_dict"]
    for sec in ("architecture1", "architecture2", "architecture3"):
        cfg[sec]["arch_library"] = "pytorch-kaldi_amd.nn"
    model = cfg["model"]["model"].split("\n")
    inp_out_dict = {"fmllr": m["fea_dict"]["fmllr"][5:]}
    nns, costs = ref_utils.model_init(inp_out_dict, model, cfg, arch_dict, False, False, "train")
    opts = ref_utils.optimizer_init(nns, cfg, arch_dict)
    for name, net in nns.items():
        sec = arch_dict[name][0]
        model_par = g.group("ck0/%s/model_par/" % sec)
        state = {}
        for key, v in g.group("ck0/%s/opt/" % sec).items():
            idx, field = key.split("/")
            state.setdefault(int(idx), {})[field] = v
        optimizer_par = {"state": state, "param_groups": m["param_groups"]["ck0/%s" % sec]}
        net.load_state_dict(model_par)                      # core.py:531
        opts[name].load_state_dict(optimizer_par)           # core.py:532
        opts[name].param_groups[0]["lr"] = float(cfg[sec]["arch_lr"])  # core.py:533-535
        for k, v in net.state_dict().items():
            assert torch.equal(v, model_par[k]), (name, k)
        got = opts[name].state_dict()["state"]
        assert sorted(got) == sorted(state)
        params = list(net.parameters())
        for idx, ent in state.items():
            assert got[idx]["square_avg"].shape == params[idx].shape
            assert torch.equal(got[idx]["square_avg"], ent["square_avg"])
