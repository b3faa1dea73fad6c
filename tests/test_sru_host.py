"""nn.SRU without a GPU: state-dict names, order and shapes, out_dim, initial bias halves, the flat-parameter layout, the
refusals at construction and the refusal of a CPU tensor; and what test_gpu_sru.py's scan cases assume of their inputs (which
block loops a walk enters, min |c_t| of the relu / selu cases, the lengths that share a wave)."""
import importlib

import pytest
import torch

import sru_cases as sc

nn_amd = importlib.import_module("pytorch-kaldi_amd.nn")
F_amd = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")


def _opts(**kw):
    o = {"sru_hidden_size": 6, "sru_num_layers": 2, "sru_dropout": 0.1, "sru_rnn_dropout": 0.1, "sru_use_tanh": False,
         "sru_use_relu": False, "sru_use_selu": False, "sru_weight_norm": False, "sru_layer_norm": False,
         "sru_bidirectional": True, "sru_is_input_normalized": False, "sru_has_skip_term": True, "sru_rescale": True,
         "sru_highway_bias": -1.5, "sru_n_proj": 0, "use_cuda": True, "to_do": "train"}
    o.update(kw)
    return {k: str(v) for k, v in o.items()}


# (options, inp_dim) -> per layer: weight shape, weight_proj shape or None (out = 12 bidirectional, 6 otherwise)
LAYOUTS = [
    (dict(), 20, [((20, 48), None), ((12, 36), None)]),                            # k = 4 then k = 3
    (dict(sru_n_proj=4), 20, [((4, 48), (20, 4)), ((4, 36), (12, 4))]),            # projection in both layers
    (dict(sru_n_proj=12), 20, [((20, 48), None), ((12, 36), None)]),               # n_proj not below min(n_in, out): none
    (dict(sru_bidirectional=False), 6, [((6, 18), None), ((6, 18), None)]),        # inp_dim == out: k = 3 from the start
    (dict(sru_has_skip_term=False), 20, [((20, 36), None), ((12, 36), None)]),     # no skip term: k = 3 everywhere
]


@pytest.mark.parametrize("kw,inp_dim,want", LAYOUTS)
def test_state_dict_names_order_shapes_and_initial_bias(kw, inp_dim, want):
    net = nn_amd.SRU(_opts(**kw), inp_dim)
    out = 6 * (2 if kw.get("sru_bidirectional", True) else 1)
    assert net.out_dim == out
    names, shapes = [], []
    for i, (w, wp) in enumerate(want):
        pre = "sru.rnn_lst.%d." % i
        names += [pre + "weight"] + ([pre + "weight_proj"] if wp else []) + [pre + "weight_c", pre + "bias"]
        shapes += [w] + ([wp] if wp else []) + [(2 * out,), (2 * out,)]
    sd = net.state_dict()
    assert list(sd) == names and [k for k, _ in net.named_parameters()] == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    for i in range(2):
        b = sd["sru.rnn_lst.%d.bias" % i]
        assert torch.equal(b[:out], torch.zeros(out)) and torch.equal(b[out:], torch.full((out,), -1.5))
        assert float(sd["sru.rnn_lst.%d.weight_c" % i].abs().max()) <= 1.5 ** 0.5 + 1e-6
    groups = net.pk_flat_groups()
    assert sorted(id(q) for grp in groups for q in grp) == sorted(id(p) for p in net.parameters())
    assert net.pk_unused_parameters() == []


@pytest.mark.parametrize("kw", [dict(sru_weight_norm=True), dict(sru_layer_norm=True), dict(sru_dropout=1.0),
                                dict(sru_rnn_dropout=-0.1), dict(sru_hidden_size=0), dict(sru_num_layers=0),
                                dict(sru_use_tanh=True, sru_use_selu=True)])
def test_refusals_at_construction(kw):
    with pytest.raises(_lib.PkError):
        nn_amd.SRU(_opts(**kw), 8)


def test_cpu_tensor_is_refused():
    with pytest.raises(_lib.PkError):
        nn_amd.SRU(_opts(), 8)(torch.randn(5, 2, 8))
    with pytest.raises(_lib.PkError):
        F_amd.sru_scan(torch.randn(5, 2, 36), None, torch.zeros(24), torch.zeros(24), 1.0, "none", bidirectional=True)


# ---- the input conditions of test_gpu_sru.py's scan cases, so that a failure on the GPU can only mean the kernel

def test_ring_cases_enter_the_loops_their_comments_name():
    blocks = {T: sc.ring_blocks(T) for T in (1, 3, 8, 9, 16, 17, 24, 25, 37, 41, 70, 130)}
    assert blocks == {1: (0, 1), 3: (0, 1), 8: (0, 1), 9: (0, 2), 16: (0, 2), 17: (1, 2), 24: (1, 2), 25: (2, 2), 37: (3, 2),
                      41: (4, 2), 70: (7, 2), 130: (15, 2)}
    for n in range(1, 150):  # the two loops cover a walk exactly once, and an unguarded block never reaches past it
        full, guarded = sc.ring_blocks(n)
        assert (full + guarded) * sc.SRU_P >= n > (full + guarded - 1) * sc.SRU_P
        assert full == 0 or (full - 1) * sc.SRU_P + 2 * sc.SRU_P + 1 <= n
    # every (K, HASX) form with every set of output gradients runs unguarded blocks: the nine instances of the backward kernel
    nine = {(c.k, c.skip, c.grads) for c in sc.RING if c.T == 41 and c.act in ("none", "tanh")}
    assert nine == {(k, skip, g) for k, skip in sc.FORMS for g in ("y", "ym", "both")}
    assert {c.T for c in sc.RING if (c.k, c.skip, c.grads, c.mask_h) == (3, True, "both", True)} >= {8, 9, 16, 17, 24, 25}
    assert any(sc.ring_blocks(c.T) == (1, 2) and (c.k, c.grads) == (4, "ym") for c in sc.RING)
    assert all((c.B, c.D, c.H) == (3, 2, 20) for c in sc.RING)  # 120 columns: a wave over the direction and the sentence boundary


@pytest.mark.parametrize("case", [sc.ScanCase(*c[:5], None, *c[5:7], None, c[7]) for c in sc.SCAN] + sc.RING, ids=lambda c: c.id)
def test_scan_cases_keep_off_the_kink(case):
    ref, min_c = sc.scan_reference(case)
    print(tuple(case), "min |c_t| %.2e" % min_c)
    # nothing to divide by zero in a relative error (one step alone has c_prev = 0 and no gradient of weight_c)
    assert all(bool(torch.isfinite(t).all()) and (float(t.norm()) > 0 or case.T == 1) for t in ref.values())
    assert ("Ym" in ref) == (case.grads is not None) and ("dx_skip" in ref) == (sc.scan_inputs(case)[1] is not None)
    if case.act in ("relu", "selu"):
        assert min_c >= sc.MIN_C, min_c


def test_length_cases_split_a_wave_between_the_loops():
    T, B, D, H = sc.LENS_CASES[0][:4]
    assert len(sc.LENS) == B and all(1 <= n <= T for n in sc.LENS) and [c[4:6] for c in sc.LENS_CASES] == sc.FORMS
    out = D * H
    waves = [{sc.LENS[gid // out] for gid in range(w, min(w + 64, B * out))} for w in range(0, B * out, 64)]
    mixed = [sorted(sc.ring_blocks(n)[0] for n in w) for w in waves]  # unguarded blocks per lane, by wave
    print(waves, mixed)
    assert {41, 40} <= waves[0] and mixed[0] == [3, 4]  # one lane in its last unguarded block, its neighbour already guarded
    assert any({17, 16} <= w for w in waves)            # one lane with an unguarded block, its neighbour with none
    # the clamp case: lengths on both sides of 0 .. T, which functional.sentence_lengths refuses and the kernel must clamp
    T = sc.CLAMP_CASE.T
    assert min(sc.CLAMP_LENS) < 0 < T < max(sc.CLAMP_LENS) and 0 in sc.CLAMP_LENS
    with pytest.raises(_lib.PkError, match="sentence lengths must lie in"):
        F_amd.sentence_lengths(sc.CLAMP_LENS).check("sru_scan", torch.zeros(T, len(sc.CLAMP_LENS), 1))
