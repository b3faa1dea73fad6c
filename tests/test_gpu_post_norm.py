"""functional.post_normalize (pk_post_normalize, pk_seqlen.hip): log-posteriors minus log-priors with the padding rows of a
decoding batch dropped in the same pass, against numpy's own expression - the reference's
`out_save - np.log(counts / np.sum(counts))` (core.py:665-668) - with np.array_equal: the widening of an fp32 value is
exact and the one IEEE subtraction is correctly rounded on both sides, so there is no tolerance.  The result has the type
numpy's has: float64 for float64 log-priors, float32 for the float32 ones data_io.load_counts leads to (both are checked;
the arks of the recipes are float32 matrices).  Then one forward chunk through core.run_nn_dp with the device path on,
byte for byte against an ark the test builds from the un-normalised posteriors and that expression."""
import importlib
import io

import numpy as np
import pytest
import torch

from golden_util import Golden

pytestmark = pytest.mark.gpu

F_ = importlib.import_module("pytorch-kaldi_amd.functional")
core = importlib.import_module("pytorch-kaldi_amd.core")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")

DTYPES = {"f64": np.float64, "f32": np.float32}


def _posteriors(R, C, seed):
    """Values in [-30, 0] with -inf and 0.0 in a few places (a log-posterior may be -inf; -inf - lp stays -inf)."""
    rng = np.random.RandomState(seed)
    x = (-30.0 * rng.rand(R, C)).astype(np.float32)
    flat = x.reshape(-1)
    for k, v in ((flat.size // 3, 0.0), (flat.size // 2, 0.0), (0, -np.inf), (flat.size - 1, -np.inf)):
        flat[k] = v
    return x


def _logprior(C, seed, dtype):
    """From integer counts with a count of 1 next to one of 10^7, the way the chunk loop computes it."""
    counts = np.random.RandomState(seed).randint(1, 5000, size=C)
    counts[0] = 1
    if C > 1:
        counts[1] = 10 ** 7
    c = counts.astype(dtype)
    return np.log(c / np.sum(c))


def _check(x, lp, rows):
    want = (x if rows is None else x[rows]) - lp  # numpy: float32 - float64 -> float64, float32 - float32 -> float32
    got = F_.post_normalize(torch.from_numpy(x).cuda(), torch.from_numpy(lp).cuda(),
                            None if rows is None else torch.from_numpy(rows).cuda())
    assert got.dtype == {np.float64: torch.float64, np.float32: torch.float32}[lp.dtype.type]
    assert want.dtype == lp.dtype and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.isneginf(want).any()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("n,C", [(1, 1), (5, 7), (3, 48), (257, 1938), (2, 2051)])
def test_post_normalize_identity_rows_equal_numpy(n, C, dtype):
    _check(_posteriors(n, C, n + C), _logprior(C, C, DTYPES[dtype]), None)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [7, 1938])
@pytest.mark.parametrize("lens,max_len", [([1, 4, 2], 4), ([9, 3, 9, 1, 5], 9)])
def test_post_normalize_through_a_padded_rows_map_equals_numpy(lens, max_len, C, dtype):
    rows = core.padded_rows(lens, max_len)
    assert len(rows) == sum(lens) < max_len * len(lens)  # (the gather skips padding rows)
    x = _posteriors(max_len * len(lens), C, C + max_len)
    _check(x, _logprior(C, 3, DTYPES[dtype]), rows)
    # the host copy of the map, when handed over, is what the range check reads: same result
    lp = _logprior(C, 3, DTYPES[dtype])
    got = F_.post_normalize(torch.from_numpy(x).cuda(), torch.from_numpy(lp).cuda(), torch.from_numpy(rows).cuda(), rows)
    assert np.array_equal(got.cpu().numpy(), x[rows] - lp)


def test_post_normalize_refusals(monkeypatch):
    x = torch.from_numpy(_posteriors(6, 5, 1)).cuda()
    lp = torch.from_numpy(_logprior(5, 1, np.float64)).cuda()
    with pytest.raises(_lib.PkError):
        F_.post_normalize(x.cpu(), lp)
    with pytest.raises(_lib.PkError):
        F_.post_normalize(x.double(), lp)
    with pytest.raises(_lib.PkError):
        F_.post_normalize(x, torch.from_numpy(_logprior(4, 1, np.float64)).cuda())
    with pytest.raises(_lib.PkError):
        F_.post_normalize(x, lp.cpu())
    # a row index past the input: refused on the host, nothing is launched
    launched = []
    lib = _lib.load()

    class Spy:
        def __getattr__(self, name):
            if name == "pk_post_normalize":
                return lambda *a: launched.append(a) or 0
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    for bad in ([0, 6], [7, 1], [-1, 2]):
        rows = torch.tensor(bad, dtype=torch.int64)
        with pytest.raises(_lib.PkError):
            F_.post_normalize(x, lp, rows.cuda())
        with pytest.raises(_lib.PkError):
            F_.post_normalize(x, lp, rows.cuda(), rows.numpy())
    assert launched == []
    F_.post_normalize(x, lp, torch.tensor([0, 5], dtype=torch.int64).cuda())  # (the spy does see an accepted call)
    assert len(launched) == 1


# --------------------------------------------------------------------------------
# one forward chunk through run_nn_dp, device path on
# --------------------------------------------------------------------------------
def _forward_run(g, tmp_path, out, monkeypatch, n, normalize, experiment):
    """The fixture's forward chunk (built as tests/test_core_chunk.py builds its `forward` run): ark bytes."""
    from test_core_chunk import engine_cfg

    meta = g.meta
    out.mkdir()
    text = engine_cfg(g, "forward", tmp_path).replace(str(tmp_path) + "/forward.info", str(out) + "/forward.info")
    if not normalize:
        assert "normalize_posteriors = True" in text
        text = text.replace("normalize_posteriors = True", "normalize_posteriors = False")
    monkeypatch.setenv("PK_FORWARD_BATCH", str(n))
    if experiment is None:
        monkeypatch.delenv("PK_EXPERIMENT", raising=False)
    else:
        monkeypatch.setenv("PK_EXPERIMENT", experiment)
    path = out / "forward.cfg"
    path.write_text(text)
    data, end = g.arrays["data_set"], g.arrays["data_end_index"]
    args = [meta["data_name"], torch.from_numpy(data).cuda(), end, {k: list(v) for k, v in meta["fea_dict"].items()},
            meta["lab_dict"], meta["arch_dict"]]
    core.run_nn_dp(*args, str(path), False, str(path), reader=lambda *a: None)
    assert (out / "forward.info").exists()
    return open(out / "forward_out_dnn2_to_decode.ark", "rb").read()


@pytest.mark.parametrize("n", [1, 3])
def test_run_nn_dp_normalises_on_the_device_to_the_reference_formula(tmp_path, monkeypatch, n):
    from test_core_chunk import CASE, checkpoint_from_fixture, parse_ark

    g = Golden(CASE)
    for i in (1, 2, 3):
        torch.save(checkpoint_from_fixture(g, "ck1", "architecture%d" % i), tmp_path / ("ck1_architecture%d.pkl" % i))
    with open(tmp_path / "counts", "w") as f:
        f.write("[ " + " ".join(str(int(c)) for c in g.arrays["counts"]) + " ]\n")
    calls = []
    real = F_.post_normalize
    monkeypatch.setattr(F_, "post_normalize", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    raw = parse_ark(_forward_run(g, tmp_path, tmp_path / "raw", monkeypatch, n, False, "post_norm_device=1"))
    assert calls == []  # (nothing to normalise: today's path)
    # the expected ark: the reference's expression on the un-normalised posteriors, written by the same writer
    counts = core.load_counts(str(tmp_path / "counts"))
    want = io.BytesIO()
    for key, m in raw:
        core.write_mat(want, m - np.log(counts / np.sum(counts)), key)
    got = _forward_run(g, tmp_path, tmp_path / "dev", monkeypatch, n, True, "post_norm_device=1")
    n_groups = len(core.forward_groups(np.diff(g.arrays["data_end_index"], prepend=0), n))
    assert len(calls) == n_groups  # one launch per group and normalised output, the padding strip included
    assert got == want.getvalue()
    # the host path of the A/B switch gives the same bytes, and the default is one of the two
    assert _forward_run(g, tmp_path, tmp_path / "host", monkeypatch, n, True, "post_norm_device=0") == got
    assert len(calls) == n_groups
    assert _forward_run(g, tmp_path, tmp_path / "default", monkeypatch, n, True, None) == got
