"""Which kernel family pk_quat_linear_* takes: the rule of pk_quat_linear_variant and its override (no GPU)."""
import importlib

import pytest

_lib = importlib.import_module("pytorch-kaldi_amd._lib")
PASSES, PRECS = (0, 1, 2), (0, 1)  # forward, dX, dcomp; PK_PREC_F32, PK_PREC_BF16


def test_the_entries_exist_and_bind():
    lib = _lib.load()
    for n, nargs in {"pk_quat_linear_variant": 5, "pk_quat_linear_set_variant": 1}.items():
        assert hasattr(lib, n) and len(_lib.SIGNATURES[n][1]) == nargs, n
    assert lib.pk_quat_linear_variant(3, 0, 64000, 256, 256) == 0 and lib.pk_quat_linear_variant(0, 2, 64000, 256, 256) == 0
    assert lib.pk_quat_linear_variant(0, 0, 64000, 256, 1 << 21) == 0  # out of range: pass, prec, O


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pas", PASSES)
def test_rule_and_override(pas, prec):
    lib = _lib.load()
    v = lambda N: lib.pk_quat_linear_variant(pas, prec, N, 256, 256)  # noqa: E731
    try:
        lib.pk_quat_linear_set_variant(-1)
        assert v(128) == 0 and v(64000) == 1
        picks = [v(N) for N in range(128, 64001, 128)]
        assert picks == sorted(picks)  # monotone in N: one switch from 0 to 1
        for forced in (0, 1):
            lib.pk_quat_linear_set_variant(forced)
            assert v(128) == forced and v(64000) == forced
        lib.pk_quat_linear_set_variant(-1)
        assert v(128) == 0 and v(64000) == 1
    finally:
        lib.pk_quat_linear_set_variant(-1)
