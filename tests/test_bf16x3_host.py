"""Host side of the bf16x3 precision: the switch, what the non-GEMM entries are handed under it, and pk_gemm's argument
checks (no device call is reached)."""
import importlib

F_ = importlib.import_module("pytorch-kaldi_amd.functional")
_lib = importlib.import_module("pytorch-kaldi_amd._lib")


def test_switch_and_entry_precision():
    assert F_.PREC["bf16x3"] == 2
    F_.set_precision("bf16x3")  # (conftest's settings fixture restores the mode)
    assert F_.settings.precision == "bf16x3" and not F_.bf16_mode()
    assert F_.entry_prec() == F_.PREC["fp32"] == 0
    for prec in ("fp32", "bf16"):
        F_.set_precision(prec)
        assert F_.entry_prec() == F_.PREC[prec]


def test_pk_gemm_takes_prec_2():
    lib = _lib.load()

    def error_of(prec, a_rs, a_cs, splitk):
        rc = lib.pk_gemm(None, prec, 4, 4, 4, 1.0, None, a_rs, a_cs, None, 1, 4, 0.0, None, 4, None, splitk, None)
        return rc, lib.pk_last_error()

    # the degenerate call of tests/test_abi.py (bad strides), then a split without a workspace: the check behind the
    # one on `prec`, and the last before anything touches the device
    for a_rs, a_cs, splitk, word in ((3, 2, 1, b"contiguous"), (4, 1, 2, b"workspace")):
        rc0, msg0 = error_of(0, a_rs, a_cs, splitk)
        rc2, msg2 = error_of(2, a_rs, a_cs, splitk)
        assert rc0 != 0 and word in msg0
        assert (rc2, msg2) == (rc0, msg0) and b"bad prec" not in msg2
    rc, msg = error_of(3, 4, 1, 2)
    assert rc != 0 and b"bad prec 3" in msg
