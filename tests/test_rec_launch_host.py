"""Host side of the persistent recurrences (pk_rec_persist2.hip: pk_rec2_prepare_* / pk_rec2_run and the entry points
in front of them), checked without a GPU: the launch plans and scratch sizes the library answers (pk_num_cu() falls back
to 256 compute units, the MI355X's count, when there is no device), and the argument checks of the eight bf16 entry
points, which all return before the first device call.

The library caches its PK_EXPERIMENT switches per process, so everything is asked in ONE fresh interpreter with
PK_EXPERIMENT removed from its environment; the tests read its answers."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (R, H) -> compute units pk_rec_plan_cus answers
PLAN_CUS = {(1, 8): 1, (10, 550): 45, (256, 550): 144, (600, 24): 40, (600, 550): 216, (66, 14): 8, (4, 576): 36, (4, 577): 0}
# pk_rec_work_floats(cell, T, B, bidir, H) for cells 0 .. 4
WORK_FLOATS = {(9, 300, 1, 24): [469824, 345408, 805056, 680640, 469824],
               (12, 5, 1, 550): [9889920, 4973632, 19724416, 14808128, 9889920]}
LN_WORK_FLOATS = {(9, 300, 1, 24): 99264}
LN_SAVED_FLOATS = {(9, 300, 1, 24): 140464}

LIGRU, GRU = 0, 3
T, B, BIDIR, H = 5, 3, 1, 64  # ndir x Hp = 128; G x Hp = 128 (liGRU), 192 (GRU)
OK = 0x10000                  # a 16-byte aligned host address; nothing dereferences it before the checks under test


def _calls(entry, cell=None, h=H, pitch=None, xoff=0, y=OK, ln=OK):
    """Argument list of one bf16 entry point (include/pk_amd.h), valid up to what the keywords spoil."""
    two = entry.startswith("pk_rec2p")
    fwd = "_fwd_" in entry
    with_ln = entry.endswith("_ln")
    cell = (GRU if two else LIGRU) if cell is None else cell
    pitch = 512 if pitch is None else pitch
    a = [None, cell, 0, T, B, BIDIR, h]
    if fwd:
        a += [OK, OK, OK, OK, OK, 1.0]                          # P, pscale, pshift, U, mask, mask_scalar
        a += [ln, OK, 1e-5] if with_ln else []                  # ln_gamma, ln_beta, ln_eps
        a += [y, OK] + ([OK] if with_ln else [])                # Y, S (, LNS)
        a += [OK + xoff] + ([OK] if two else [])                # Yb (, Xb)
        a += [pitch, 1] + ([OK] if with_ln else [])             # y_pitch, prefilled (, lnwork)
    else:
        a += [OK, OK, 1.0]                                      # U, mask, mask_scalar
        a += [ln, 1e-5] if with_ln else []                      # ln_gamma, ln_eps
        a += [OK, OK] + ([OK] if with_ln else []) + [OK]        # Y, S (, LNS), dY
        a += [] if two else [OK]                                # dP2
        a += [OK + xoff, pitch, 1]                              # dGb, g_pitch, prefilled
        a += [OK, OK, OK] if with_ln else []                    # lnwork, dln_gamma, dln_beta
    return a


ENTRIES = ["pk_rec%s_%s_bf16%s" % (p, d, l) for p in ("", "2p") for d in ("fwd", "bwd") for l in ("", "_ln")]


def _impl(entry):  # the name the messages of the shared implementation carry
    return entry[:-3] if entry.endswith("_ln") else entry


def _rejections():
    """(id, entry, args, expected pk_last_error text)"""
    out = []
    for e in ENTRIES:
        two, fwd, who = e.startswith("pk_rec2p"), "_fwd_" in e, _impl(e)
        out.append(("H577", e, _calls(e, h=577), "%s: bad geometry T=%d B=%d H=577 (H <= 576)" % (who, T, B)))
        what = ("Yb / Xb" if two else "Yb") if fwd else "dGb"
        hold = "2 x 64" if fwd else ("3 x 64" if two else "2 x 64")
        msg = "%s: %s pitch must be a multiple of 8 and hold %s elements" % (who, what, hold)
        for pitch in (40, 64):
            out.append(("pitch%d" % pitch, e, _calls(e, pitch=pitch), msg))
        out.append(("misaligned", e, _calls(e, xoff=2), msg))
        if two:
            out.append(("cell0", e, _calls(e, cell=LIGRU), "%s: cell 0 is not covered by this entry point" % who))
        elif fwd:
            out.append(("Ynull", e, _calls(e, y=None), "pk_rec_fwd_bf16: Y may be null only together with S"))
        if e.endswith("_ln"):
            out.append(("LNnull", e, _calls(e, ln=None), "%s: null LayerNorm argument" % e))
    return out


REJECTIONS = _rejections()

CHILD = r"""
import importlib, json, sys
sys.path.insert(0, sys.argv[1])
lib = importlib.import_module('pytorch-kaldi_amd._lib').load()
q = json.loads(sys.stdin.read())
out = {'cus': [lib.pk_rec_plan_cus(*a) for a in q['cus']],
       'work': [[lib.pk_rec_work_floats(c, *a) for c in range(5)] for a in q['work']],
       'ln_work': [lib.pk_rec_ln_work_floats(*a) for a in q['ln_work']],
       'ln_saved': [lib.pk_rec_ln_saved_floats(*a) for a in q['ln_saved']],
       'rej': []}
for entry, args in q['rej']:
    rc = getattr(lib, entry)(*args)
    out['rej'].append([rc, lib.pk_last_error().decode()])
print('ANSWERS ' + json.dumps(out))
"""


@pytest.fixture(scope="module")
def answers():
    lib_path = os.path.join(ROOT, "pytorch-kaldi_amd", "lib", "libpk_amd.so")
    if not os.path.exists(lib_path):
        sys.path.insert(0, ROOT)
        __import__("importlib").import_module("pytorch-kaldi_amd.build").build()
    q = {"cus": list(PLAN_CUS), "work": list(WORK_FLOATS), "ln_work": list(LN_WORK_FLOATS), "ln_saved": list(LN_SAVED_FLOATS),
         "rej": [[e, a] for _, e, a, _ in REJECTIONS]}
    env = {k: v for k, v in os.environ.items() if k != "PK_EXPERIMENT"}
    r = subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, ROOT], input=json.dumps(q), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ANSWERS ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len("ANSWERS "):])


def test_plans_are_unchanged(answers):
    assert dict(zip(PLAN_CUS, answers["cus"])) == PLAN_CUS


def test_scratch_sizes_are_unchanged(answers):
    assert dict(zip(WORK_FLOATS, answers["work"])) == WORK_FLOATS
    assert dict(zip(LN_WORK_FLOATS, answers["ln_work"])) == LN_WORK_FLOATS
    assert dict(zip(LN_SAVED_FLOATS, answers["ln_saved"])) == LN_SAVED_FLOATS


@pytest.mark.parametrize("i", range(len(REJECTIONS)), ids=["%s-%s" % (e, n) for n, e, _, _ in REJECTIONS])
def test_rejections_are_unchanged(answers, i):
    _, entry, _, text = REJECTIONS[i]
    rc, err = answers["rej"][i]
    assert rc != 0, entry
    assert err == text
