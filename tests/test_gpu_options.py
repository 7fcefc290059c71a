"""dmp_ctx_get_option / dmp_ctx_set_option against a recording (tests/golden/options.json, tools/record_options.py).

The recording was made on the commit before the two if-chains became one option table: for every option name of
include/dmpfold_hip.h - and one unknown name - what a fresh context (max_L 8, max_N 1) reads, and for each probe value the
setter's return code, its dmp_last_error text and what the option reads afterwards.  The library must answer all of it the
same: the names, the defaults, the values accepted and rejected, every error text.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "options.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_options", os.path.join(ROOT, "tools", "record_options.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert [mod.MAX_L, mod.MAX_N, list(mod.PROBES), mod.UNTOUCHED] == [RECORDED[k] for k in ("max_L", "max_N", "probes", "untouched")]
    assert set(mod.NAMES) | {mod.UNKNOWN} == set(RECORDED["options"])
    return mod


@pytest.mark.parametrize("name", sorted(RECORDED["options"]))
def test_option_answers_as_recorded(recorder, name):
    from dmpfold2_amd import _lib
    got = recorder.probe(_lib.load(), name)
    want = RECORDED["options"][name]
    assert got["fresh"] == want["fresh"]
    for g, w in zip(got["set"], want["set"]):
        assert g == w
    assert len(got["set"]) == len(want["set"])


def test_unknown_name_fails_as_recorded(recorder):
    rec = RECORDED["options"][recorder.UNKNOWN]
    assert rec["fresh"][0] < 0 and rec["fresh"][2] == "unknown option " + recorder.UNKNOWN
    assert all(s[1] < 0 and s[2] == "unknown option " + recorder.UNKNOWN for s in rec["set"])
