"""The one Python description of the `d_conf` buffer (score.Layout behind score.split_conf_buffer, score.Outputs), the
per-call options of an engine (Engine._call_options with a predict.Extras) and the rule the engines of a pipeline must agree
by (predict.agree_options).  No GPU."""
import itertools

import numpy as np
import pytest
import torch

from dmpfold2_amd import score as S
from dmpfold2_amd.predict import Engine, Extras, agree_options

LENGTHS = (8, 9, 82, 2048)
FLAGS = list(itertools.product((False, True), repeat=2))


def _offset(part, buf):
    """Element offset of a view in its buffer; raises if it is a copy."""
    if isinstance(buf, torch.Tensor):
        assert part.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        return part.storage_offset()
    assert np.shares_memory(part, buf)
    return (part.__array_interface__["data"][0] - buf.__array_interface__["data"][0]) // 4


@pytest.mark.parametrize("emit,score", FLAGS)
@pytest.mark.parametrize("L", LENGTHS)
def test_split_conf_buffer_gives_views_at_the_headers_offsets(L, emit, score):
    """include/dmpfold_hip.h: L confidences | L*L map, 3 info floats ("emit_distmap") | 5L + 24 floats ("score_native")."""
    total = L + (L * L + 3 if emit else 0) + (5 * L + 24 if score else 0)
    assert S.conf_floats(L, emit, score) == total
    for buf in (np.arange(total + 7, dtype=np.float32), torch.arange(total + 7, dtype=torch.float32)):
        coords = object()
        out = S.split_conf_buffer(buf, L, emit, score, coords)
        assert out.coords is coords
        want = {"confs": (0, (L,))}
        if emit:
            want.update(distmap=(L, (L, L)), info=(L + L * L, (3,)))
        if score:
            want["score_block"] = (L + (L * L + 3 if emit else 0), (5 * L + 24,))
        for name in ("confs", "distmap", "info", "score_block"):
            part = getattr(out, name)
            if name not in want:
                assert part is None
                continue
            off, shape = want[name]
            assert tuple(part.shape) == shape and _offset(part, buf) == off, (name, L, emit, score)
            assert float(part.reshape(-1)[0]) == float(off) and float(part.reshape(-1)[-1]) == float(off + int(np.prod(shape)) - 1)
    with pytest.raises(ValueError):
        S.split_conf_buffer(np.zeros(total - 1, dtype=np.float32), L, emit, score)
    with pytest.raises(ValueError):
        S.split_conf_buffer(np.zeros((1, total), dtype=np.float32), L, emit, score)
    if emit and not score:                      # the older helper is the same split
        old = S.split_distmap_buffer(buf[:total], L)
        assert [_offset(p, buf) for p in old] == [0, L, L + L * L] and tuple(old[1].shape) == (L, L)


@pytest.mark.parametrize("emit,score", FLAGS)
@pytest.mark.parametrize("L", LENGTHS)
def test_public_tuples(L, emit, score):
    """Engine.predict: (coords, confs), with distmap=True (coords, confs, distmap, info), never the score block.
    Pipeline.result: (coords, confs[, distmap, info][, score block])."""
    buf = np.zeros(S.conf_floats(L, emit, score), dtype=np.float32)
    out = S.split_conf_buffer(buf, L, emit, score, "coords")
    for asked in (False, True):
        got = out.public(asked, score=False)
        assert isinstance(got, tuple) and len(got) == (4 if emit and asked else 2)
        assert got[0] == "coords" and got[1] is out.confs
        if emit and asked:
            assert got[2] is out.distmap and got[3] is out.info
    got = out.public()
    assert len(got) == 2 + (2 if emit else 0) + (1 if score else 0)
    assert got[:2] == ("coords", out.confs)
    if emit:
        assert got[2] is out.distmap and got[3] is out.info
    if score:
        assert got[-1] is out.score_block and tuple(got[-1].shape) == (5 * L + 24,)
    back = S.Outputs.of(got, emit, score)
    assert all(a is b for a, b in zip(back, out))


def test_names_stay_importable_from_predict():
    from dmpfold2_amd import predict as P
    assert P.distmap_floats is S.distmap_floats and P.split_distmap_buffer is S.split_distmap_buffer
    assert P.distmap_floats(82) == 82 + 82 * 82 + 3 and P.distmap_floats(82, False) == 82


class _Stub:
    """get_option / set_option of an engine, every call recorded."""

    def __init__(self, **options):
        self.options = {"recycle_tol_mA": 0, "emit_distmap": 0, "score_native": 0}
        self.options.update(options)
        self.sets = []

    def get_option(self, name):
        return self.options[name]

    def set_option(self, name, value):
        self.sets.append((name, value))
        self.options[name] = value


NATIVE = np.zeros((8, 3), dtype=np.float32)


@pytest.mark.parametrize("raises", [False, True])
def test_call_options_set_and_restore(raises):
    stub = _Stub(recycle_tol_mA=7)
    before = dict(stub.options)
    try:
        with Engine._call_options(stub, 0.25, Extras(True, NATIVE)):
            assert stub.options == {"recycle_tol_mA": 250, "emit_distmap": 1, "score_native": 1}
            if raises:
                raise KeyError("the body failed")
    except KeyError:
        assert raises
    assert stub.options == before
    assert sorted(stub.sets) == sorted([("recycle_tol_mA", 250), ("emit_distmap", 1), ("score_native", 1),
                                        ("recycle_tol_mA", 7), ("emit_distmap", 0), ("score_native", 0)])


def test_call_options_leave_what_was_set_by_hand():
    stub = _Stub(recycle_tol_mA=40, emit_distmap=1, score_native=1)
    with Engine._call_options(stub, None, Extras(True, NATIVE)):
        assert stub.options == {"recycle_tol_mA": 40, "emit_distmap": 1, "score_native": 1}
    assert stub.sets == [] and stub.options == {"recycle_tol_mA": 40, "emit_distmap": 1, "score_native": 1}
    with Engine._call_options(stub, None, Extras(False, None)):         # nothing asked for: nothing touched
        pass
    assert stub.sets == []


def test_call_options_reject_a_bad_tolerance_before_any_change():
    stub = _Stub()
    with pytest.raises(ValueError):
        with Engine._call_options(stub, -0.5, Extras(True, NATIVE)):
            raise AssertionError("the body ran")
    assert stub.sets == [] and stub.options == {"recycle_tol_mA": 0, "emit_distmap": 0, "score_native": 0}


# ---- all five extras of a call ------------------------------------------------------------------------------------------
ALL_OFF = {"recycle_tol_mA": 0, "emit_distmap": 0, "score_native": 0, "score_map": 0, "align_structure": 0,
           "search_structures": 0, "search_max_m": 0}
LIBRARY = S.Library.from_traces([np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32), np.zeros((3, 3), np.float32)])
EVERYTHING = Extras(True, NATIVE, np.zeros((6, 3), dtype=np.float32), LIBRARY, True)
# the order the options are set in: "search_max_m" before "search_structures" (the scratch is sized from it)
SET_ORDER = [("recycle_tol_mA", 250), ("emit_distmap", 1), ("score_map", 1), ("score_native", 1), ("align_structure", 1),
             ("search_max_m", 7), ("search_structures", 3)]


def _stub7(**options):
    stub = _Stub(**dict(ALL_OFF, **options))
    stub.max_L = 64
    return stub


@pytest.mark.parametrize("raises", [False, True])
def test_call_options_set_all_five_extras_in_order_and_restore_in_reverse(raises):
    stub = _stub7(recycle_tol_mA=7)
    before = dict(stub.options)
    try:
        with Engine._call_options(stub, 0.25, EVERYTHING):
            assert stub.sets == SET_ORDER
            assert stub.options == dict(SET_ORDER)
            if raises:
                raise KeyError("the body failed")
    except KeyError:
        assert raises
    assert stub.options == before
    assert stub.sets == SET_ORDER + [(name, before[name]) for name, _ in reversed(SET_ORDER)]


def test_call_options_touch_nothing_that_was_set_by_hand():
    by_hand = {"recycle_tol_mA": 40, "emit_distmap": 1, "score_native": 1, "score_map": 1, "align_structure": 1,
               "search_structures": 3, "search_max_m": 9}
    stub = _stub7(**by_hand)
    with Engine._call_options(stub, None, EVERYTHING):
        assert stub.options == by_hand
    assert stub.sets == [] and stub.options == by_hand
    # one of them by hand: the others are set and restored around it
    stub = _stub7(score_native=1)
    with Engine._call_options(stub, None, EVERYTHING):
        assert stub.sets == [s for s in SET_ORDER[1:] if s[0] != "score_native"]
    assert stub.options == dict(ALL_OFF, score_native=1) and len(stub.sets) == 10


@pytest.mark.parametrize("extras", [Extras(True, None, None, None, True),                                   # score_map without a native
                                    EVERYTHING._replace(structure=np.zeros((5, 2), dtype=np.float32)),      # a structure of shape (5, 2)
                                    EVERYTHING._replace(library=S.Library.from_traces([np.zeros((65, 3), np.float32)]))])
def test_call_options_reject_bad_extras_before_any_change(extras):
    stub = _stub7()
    with pytest.raises(ValueError):
        with Engine._call_options(stub, 0.25, extras):
            raise AssertionError("the body ran")
    assert stub.sets == [] and stub.options == ALL_OFF
    if extras.native is None:                   # an engine whose "score_native" is on by hand needs no native for score_map
        stub = _stub7(score_native=1)
        with Engine._call_options(stub, None, extras):
            assert stub.options == dict(ALL_OFF, score_native=1, emit_distmap=1, score_map=1)
        assert stub.options == dict(ALL_OFF, score_native=1)


# ---- the agreement of a pipeline's engines ------------------------------------------------------------------------------
def _submit_before_the_rule(rows):
    """The specification: the flags block of Pipeline.submit as it stood before `agree_options`, its four conditions
    transcribed literally.  -> (emit, emit_alloc, score, smap, align, search), or RuntimeError."""
    flags = [bool(r[0]) for r in rows]
    emit = all(flags)
    sflags = [bool(r[1]) for r in rows]
    score = all(sflags)
    if any(sflags) and not (score and emit == any(flags)):
        raise RuntimeError("score_native")
    mflags = [bool(r[2]) for r in rows]
    smap = all(mflags)
    if any(mflags) and not (smap and emit and score):
        raise RuntimeError("score_map")
    aflags = [bool(r[3]) for r in rows]
    align = all(aflags)
    if any(aflags) and not (align and emit == any(flags) and score == any(sflags)):
        raise RuntimeError("align_structure")
    kflags = [r[4] for r in rows]
    search = kflags[0]
    if any(kflags) and not (all(k == search for k in kflags) and emit == any(flags) and score == any(sflags)
                            and align == any(aflags)):
        raise RuntimeError("search_structures")
    return emit, any(flags), score, smap, align, search


STATES = [bits + (k,) for bits in itertools.product((0, 1), repeat=4) for k in (0, 3)]


def _same_as_before(rows):
    try:
        want = _submit_before_the_rule(rows)
    except RuntimeError:
        with pytest.raises(RuntimeError) as err:
            agree_options(rows)
        for name in ("emit_distmap", "score_native", "score_map", "align_structure", "search_structures",
                     "set_distmap", "set_score", "set_score_map", "set_align", "set_search"):
            assert name in str(err.value)
        return False
    got = agree_options(rows)
    assert tuple(got[:6]) == want and got.max_L is None, rows
    assert [type(v) for v in got[:6]] == [bool, bool, bool, bool, bool, int]
    return True


def test_agree_options_is_the_four_checks_it_replaced():
    assert len(STATES) == 32
    passed = sum(_same_as_before([a, b]) for a in STATES for b in STATES)
    # 32 pairs of equal states less the 12 with "score_map" on and not both of its needs, and the 2 pairs that differ in
    # "emit_distmap" alone
    assert passed == 32 - 12 + 2
    assert agree_options(iter([(1, 0, 0, 0, 0), (0, 0, 0, 0, 0)]))[:2] == (False, True)


def test_agree_options_three_engines_the_odd_one_last():
    for state in STATES:
        for odd in STATES:
            _same_as_before([state, state, odd])
    assert _same_as_before([(1, 1, 1, 1, 3)] * 3) and not _same_as_before([(1, 1, 1, 1, 3)] * 2 + [(1, 1, 1, 1, 2)])
    assert not _same_as_before([(0, 0, 0, 0, 0)] * 2 + [(0, 0, 0, 1, 0)])
    assert agree_options([(1, 0, 0, 0, 0)] * 2 + [(0, 0, 0, 0, 0)])[:2] == (False, True)


# ---- Outputs.public / Outputs.of ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("present", list(itertools.product((False, True), repeat=5)))
def test_public_and_of_round_trip(present):
    """All 32 presence combinations of (distmap + info, score, align, search, map): `of` undoes `public`, every field the
    same object; the map-score block is the tuple's last though it lies behind the score block in the buffer."""
    distmap, score, align, search, smap = present
    parts = {name: object() for name in S.Outputs._fields}
    out = S.Outputs(parts["coords"], parts["confs"], parts["distmap"] if distmap else None, parts["info"] if distmap else None,
                    parts["score_block"] if score else None, parts["align_block"] if align else None,
                    parts["search_block"] if search else None, parts["map_block"] if smap else None)
    pub = out.public()
    assert len(pub) == 2 + 2 * distmap + score + align + search + smap
    order = ["coords", "confs"] + ["distmap", "info"] * distmap + ["score_block"] * score + ["align_block"] * align \
        + ["search_block"] * search + ["map_block"] * smap
    assert all(got is parts[name] for got, name in zip(pub, order))
    if smap:
        assert pub[-1] is out.map_block
    back = S.Outputs.of(pub, distmap, score, align, search, smap)
    assert all(a is b for a, b in zip(back, out))
    # what a call of an Engine returns: coords, confs, and the map only if asked - the keyword form says the same
    for asked in (False, True):
        plain = out.public(asked, blocks=False)
        assert len(plain) == (4 if asked and distmap else 2) and all(a is b for a, b in zip(plain, pub))
        spelt = out.public(asked, score=False, align=False, search=False, score_map=False)
        assert len(spelt) == len(plain) and all(a is b for a, b in zip(spelt, plain))
