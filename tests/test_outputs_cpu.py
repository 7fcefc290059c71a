"""The one Python description of the `d_conf` buffer (score.split_conf_buffer, score.Outputs) and the per-call options of
an engine (Engine._call_options).  No GPU."""
import itertools

import numpy as np
import pytest
import torch

from dmpfold2_amd import score as S
from dmpfold2_amd.predict import Engine

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
        with Engine._call_options(stub, 0.25, True, NATIVE):
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
    with Engine._call_options(stub, None, True, NATIVE):
        assert stub.options == {"recycle_tol_mA": 40, "emit_distmap": 1, "score_native": 1}
    assert stub.sets == [] and stub.options == {"recycle_tol_mA": 40, "emit_distmap": 1, "score_native": 1}
    with Engine._call_options(stub, None, False, None):         # nothing asked for: nothing touched
        pass
    assert stub.sets == []


def test_call_options_reject_a_bad_tolerance_before_any_change():
    stub = _Stub()
    with pytest.raises(ValueError):
        with Engine._call_options(stub, -0.5, True, NATIVE):
            raise AssertionError("the body ran")
    assert stub.sets == [] and stub.options == {"recycle_tol_mA": 0, "emit_distmap": 0, "score_native": 0}
