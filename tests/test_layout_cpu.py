"""score.Layout, the one Python description of the `d_conf` buffer, against tests/golden/conf_layout.json: what the six
positional layout functions gave on the commit before `Layout` existed (tools/record_conf_layout.py wrote the file there and
explains its rows).  Every row is asked of the functions that stayed and of a `Layout` directly.  No GPU, no library."""
import importlib.util
import json
import os

import numpy as np
import pytest

from dmpfold2_amd import score as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "conf_layout.json")) as _fh:
    ROWS = json.load(_fh)

_spec = importlib.util.spec_from_file_location("record_conf_layout", os.path.join(ROOT, "tools", "record_conf_layout.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)


def _views(out):
    return [[f, int(getattr(out, f).reshape(-1)[0]), int(getattr(out, f).size)] for f in REC.FIELDS if getattr(out, f) is not None]


def test_the_grid_is_the_recorders():
    """576 rows: L (8, 2048) x 8 flag triples x align_m (None, 3, max_L + 1, NaN) x max_L (None, 64, 2048) x 3 searches."""
    assert len(ROWS) == 2 * 8 * 4 * 3 * 3
    keys = {json.dumps(r[:7]) for r in ROWS}
    assert len(keys) == len(ROWS) and {r[0] for r in ROWS} == {8, 2048} and {r[4] for r in ROWS} == {None, 3, "max_L+1", "nan"}
    # what the parent rejected, and nothing else: an align block whose m is no number cannot be sized
    for r in ROWS:
        nan = r[4] == "nan"
        assert (r[7] is None) == nan and (r[12] is None) == nan and (r[11] is None) == (nan and r[5] is None), r[:7]


def test_the_module_functions_reproduce_every_row():
    bufs = {}
    for L, distmap, score, score_map, align_m, max_L, search, floats, s0, m0, a0, b0, views in ROWS:
        m = REC.resolve(align_m, max_L)
        row = (L, distmap, score, score_map, align_m, max_L, search)
        if floats is None:
            with pytest.raises(ValueError):
                S.conf_floats(L, distmap, score, m, score_map)
        else:
            assert S.conf_floats(L, distmap, score, m, score_map) == floats, row
        assert S.score_offset(L, distmap) == s0 and S.mapscore_offset(L, distmap, score) == m0, row
        assert S.align_offset(L, distmap, score, score_map) == a0, row
        if b0 is None:
            with pytest.raises(ValueError):
                S.search_offset(L, distmap, score, m, max_L, score_map)
        else:
            assert S.search_offset(L, distmap, score, m, max_L, score_map) == b0, row
        triple = None if search is None else (search[0], search[1], max_L)
        if views is None:
            with pytest.raises(ValueError):
                S.split_conf_buffer(np.zeros(1 << 10), L, distmap, score, None, m, triple, score_map)
            continue
        need = max(end for end in (o + n for _, o, n in views))
        buf = bufs.setdefault(need, np.arange(need, dtype=np.float64))
        assert _views(S.split_conf_buffer(buf, L, distmap, score, None, m, triple, score_map)) == views, row
        with pytest.raises(ValueError):
            S.split_conf_buffer(buf[:-1], L, distmap, score, None, m, triple, score_map)


def test_a_layout_reproduces_every_row():
    bufs = {}
    for L, distmap, score, score_map, align_m, max_L, search, floats, s0, m0, a0, b0, views in ROWS:
        row = (L, distmap, score, score_map, align_m, max_L, search)
        lay = S.Layout(L, distmap=distmap, score=score, score_map=score_map, align_m=REC.resolve(align_m, max_L), search=search,
                       max_L=max_L)
        # (score_offset, mapscore_offset and align_offset were asked without what lies behind them: so is the layout)
        assert (lay.score_off, lay.align_off) == (s0, a0), row
        assert lay._replace(score_map=False).mapscore_off == m0 == lay.mapscore_off, row
        if b0 is None:
            with pytest.raises(ValueError):
                lay.search_off
        else:
            assert lay.search_off == b0, row
        if floats is None:
            with pytest.raises(ValueError):
                lay.total
            with pytest.raises(ValueError):
                lay.split(np.zeros(1 << 10))
            continue
        assert lay._replace(search=None).total == floats == lay.align_end, row
        need = max(end for end in (o + n for _, o, n in views))
        assert lay.total == need, row
        buf = bufs.setdefault(need, np.arange(need, dtype=np.float64))
        assert _views(lay.split(buf)) == views, row
        with pytest.raises(ValueError):
            lay.split(buf[:-1])
        with pytest.raises(ValueError):
            lay.split(buf.reshape(1, -1))


def test_layout_is_a_value():
    a, b = S.Layout(82, True, True, align_m=61), S.Layout(82.0, 1, 1, 0, 61)
    assert a == b and hash(a) == hash(b) and a.search is None and a.L == 82 and a.distmap is True
    with pytest.raises(AttributeError):
        a.L = 9
    # the allocation of a pipeline whose engines disagree on "emit_distmap" alone: the larger of two layouts
    assert max(S.Layout(82).total, S.Layout(82, True).total) == 82 + 82 * 82 + 3 and S.Layout(82).split(np.zeros(9000)).distmap is None
