#!/usr/bin/env python
"""Record what the module-level layout functions of dmpfold2_amd/score.py give, as tests/golden/conf_layout.json.

    python tools/record_conf_layout.py [--full] [OUT.json]

Run it on the commit whose answers are to be kept; tests/test_layout_cpu.py then holds every later commit to them.  It
calls nothing but conf_floats, score_offset, mapscore_offset, align_offset, search_offset and split_conf_buffer, with
positional arguments in the order they have had since "score_map" went in.  No GPU, no library.

Grid: L x (distmap, score, score_map) x align_m x max_L x search.  align_m "max_L" and "max_L+1" mean the row's max_L, and
2048 (DMP_MAX_L) where that is None; "nan" is a NaN.  The default grid is the thinned one (L 8 and 2048; align_m None, 3,
max_L + 1, NaN), 576 rows; --full takes L 8, 9, 82, 2048 and align_m None, 0, 2, 3, 61, max_L, max_L + 1, 2.5, NaN.

A row is [L, distmap, score, score_map, align_m, max_L, search, conf_floats, score_offset, mapscore_offset, align_offset,
search_offset, views]: `views` = [[field, offset, length] ...] of every non-None view split_conf_buffer returns on an
arange buffer of exactly the floats it asks for (an offset is the view's first element).  null in the place of a number or
of `views` = that call raised ValueError: the functions that size an align block reject an align_m that is no number
(conf_floats and split_conf_buffer with NaN; search_offset too where max_L is None), while search_offset with a max_L
counts such a block as m' = 0.  Nothing else on the grid is rejected.  mapscore_offset takes no score_map and
split_conf_buffer nothing it is not given: each row records the calls as a caller with these settings would make them."""
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dmpfold2_amd import score as S          # noqa: E402

FIELDS = ("confs", "distmap", "info", "score_block", "align_block", "search_block", "map_block")
SEARCHES = (None, (1, 3), (3, 120))
MAX_LS = (None, 64, 2048)


def align_values(full):
    return (None, 0, 2, 3, 61, "max_L", "max_L+1", 2.5, "nan") if full else (None, 3, "max_L+1", "nan")


def resolve(align_m, max_L):
    """The grid's name of an align_m -> the value handed to the functions."""
    cap = 2048 if max_L is None else max_L
    return {"max_L": cap, "max_L+1": cap + 1, "nan": float("nan")}.get(align_m, align_m) if isinstance(align_m, str) else align_m


def or_none(fn, *args):
    try:
        return fn(*args)
    except ValueError:
        return None


def views(L, distmap, score, score_map, m, max_L, search):
    """[[field, offset, length]] of split_conf_buffer on an arange buffer just long enough, None if it raises."""
    need = or_none(S.conf_floats, L, distmap, score, m, score_map)
    if need is None:
        return None
    triple = None
    if search is not None:
        triple = (search[0], search[1], max_L)
        need = max(need, S.search_offset(L, distmap, score, m, max_L, score_map) + S.search_floats(L, *search))
    buf = np.arange(need, dtype=np.float64)          # float64: every index up to 2048^2 + ... is exact
    out = S.split_conf_buffer(buf, L, distmap, score, None, m, triple, score_map)
    return [[name, int(part.reshape(-1)[0]) if part.size else None, int(part.size)]
            for name, part in ((f, getattr(out, f)) for f in FIELDS) if part is not None]


def rows(full=False):
    lengths = (8, 9, 82, 2048) if full else (8, 2048)
    for L, (distmap, score, score_map), align_m, max_L, search in itertools.product(
            lengths, itertools.product((False, True), repeat=3), align_values(full), MAX_LS, SEARCHES):
        m = resolve(align_m, max_L)
        yield [L, distmap, score, score_map, align_m, max_L, search,
               or_none(S.conf_floats, L, distmap, score, m, score_map), S.score_offset(L, distmap),
               S.mapscore_offset(L, distmap, score), S.align_offset(L, distmap, score, score_map),
               or_none(S.search_offset, L, distmap, score, m, max_L, score_map),
               views(L, distmap, score, score_map, m, max_L, search)]


def main(argv):
    full = "--full" in argv
    paths = [a for a in argv if not a.startswith("--")]
    out = paths[0] if paths else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "conf_layout.json")
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows(full)) + "\n]\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
