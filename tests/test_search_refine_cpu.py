"""Option "search_refine" without a GPU: the condition on the inputs of the selection tests (tests/search_refine_ref.py has
the screen's yardstick and the library of 16), and the host side - `score.Library.refine`, `unpack_search` / `hits_json` with
and without it, the two front ends' flag, and that the C ABI did not grow."""
import numpy as np
import pytest

from dmpfold2_amd import score as S
from search_refine_ref import RELATED, input_condition, library_traces, screen_yardstick
from test_align_cpu import NEAR_TIE, random_walk, yardstick


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("L", [33, 64])
def test_the_library_separates_related_from_unrelated(L):
    """A condition on the inputs, not a measurement: the four related entries are the four best by the screen and by the
    whole definition alike, the fourth and fifth screened tm_model lie 0.05 apart, and no decision is a near tie."""
    model = random_walk(L, 1)
    traces = library_traces(model)
    assert len(traces) == 16 and [len(t) for t in traces[:4]] == [L, L - max(4, L // 12) + 7, L + 5, max(L - 3, 3)]
    tm, margins, problems = input_condition(model, traces, full=True)
    print(f"L={L}: screened tm_model", np.round(tm, 4).tolist(), "smallest margin", float(margins.min()))
    assert not problems, problems
    assert sorted(S.host_rank(tm)[:4].tolist()) == list(RELATED)
    assert margins.min() >= NEAR_TIE


def test_the_screen_is_a_lower_bound_and_a_rigid_copy_screens_whole():
    model = random_walk(40, 3)
    traces = library_traces(model)
    rigid, _ = screen_yardstick(model, traces[0])
    assert rigid["n_ali"] == 40 and abs(rigid["tm_model"] - 1.0) <= 1e-6 and np.array_equal(rigid["ali"], np.arange(40))
    assert rigid["seed_offset"] == 0 and abs(rigid["tm_struct"] - 1.0) <= 1e-6 and rigid["rmsd_ali"] <= 1e-4
    for k in (1, 5):
        got, _ = screen_yardstick(model, traces[k])
        full, _ = yardstick(model, traces[k])
        assert got["tm_model"] <= full["tm_model"] + 1e-12, k
        assert got["seeds"] == full["seeds"] and (got["ali"] >= 0).sum() == got["n_ali"]
        gaps = np.diff(got["ali"][got["ali"] >= 0])
        assert (gaps == 1).all(), "a screened alignment is gapless"


# ------------------------------------------------------------------------------------------------ the host side
def _lib(K=5):
    return S.Library.from_traces([random_walk(4 + k, 10 + k) for k in range(K)], [f"d{k}" for k in range(K)])


def test_library_refine_is_validated(tmp_path):
    lib = _lib()
    assert lib.refine == 0
    lib.refine = 3
    assert lib.refine == 3
    lib.refine = S.SEARCH_MAX
    for bad in (-1, S.SEARCH_MAX + 1, 2.5, True, "3"):
        with pytest.raises((ValueError, TypeError)):
            lib.refine = bad
    assert lib.refine == S.SEARCH_MAX
    lib.save(str(tmp_path / "lib.npz"))
    assert S.Library.open(str(tmp_path / "lib.npz")).refine == 0
    assert S.Library.open(str(tmp_path / "lib.npz"), refine=2).refine == 2
    with pytest.raises(ValueError, match="refine"):
        S.Library.open(str(tmp_path / "lib.npz"), refine=-2)
    assert S.Library(lib.names, lib.lengths, lib.ca, refine=4).refine == 4


def _answered(lib, L, screened):
    """A search block as the library would answer it: entry k's tm_model 0.1 (k + 1), offset 21 = 1 for the `screened`."""
    K = len(lib)
    block = S.pack_library(lib, L)
    for k in range(K):
        block[2 * K + 24 * k:2 * K + 24 * (k + 1)] = 0.0
        block[2 * K + 24 * k + 2] = 0.1 * (k + 1)
        block[2 * K + 24 * k + 20] = 1.0 if k in screened else 0.0
    block[K:2 * K] = np.arange(K)[::-1]
    return block


def test_unpack_and_json_with_and_without_refine():
    L, lib = 9, _lib()
    K = len(lib)
    block = _answered(lib, L, screened=(0, 1, 2))
    plain = S.unpack_search(block, L, lib.lengths)
    assert sorted(plain) == ["hits", "rank"]
    for same in (0, K, K + 1):                           # off, or nothing to choose: today's keys
        assert sorted(S.unpack_search(block, L, lib.lengths, refine=same)) == ["hits", "rank"]
    un = S.unpack_search(block, L, lib.lengths, refine=2)
    assert sorted(un) == ["hits", "rank", "refined"]
    assert un["refined"].dtype == np.bool_ and un["refined"].tolist() == [False, False, False, True, True]
    assert un["rank"].tolist() == plain["rank"].tolist() == [4, 3, 2, 1, 0]
    js0 = S.hits_json(plain, lib.names, top=3)
    assert sorted(js0) == ["entries", "hits"]
    assert sorted(js0["hits"][0]) == ["R", "index", "n_ali", "name", "rmsd_ali", "t", "tm_model", "tm_struct"]
    assert S.hits_json(un, lib.names, top=3) == js0, "without `refine` the dict is unchanged"
    js = S.hits_json(un, lib.names, top=3, refine=2)
    assert list(js) == ["entries", "refine", "hits"] and js["refine"] == 2 and js["entries"] == K
    assert [(h["index"], h["refined"]) for h in js["hits"]] == [(4, True), (3, True), (2, False)]
    assert [{k: v for k, v in h.items() if k != "refined"} for h in js["hits"]] == js0["hits"]
    # a block the library answered with NaN: nothing is refined
    nan = S.unpack_search(S.pack_library(lib, L), L, lib.lengths, refine=2)
    assert not nan["refined"].any()
    # the row of BLOCKS passes the library's refine through
    row = S.BLOCK["search"]
    assert sorted(row.unpack(block, L, library=lib)) == ["hits", "names", "rank"]
    assert row.json(row.unpack(block, L, library=lib), top=3) == js0
    lib.refine = 2
    hits = row.unpack(block, L, library=lib)
    assert sorted(hits) == ["hits", "names", "rank", "refine", "refined"] and hits["refine"] == 2
    assert row.json(hits, top=3) == js


def test_the_front_ends_take_the_flag_with_its_partner_only(capsys):
    from dmpfold2_amd import batch
    from dmpfold2_amd import predict as P
    args = P.dmpfold_parser().parse_args(["-i", "x.aln", "--search", "lib.npz", "--search-refine", "4"])
    assert args.search_refine == 4 and args.search == "lib.npz"
    assert not hasattr(P.dmpfold_parser().parse_args(["-i", "x.aln"]), "search_refine")
    args = batch.batch_parser().parse_args(["-o", "out", "--library", "lib.npz", "--search-refine", "7"])
    assert args.search_refine == 7 and args.library == "lib.npz"
    for run, argv, partner in ((P.run_dmpfold, ["-i", "x.aln", "--search-refine", "4"], "--search"),
                               (batch.main, ["-o", "out", "-i", "x.aln", "--search-refine", "4"], "--library"),
                               (P.run_dmpfold, ["-i", "x.aln", "--search", "lib.npz", "--search-refine", "-1"], "0 or 1 .. 4096"),
                               (batch.main, ["-o", "out", "-i", "x.aln", "--library", "lib.npz", "--search-refine", "4097"],
                                "0 or 1 .. 4096")):
        with pytest.raises(SystemExit) as stop:
            run(argv)
        assert stop.value.code == 2
        assert partner in capsys.readouterr().err


def test_the_c_abi_did_not_grow():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5
