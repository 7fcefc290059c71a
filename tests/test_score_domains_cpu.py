"""Option "score_domains" without a GPU: the layout, the host helpers of dmpfold2_amd/score.py, both parsers, the engine's call
options on a recording stub, and the restatement of the definition (tests/score_domains_ref.py: mask the native by label,
test_score_cpu.yardstick, scatter, the outer counts as integer loops) on constructed two-domain traces whose domains are perfect
and whose arrangement is wrong.  On the parent commit none of these names exist."""
import itertools
import json

import numpy as np
import pytest

import domains_ref as R
import score_domains_ref as DR
from dmpfold2_amd import score as S
from test_score_cpu import NEAR_TIE, yardstick


# ------------------------------------------------------------------------------------------------ layout
def test_layout_for_every_combination_of_the_neighbouring_options():
    L, K, M = 33, 5, 120
    n = S.domain_score_floats(L)
    assert n == 16 + 2 * 16 * 32 + 4 * L == 1040 + 4 * L
    for distmap, ss, exposure, align_m, passes, search, search_domains in itertools.product(
            (False, True), (False, True), (False, True), (None, 40), (None, 3), (None, (K, M)), (False, True)):
        kw = dict(distmap=distmap, score=True, score_map=distmap, align_m=align_m, search=search, max_L=64, passes=passes, ss=ss,
                  exposure=exposure, domains=True, search_domains=search_domains)
        off, on = S.Layout(L, **kw), S.Layout(L, score_domains=True, **kw)
        # in front of the block nothing moves; behind it everything moves by its size
        for name in ("info_off", "score_off", "mapscore_off", "pass_off", "ss_off", "exposure_off", "domains_off", "domain_search_off",
                     "domain_score_off"):
            assert getattr(on, name) == getattr(off, name), name
        assert on.domain_score_off == off.domain_search_off + off.floats(S.DOMAIN_SEARCH) == off.align_off
        for name in ("align_off", "align_end", "search_off", "total") + (("search_end",) if search else ()):
            assert getattr(on, name) == getattr(off, name) + n, name
        buf = np.arange(on.total, dtype=np.float64)
        out = on.split(buf)
        assert out.domain_score_block.shape == (n,) and out.domain_score_block[0] == on.domain_score_off
        assert on.domain_score_block(buf)[0] == on.domain_score_off and off.domain_score_block(buf) is None
        assert off.split(buf[:off.total]).domain_score_block is None
        if search and search_domains:
            assert out.domain_search_block[-1] == on.domain_score_off - 1
        else:
            assert out.domains_block[-1] == on.domain_score_off - 1
        if align_m is not None:
            assert out.align_block[0] == on.domain_score_off + n
        # `public` never hands the block out, `_replace` keeps it
        assert all(x is not out.domain_score_block for x in out.public())
        assert out._replace(coords=None).domain_score_block is out.domain_score_block
        assert on._replace(L=L).score_domains and not off._replace(L=L).score_domains


def test_offsets_with_the_attribute_off_are_todays():
    """The recorded layouts (tests/golden/conf_layout.json, tests/golden/host_plumbing.json.gz) know nothing of the option: with
    the attribute off every offset is what it was, and no field, row or positional part was added."""
    for L in (8, 300):
        for search in (None, (3, 40)):
            base = S.Layout(L, True, True, True, 65, search, 64, passes=2, ss=True, exposure=True, domains=True, search_domains=True)
            same = base._replace(score_domains=False)
            for name in ("domains_off", "domain_search_off", "align_off", "align_end", "search_off", "total"):
                assert getattr(base, name) == getattr(same, name)
            assert base.domain_score_off == base.align_off
    assert S.Layout(40).score_domains is False and S.Layout._make(S.Layout(40)).score_domains is False
    assert "score_domains" not in S.Layout._fields and [r.key for r in S.BLOCKS][-3:] == ["domains", "align", "search"]
    assert S.DOMAIN_SCORES not in S.BLOCKS and S.DOMAIN_SCORES.option == "score_domains" and S.DOMAIN_SCORES.field == "domain_score_block"
    assert "domain_score_block" not in S.Outputs._fields and len(S.Outputs._fields) == 11


# ------------------------------------------------------------------------------------------------ pack, unpack, JSON
def _made_up(L, D0, D1, seed=0):
    rng = np.random.default_rng(seed)
    header = np.zeros(16, dtype=np.float32)
    header[:3] = [D0, D1, L - 1]
    table = np.full((2, 16, 32), np.nan, dtype=np.float32)
    for leg, D in enumerate((D0, D1)):
        table[leg, :D] = rng.uniform(0.1, 0.9, size=(D, 32)).astype(np.float32)
        table[leg, :D, 0] = table[leg, :D, 1] = rng.integers(3, 9, size=D)
        table[leg, :D, 7:12] = rng.integers(0, 9, size=(D, 5))
        table[leg, :D, 24:28] = rng.integers(1, 400, size=(D, 4))
        table[leg, :D, 28] = table[leg, :D, 0] + 1
        table[leg, :D, 29:] = 0
    res = rng.uniform(0, 1, size=(4, L)).astype(np.float32)
    res[:, 3] = np.nan
    if not D1:
        res[2:] = np.nan
    return header, table, res


def test_pack_and_unpack_round_trip():
    L = 21
    header, table, res = _made_up(L, 3, 2)
    block = S.pack_domain_scores(L, header, table, res)
    assert block.dtype == np.float32 and block.shape == (S.domain_score_floats(L),)
    un = S.unpack_domain_scores(block, L)
    assert un["domains"] == 3 and un["domains_native"] == 2 and un["present"] == L - 1 and len(un["legs"]) == 2
    for name, part in (("header", header), ("table", table), ("res", res)):
        assert np.array_equal(un[name].view(np.uint32), part.view(np.uint32)), name
    again = S.pack_domain_scores(L, un["header"], un["table"], un["res"])
    assert np.array_equal(again.view(np.uint32), block.view(np.uint32))
    row, h = un["legs"][1]["rows"][1], table[1, 1]
    assert row["n"] == int(h[0]) and row["n_pairs"] == int(h[1]) and row["size"] == int(h[28])
    assert [row[k] for k in S.SCORE_NAMES[1:]] == [float(v) for v in h[2:7]] and row["counts"] == [int(v) for v in h[7:12]]
    assert np.array_equal(row["R"], h[12:21].reshape(3, 3)) and np.array_equal(row["t"], h[21:24])
    assert [row[k] for k in ("preserved", "pairs", "outer_preserved", "outer_pairs")] == [int(v) for v in h[24:28]]
    leg = un["legs"][0]
    rows = leg["rows"]
    assert leg["tm_domains"] == sum(r["size"] * r["tm"] for r in rows) / sum(r["size"] for r in rows)
    assert leg["lddt_intra"] == sum(r["preserved"] for r in rows) / (4.0 * sum(r["pairs"] for r in rows))
    assert leg["lddt_inter"] == sum(r["outer_preserved"] for r in rows) / (4.0 * sum(r["outer_pairs"] for r in rows))
    assert np.array_equal(leg["lddt_res"], res[0], equal_nan=True) and np.array_equal(un["legs"][1]["deviation"], res[3], equal_nan=True)
    # a starved domain (n < 3: NaN scores, counts given) weighs nothing in tm_domains
    table[0, 2, 0:2] = 2
    table[0, 2, 2:24] = np.nan
    un2 = S.unpack_domain_scores(S.pack_domain_scores(L, header, table, res), L)
    rows = un2["legs"][0]["rows"]
    assert np.isnan(rows[2]["tm"]) and rows[2]["counts"] == [0] * 5 and rows[2]["pairs"] == int(table[0, 2, 25])
    assert un2["legs"][0]["tm_domains"] == sum(r["size"] * r["tm"] for r in rows[:2]) / sum(r["size"] for r in rows[:2])
    # without the native's leg
    header1, table1, res1 = _made_up(L, 2, 0, seed=1)
    un1 = S.unpack_domain_scores(S.pack_domain_scores(L, header1, table1, res1), L)
    assert un1["domains_native"] == 0 and len(un1["legs"]) == 1 and np.isnan(un1["table"][1]).all()
    # a NaN block: invalid labels, a latched fault
    nan = S.pack_domain_scores(L)
    assert np.isnan(nan).all()
    un0 = S.unpack_domain_scores(nan, L)
    assert un0["domains"] == 0 and un0["legs"] == [] and un0["present"] == 0
    assert S.domain_scores_json(un0) == {"domains": 0, "domains_native": 0, "present": 0}
    with pytest.raises(ValueError, match="domain-score block"):
        S.unpack_domain_scores(block[:-1], L)


def test_json_form():
    L = 21
    header, table, res = _made_up(L, 3, 2, seed=2)
    table[0, 1, 2] = np.nan
    labels = np.repeat([0, 1, 2, 0], [5, 6, 7, 3])
    native_labels = np.repeat([0, 1], [10, 11])
    parse = {"table": [{"size": int((labels == d).sum()), "segment_list": S._segments(labels, d)} for d in range(3)],
             "native": {"table": [{"size": int((native_labels == d).sum()), "segment_list": S._segments(native_labels, d)} for d in range(2)]}}
    un = S.unpack_domain_scores(S.pack_domain_scores(L, header, table, res), L)
    js = S.domain_scores_json(un, parse)
    assert js["domains"] == 3 and js["domains_native"] == 2 and js["present"] == L - 1 and set(js) == {"domains", "domains_native", "present", "model", "native"}
    assert [r["domain"] for r in js["model"]["rows"]] == [0, 1, 2] and js["model"]["rows"][0]["segments"] == [[0, 4], [18, 20]]
    assert js["native"]["rows"][1]["segments"] == [[10, 20]] and js["model"]["rows"][1]["rmsd"] is None
    assert set(js["model"]["rows"][0]) == {"domain", "size", "n", "segments", "rmsd", "tm", "gdt_ts", "gdt_ha", "lddt", "counts",
                                          "preserved", "pairs", "outer_preserved", "outer_pairs"}
    assert js["model"]["rows"][2]["tm"] == float(table[0, 2, 3]) and js["native"]["lddt_inter"] == un["legs"][1]["lddt_inter"]
    plain = S.domain_scores_json(un)
    assert "segments" not in plain["model"]["rows"][0]
    json.dumps(js)
    assert S.DOMAIN_SCORES.json(un, domains=parse) == js and S.DOMAIN_SCORES.floats(L, True) == S.domain_score_floats(L)
    assert S.DOMAIN_SCORES.unpack(S.pack_domain_scores(L, header, table, res), L)["domains"] == 3


# ------------------------------------------------------------------------------------------------ the host layers
def test_parsers_accept_the_flags_and_hide_them():
    from dmpfold2_amd import batch
    from dmpfold2_amd.predict import dmpfold_parser
    for make, empty, with_native in ((dmpfold_parser, ["-i", "x.aln"], ["--native", "x.pdb"]),
                                     (batch.batch_parser, ["-o", "out"], ["--natives", "dir"])):
        assert "score-domains" not in make().format_help() and "score_domains" not in make().format_help()
        assert not hasattr(make().parse_args(empty), "score_domains")
        assert make().parse_args(empty + with_native + ["--score-domains"]).score_domains is True


def test_parser_errors_name_the_flag(capsys):
    from dmpfold2_amd import batch
    from dmpfold2_amd.predict import run_dmpfold
    with pytest.raises(SystemExit) as exc:
        run_dmpfold(["-i", "x.aln", "--score-domains"])
    assert exc.value.code == 2 and "--score-domains needs --native" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        batch.main(["-i", "x.aln", "-o", "out", "--score-domains"])
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "--score-domains needs --natives" in err


def test_run_batch_needs_natives(tmp_path):
    from dmpfold2_amd import batch
    with batch.batch_score_domains():
        with pytest.raises(ValueError, match="give `natives`"):
            batch.run_batch([], str(tmp_path / "out"))
    assert batch._SCORE_DOMAINS is False


def test_the_abi_stays():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5


class _Stub:
    """A recording stand-in for an Engine (as tests/test_search_domains_cpu.py has it)."""
    max_L = 64

    def __init__(self):
        from dmpfold2_amd.predict import Engine
        self.options, self.calls = {}, []
        self._call = Engine._call_options.__get__(self)
        self.set_score_domains = Engine.set_score_domains.__get__(self)
        self.with_score_domains = Engine.with_score_domains.__get__(self)
        self._score_domains = False

    def get_option(self, name):
        return self.options.get(name, 0)

    def set_option(self, name, value):
        self.options[name] = value
        self.calls.append((name, value))


def test_call_options_turn_domains_on_and_put_it_back():
    from dmpfold2_amd.predict import Extras
    native = np.zeros((20, 3), dtype=np.float32)
    stub = _Stub()
    with stub._call(None, Extras(native=native)):
        assert "score_domains" not in stub.options and "domains" not in stub.options
    stub = _Stub()
    with stub.with_score_domains():
        with stub._call(None, Extras(native=native)):
            assert stub.options == {"score_native": 1, "domains": 1, "score_domains": 1}
            assert stub.calls == [("score_native", 1), ("domains", 1), ("score_domains", 1)], "an option behind what it needs"
        assert all(stub.options[k] == 0 for k in ("score_domains", "domains", "score_native"))
        assert stub.calls[3:] == [("score_domains", 0), ("domains", 0), ("score_native", 0)]
    assert stub._score_domains is False
    stub = _Stub()
    stub.options["domains"] = 1                              # set by hand (set_domains): it stays
    stub.set_score_domains(True)
    with stub._call(None, Extras(native=native)):
        assert ("domains", 1) not in stub.calls and stub.options["score_domains"] == 1
    assert stub.options["domains"] == 1 and stub.options["score_domains"] == 0
    # without a native: as score_map without one, before anything changes
    stub = _Stub()
    stub.set_score_domains(True)
    with pytest.raises(ValueError, match="score_domains scores every domain against a native structure: give `native`"):
        with stub._call(None, Extras()):
            pass
    assert stub.calls == []
    stub.set_score_domains(False)
    with stub._call(None, Extras()):
        assert stub.calls == []


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["80+80", "insertion"])
def test_perfect_domains_in_a_wrong_arrangement(name):
    """Each domain of the "native" moved by its own rigid transform: every domain alone is perfect, the whole chain is not, and
    only the inter-domain lDDT says so."""
    trace, built = R.constructed(name)
    parse = R.parse(trace)
    labels, D = parse["labels"], parse["header"][0]
    assert D == 2 and (name != "80+80" or np.array_equal(labels, built))
    L = len(labels)
    native = DR.moved_by_domain(trace, labels)
    whole, _ = yardstick(trace, native)
    assert whole["tm"] < 0.7 and whole["lddt"] > 0.99
    block, legs = DR.block(trace, native, labels, D)
    un = S.unpack_domain_scores(block, L)
    assert un["domains"] == D and un["domains_native"] == 0 and un["present"] == L and len(un["legs"]) == 1
    leg = un["legs"][0]
    for d, (row, want) in enumerate(zip(leg["rows"], legs[0]["rows"])):
        assert want["margin"] >= NEAR_TIE, (d, want["margin"])
        assert want["tm"] >= 1.0 - 1e-6 and want["lddt"] == 1.0 and row["lddt"] == 1.0 and row["tm"] >= np.float32(1.0 - 1e-6)
        assert row["n"] == row["size"] == int((labels == d).sum()) and row["preserved"] == 4 * row["pairs"] > 0
        assert row["outer_pairs"] > 0 and row["outer_preserved"] < 4 * row["outer_pairs"]
    assert leg["lddt_intra"] == 1.0 and leg["lddt_inter"] < leg["lddt_intra"] and leg["tm_domains"] >= 1.0 - 1e-6
    assert leg["tm_domains"] - whole["tm"] > 0.3
    assert sum(r["pairs"] + r["outer_pairs"] for r in leg["rows"]) == DR.near_pairs(native)
    # the scatter: every residue carries its own domain's values
    for d in range(D):
        mine = labels == d
        assert np.array_equal(leg["lddt_res"][mine], legs[0]["rows"][d]["lddt_res"][mine].astype(np.float32))
        assert np.array_equal(leg["deviation"][mine], legs[0]["rows"][d]["deviation"][mine].astype(np.float32))
    js = S.domain_scores_json(un, S.unpack_domains(R.block(parse), L))
    assert [r["size"] for r in js["model"]["rows"]] == parse["table"][:, 0].tolist() and "native" not in js
    if name == "insertion":
        assert len(js["model"]["rows"][0]["segments"]) == 2, "a domain of two segments"


def test_masking_and_partial_natives_in_the_restatement():
    """A domain left with fewer than three native rows has NaN scores and its counts; an absent row is absent from every count."""
    trace, _ = R.constructed("80+80")
    labels = R.parse(trace)["labels"]
    native = DR.moved_by_domain(trace, labels)
    native[2:80] = np.nan                                     # domain 0 keeps rows 0 and 1
    one = DR.leg(trace, native, labels, 2)
    row = one["rows"][0]
    assert row["n"] == 2 and row["size"] == 80 and np.isnan(row["tm"]) and row["pairs"] == 2 and row["preserved"] == 8
    assert np.isnan(one["lddt_res"][:80]).all() and not np.isnan(one["lddt_res"][80:]).any()
    assert one["rows"][1]["n"] == 80 and one["rows"][1]["outer_pairs"] == row["outer_pairs"], "the outer pairs are mutual"
    h = DR.row_floats(row)
    assert h[0] == 2 and h[1] == 2 and np.isnan(h[2:7]).all() and h[28] == 80 and (h[29:] == 0).all()
