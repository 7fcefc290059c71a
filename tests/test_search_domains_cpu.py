"""Option "search_domains" without a GPU: the layout functions, the host helpers of dmpfold2_amd/score.py, both parsers, and the
restatement of the definition (tests/search_domains_ref.py: gather by label, test_align_cpu.yardstick on the gathered trace,
scatter, rank) on constructed two-domain traces.  On the parent commit none of these names exist."""
import itertools

import numpy as np
import pytest

import domains_ref as R
import search_domains_ref as SR
from dmpfold2_amd import score as S
from test_align_cpu import NEAR_TIE, moved, random_walk


# ------------------------------------------------------------------------------------------------ layout
def test_layout_for_every_combination_of_the_neighbouring_options():
    L, K, M = 33, 5, 120
    for distmap, score, ss, exposure, align_m, passes in itertools.product((False, True), (False, True), (False, True), (False, True),
                                                                          (None, 40), (None, 3)):
        kw = dict(distmap=distmap, score=score, score_map=distmap and score, align_m=align_m, search=(K, M), max_L=64,
                  passes=passes if score else None, ss=ss, exposure=exposure)
        off = S.Layout(L, domains=True, **kw)
        on = S.Layout(L, domains=True, search_domains=True, **kw)
        n = S.domain_search_floats(L, K)
        assert n == 16 * K + 16 * K * 24 + 2 * L * K == (400 + 2 * L) * K
        # in front of the block nothing moves; behind it everything moves by its size
        for name in ("info_off", "score_off", "mapscore_off", "pass_off", "ss_off", "exposure_off", "domains_off", "domain_search_off"):
            assert getattr(on, name) == getattr(off, name), name
        assert on.domain_search_off == off.domains_off + S.domains_floats(L) == off.align_off
        for name in ("align_off", "align_end", "search_off", "search_end", "total"):
            assert getattr(on, name) == getattr(off, name) + n, name
        assert on.domain_search_off == S.domain_search_offset(L, distmap, score, distmap and score, passes if score else None, ss, exposure)
        buf = np.arange(on.total, dtype=np.float64)
        out = on.split(buf)
        assert out.domain_search_block.shape == (n,) and out.domain_search_block[0] == on.domain_search_off
        assert out.domains_block[-1] == on.domain_search_off - 1
        assert on.domain_search_block(buf)[0] == on.domain_search_off and off.domain_search_block(buf) is None
        assert off.split(buf[:off.total]).domain_search_block is None
        # `public` never hands the block out, `_replace` keeps it
        assert all(x is not out.domain_search_block for x in out.public())
        assert out._replace(coords=None).domain_search_block is out.domain_search_block
        assert on._replace(L=L).search_domains and not off._replace(L=L).search_domains


def test_offsets_with_the_option_off_are_todays():
    """The recorded layouts (tests/golden/host_plumbing.json.gz has more) know nothing of the option: an attribute that is off, or on
    without a search, changes no offset."""
    for L in (8, 300):
        for search in (None, (3, 40)):
            base = S.Layout(L, True, True, True, 65, search, 64, passes=2, ss=True, exposure=True, domains=True)
            same = base._replace(search_domains=search is None)          # (on without a library: the block is empty)
            for name in ("domains_off", "align_off", "align_end", "search_off", "total"):
                assert getattr(base, name) == getattr(same, name)
    assert S.Layout(40).search_domains is False and S.Layout._make(S.Layout(40)).search_domains is False
    assert "search_domains" not in S.Layout._fields and [r.key for r in S.BLOCKS][-3:] == ["domains", "align", "search"]
    assert S.DOMAIN_SEARCH not in S.BLOCKS and S.DOMAIN_SEARCH.option == "search_domains"


# ------------------------------------------------------------------------------------------------ pack, unpack, JSON
def _made_up(L, K, D, seed=0):
    rng = np.random.default_rng(seed)
    headers = np.full((16, K, 24), np.nan, dtype=np.float32)
    headers[:D] = rng.uniform(0.1, 0.9, size=(D, K, 24)).astype(np.float32)
    headers[:D, :, 0] = rng.integers(3, 9, size=(D, K))
    headers[:D, :, 18] = rng.integers(-4, 5, size=(D, K))
    headers[:D, :, 19] = 7
    headers[:D, :, 20:] = 0
    rank = np.full((16, K), np.nan, dtype=np.float32)
    for d in range(D):
        rank[d] = S.host_rank(headers[d, :, 2])
    ali = rng.integers(-1, 6, size=(K, L)).astype(np.float32)
    dev = np.where(ali < 0, np.nan, rng.uniform(0, 3, size=(K, L))).astype(np.float32)
    return rank, headers, ali, dev


def test_pack_and_unpack_round_trip():
    L, K, D = 21, 4, 3
    rank, headers, ali, dev = _made_up(L, K, D)
    block = S.pack_domain_search(L, K, rank, headers, ali, dev)
    assert block.dtype == np.float32 and block.shape == (S.domain_search_floats(L, K),)
    un = S.unpack_domain_search(block, L, K)
    assert un["domains"] == D and un["rank"].tolist() == rank[:D].astype(int).tolist()
    assert np.array_equal(un["headers"].view(np.uint32), headers.view(np.uint32)) and np.array_equal(un["ali"], ali.astype(np.int64))
    assert np.array_equal(np.isnan(un["deviation"]), np.isnan(dev)) and np.array_equal(np.nan_to_num(un["deviation"]), np.nan_to_num(dev))
    h = un["hits"][1][2]
    assert h["n_ali"] == int(headers[1, 2, 0]) and h["tm_model"] == float(headers[1, 2, 2]) and h["seed_offset"] == int(headers[1, 2, 18])
    assert np.array_equal(h["R"], headers[1, 2, 4:13].reshape(3, 3)) and np.array_equal(h["t"], headers[1, 2, 13:16]) and h["seeds"] == 7
    assert "refined" not in un
    again = S.pack_domain_search(L, K, un["rank_raw"], un["headers"], np.where(ali < 0, -1, ali), un["deviation"])
    assert np.array_equal(again.view(np.uint32), block.view(np.uint32))
    # with "search_refine": header offset 21
    headers[:D, 1, 20] = 1
    un = S.unpack_domain_search(S.pack_domain_search(L, K, rank, headers, ali, dev), L, K, refine=2)
    assert un["refined"].shape == (D, K) and un["refined"][:, 1].tolist() == [False] * D and un["refined"][:, 0].all()
    # a NaN block: a bad m_k, a latched fault
    nan = S.pack_domain_search(L, K)
    assert np.isnan(nan).all()
    un = S.unpack_domain_search(nan, L, K)
    assert un["domains"] == 0 and un["hits"] == [] and un["rank"].shape == (0, K) and (un["ali"] == -1).all()
    assert S.domain_hits_json(un, ["a", "b", "c", "d"]) == {"entries": 4, "domains": []}
    with pytest.raises(ValueError, match="domain-search block"):
        S.unpack_domain_search(block[:-1], L, K)


def test_json_form():
    L, K, D = 21, 4, 3
    rank, headers, ali, dev = _made_up(L, K, D, seed=1)
    headers[0, 3, 1] = np.nan
    labels = np.repeat([0, 1, 2, 0], [5, 6, 7, 3])
    table = [{"size": int((labels == d).sum()), "segment_list": S._segments(labels, d)} for d in range(D)]
    un = S.unpack_domain_search(S.pack_domain_search(L, K, rank, headers, ali, dev), L, K)
    js = S.domain_hits_json(un, ["a", "b", "c", "d"], {"table": table}, top=2)
    assert js["entries"] == 4 and [d["domain"] for d in js["domains"]] == [0, 1, 2] and "refine" not in js
    assert js["domains"][0]["size"] == 8 and js["domains"][0]["segments"] == [[0, 4], [18, 20]] and js["domains"][1]["segments"] == [[5, 10]]
    for d in range(D):
        hits = js["domains"][d]["hits"]
        assert [h["index"] for h in hits] == rank[d][:2].astype(int).tolist() and [h["name"] for h in hits] == ["abcd"[h["index"]] for h in hits]
        assert set(hits[0]) == {"name", "index", "tm_domain", "tm_struct", "rmsd_ali", "n_ali", "R", "t"}
        assert hits[0]["tm_domain"] == float(headers[d, hits[0]["index"], 2])
    every = S.domain_hits_json(un, ["a", "b", "c", "d"], top=9)
    assert "size" not in every["domains"][0] and len(every["domains"][0]["hits"]) == 4
    assert [h["rmsd_ali"] for h in every["domains"][0]["hits"] if h["index"] == 3] == [None]
    import json
    json.dumps(every)
    refined = S.domain_hits_json(S.unpack_domain_search(S.pack_domain_search(L, K, rank, headers, ali, dev), L, K, refine=2), "abcd", top=1, refine=2)
    assert refined["refine"] == 2 and refined["domains"][0]["hits"][0]["refined"] is True
    assert S.DOMAIN_SEARCH.json(un, names="abcd", top=1)["domains"][2]["hits"][0]["name"] in "abcd"


# ------------------------------------------------------------------------------------------------ the host layers
def test_library_domains(tmp_path):
    lib = S.Library.from_traces([random_walk(9, 1), random_walk(12, 2)])
    assert lib.domains is False
    path = str(tmp_path / "lib.npz")
    lib.save(path)
    assert S.Library.open(path).domains is False and S.Library.open(path, refine=1).domains is False
    opened = S.Library.open(path, refine=1, domains=True)
    assert opened.domains is True and opened.refine == 1 and opened.names == lib.names
    lib.domains = True
    assert lib.domains is True and S.Library.load(path).domains is False


def test_parsers_accept_the_flags_and_hide_them():
    from dmpfold2_amd import batch
    from dmpfold2_amd.predict import dmpfold_parser, run_dmpfold
    for make, empty, with_library in ((dmpfold_parser, ["-i", "x.aln"], ["--search", "lib.npz"]),
                                      (batch.batch_parser, ["-o", "out"], ["--library", "lib.npz"])):
        assert "search-domains" not in make().format_help() and "search_domains" not in make().format_help()
        assert not hasattr(make().parse_args(empty), "search_domains")
        assert make().parse_args(empty + with_library + ["--search-domains"]).search_domains is True
    with pytest.raises(SystemExit) as exc:
        run_dmpfold(["-i", "x.aln", "--search-domains"])
    assert exc.value.code == 2
    with pytest.raises(SystemExit) as exc:
        batch.main(["-i", "x.aln", "-o", "out", "--search-domains"])
    assert exc.value.code == 2


def test_parser_errors_name_the_flag(capsys):
    from dmpfold2_amd import batch
    from dmpfold2_amd.predict import run_dmpfold
    with pytest.raises(SystemExit):
        run_dmpfold(["-i", "x.aln", "--search-domains"])
    assert "--search-domains needs --search" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        batch.main(["-i", "x.aln", "-o", "out", "--search-domains"])
    assert "--search-domains needs --library" in capsys.readouterr().err


def test_the_abi_stays():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5


def test_call_options_turn_domains_on_for_a_library_that_asks():
    """Engine._call_options on a recording stub (as tests/test_search_refine_cpu.py calls it): the library's `domains` sets
    "domains" and "search_domains" for the call and puts both back; without it nothing new is set."""
    from dmpfold2_amd.predict import Engine, Extras

    class Stub:
        max_L = 64
        _call_options = Engine._call_options

        def __init__(self):
            self.options, self.calls = {}, []

        def get_option(self, name):
            return self.options.get(name, 0)

        def set_option(self, name, value):
            self.options[name] = value
            self.calls.append((name, value))

    lib = S.Library.from_traces([random_walk(9, 1), random_walk(12, 2)])
    stub = Stub()
    with stub._call_options(None, Extras(library=lib)):
        assert "search_domains" not in stub.options and "domains" not in stub.options
    lib.domains = True
    stub = Stub()
    with stub._call_options(None, Extras(library=lib)):
        assert stub.options["search_domains"] == 1 and stub.options["domains"] == 1 and stub.options["search_structures"] == 2
    assert all(stub.options[k] == 0 for k in ("search_domains", "domains", "search_structures", "search_max_m"))
    stub = Stub()
    stub.options["domains"] = 1                              # set by hand (set_domains): it stays
    with stub._call_options(None, Extras(library=lib)):
        assert ("domains", 1) not in stub.calls and stub.options["search_domains"] == 1
    assert stub.options["domains"] == 1 and stub.options["search_domains"] == 0


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["80+80", "insertion"])
def test_restatement_on_constructed_two_domain_traces(name):
    """A library holding a moved copy of each domain ranks that copy first for its domain, with the identity alignment on the
    domain's residues; the scatter leaves every residue with its own domain's row."""
    trace, built = R.constructed(name)
    parse = R.parse(trace)
    labels, D = parse["labels"], parse["header"][0]
    assert D == 2 and (name != "80+80" or np.array_equal(labels, built))
    if name == "insertion":
        assert parse["table"][0, 1] == 2, "a domain of two segments"
    L = len(labels)
    copies = [moved(SR.gather(trace, labels, d), 3 + d)[2] for d in range(D)]
    lib = S.Library.from_traces(copies + [random_walk(41, 7)], ["copy0", "copy1", "walk"])
    pairs = {(0, 0), (1, 1), (0, 2), (1, 2), (1, 0)}
    ans = SR.search(trace, labels, D, lib, pairs=pairs)
    for d in range(D):
        idx, want = SR.residues(labels, d), ans["wants"][d, d]
        assert ans["margins"][d, d] >= NEAR_TIE
        assert want["n_ali"] == len(idx) and np.array_equal(want["ali"], np.arange(len(idx))), "the identity on the domain's residues"
        assert abs(want["tm_model"] - 1.0) <= 1e-6 and want["d0_model"] == SR.yardstick(copies[d], copies[d])[0]["d0_model"]
        assert np.array_equal(ans["ali"][d, idx], np.arange(len(idx)))
        assert want["tm_model"] > ans["wants"][d, 2]["tm_model"], "the copy beats the unrelated walk"
    # entry 0 (the copy of domain 0): the residues of domain 1 carry the row of pair (1, 0), not of (0, 0)
    idx1 = SR.residues(labels, 1)
    assert np.array_equal(ans["ali"][0, idx1], ans["wants"][1, 0]["ali"])
    # the whole answer as a block, unpacked, ranked: each domain's first hit is its copy
    full = SR.search(trace, labels, D, lib, pairs=pairs | {(0, 1)})
    un = S.unpack_domain_search(SR.block(L, full), L, len(lib))
    assert un["domains"] == 2 and un["rank"][0][0] == 0 and un["rank"][1][0] == 1
    assert np.isnan(un["rank_raw"][2:]).all() and np.isnan(un["headers"][2:]).all()
    for d in range(D):
        got = SR.hit_of(un, d, d, labels)
        assert np.array_equal(got["ali"], np.arange(len(SR.residues(labels, d)))) and got["n_ali"] == len(got["ali"])
        assert un["rank"][d].tolist() == S.host_rank(full["headers"][d, :, 2].astype(np.float32)).tolist()
    js = S.domain_hits_json(un, lib.names, S.unpack_domains(R.block(parse), L), top=1)
    assert [d["hits"][0]["name"] for d in js["domains"]] == ["copy0", "copy1"] and [d["size"] for d in js["domains"]] == parse["table"][:, 0].tolist()


def test_ranking_rule_of_the_restatement():
    """NaN entries last in index order, ties to the lower index: the rule of search_rank, per domain."""
    tm = np.array([0.5, np.nan, 0.7, 0.5, np.nan, 0.2], dtype=np.float32)
    assert S.host_rank(tm).tolist() == [2, 0, 3, 5, 1, 4]
