"""Option "domains" on the host: the NumPy restatement's known answers (tests/domains_ref.py), the rules at their edges, the
place of the domain block in the buffer, its unpacker, and the plumbing of both front ends.  No GPU, no library."""
import contextlib
import io
import itertools
import json
import os

import numpy as np
import pytest

import domains_ref as R

from dmpfold2_amd import _lib, batch
from dmpfold2_amd import predict as P
from dmpfold2_amd import score as S


def _q(parse):
    return [ext / den for _, _, _, _, ext, den in parse["splits"]]


# ---------------------------------------------------------------------------------------------------- known answers
def test_single_globules_stay_whole():
    """22 compact globules of 40 .. 250 residues (seed 3): none is split, and the best cut of those large enough to examine
    lies above the rule's tau = 0.25.  (Not every seed's globule does: seed 0 at 190 residues has a cut of q = 0.244.)"""
    best = []
    for L in range(40, 260, 10):
        ca = R.globule(L, 3)
        p = R.parse(ca)
        assert p["header"][0] == 1 and p["splits"] == [] and (p["labels"] == 0).all(), L
        assert p["table"].tolist() == [[L, 1, 0, p["header"][1], 0, 0, 0, 0]]
        if L >= 80:
            _, _, ext, den = R.best_cut(R.contact_table(ca), np.arange(L))
            best.append(ext / den)
    print("best q of the single globules: %.3f .. %.3f" % (min(best), max(best)))
    assert min(best) > 0.25
    stray = R.parse(R.globule(190, 0))
    assert stray["header"][0] == 2 and 0.24 < _q(stray)[0] < 0.25


@pytest.mark.parametrize("sizes", [(80, 80), (100, 150)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_globules_split_at_the_junction(sizes, seed):
    a, b = sizes
    p = R.parse(R.chain(R.globule(a, seed), R.globule(b, seed + 10)))
    assert np.array_equal(p["labels"], np.repeat([0, 1], [a, b]))                  # neither half splits further
    assert [s[:4] for s in p["splits"]] == [(0, 1, 0, a)] and 0.0 < _q(p)[0] < 0.25
    assert p["header"] == [2, p["header"][1], 250, 40, 10, 0, 1, 0]
    ext, den = p["splits"][0][4:]
    assert p["table"].tolist() == [[a, 1, 0, p["table"][0, 3], ext, ext, den, 1], [b, 1, a, p["table"][1, 3], ext, ext, den, 1]]
    assert p["table"][:, 3].sum() + ext == p["header"][1] and den == min(p["table"][:, 3]) + ext


def test_three_globules_and_an_insertion():
    trace, built = R.constructed("3x80")
    p = R.parse(trace)
    assert np.array_equal(p["labels"], built) and p["header"][0] == 3 and p["header"][6] == 2
    assert p["table"][:, 2].tolist() == [0, 80, 160] and sorted(p["table"][:, 7].tolist()) == [1, 2, 2]
    trace, built = R.constructed("insertion")
    p = R.parse(trace)
    assert np.array_equal(p["labels"], built) and p["header"][0] == 2 and p["header"][5] == 1
    assert p["table"][:, :3].tolist() == [[120, 2, 0], [90, 1, 50]] and p["splits"][0][2:4] == (50, 140)


# ---------------------------------------------------------------------------------------------------- the rules at their edges
def _cliques(sizes, links):
    """A contact table made by hand: cliques of the given sizes, and the single contacts `links` between residues."""
    n = sum(sizes)
    t = np.zeros((n, n), dtype=bool)
    at = 0
    for s in sizes:
        t[at:at + s, at:at + s] = True
        at += s
    for i, j in links:
        t[i, j] = t[j, i] = True
    t[np.arange(n), np.arange(n)] = False
    return t


def test_ties_go_to_the_smallest_cut():
    """Three cliques of eight in a row, one contact between neighbours: (0, 8), (0, 16) and (16, 24) all have ext = 1 beside 28
    pairs - q = 1/29 - and (8, 16) has 2/30.  The first in (I, J) order is taken."""
    t = _cliques([8, 8, 8], [(7, 8), (15, 16)])
    ext, int_a, int_b = R.cut_counts(t, np.arange(24))
    assert (ext[0, 8], int_a[0, 8], int_b[0, 8]) == (1, 28, 57) and (ext[0, 16], int_a[0, 16], int_b[0, 16]) == (1, 57, 28)
    assert (ext[16, 24], int_a[16, 24], int_b[16, 24]) == (1, 28, 57) and (ext[8, 16], int_a[8, 16], int_b[8, 16]) == (2, 28, 56)
    assert R.best_cut(t, np.arange(24), 8, 2) == (0, 8, 1, 29)
    # equal ratios of different numbers tie as well: two contacts beside cliques of twice the pairs (2/58 = 1/29)
    t = _cliques([8, 11, 8], [(7, 8), (18, 19), (18, 20)])
    ext, int_a, int_b = R.cut_counts(t, np.arange(27))
    assert (ext[0, 8], min(int_a[0, 8], int_b[0, 8])) == (1, 28) and (ext[19, 27], min(int_a[19, 27], int_b[19, 27])) == (2, 28)
    t = _cliques([8, 8, 11], [(7, 8), (15, 16), (15, 17)])               # ... (0, 8): 1/29; (0, 16): min(57, 55) + 2
    assert R.best_cut(t, np.arange(27), 8, 2)[:2] == (0, 8)


def test_size_and_segment_rules_at_their_edges():
    far = np.asarray([200.0, 0.0, 0.0])
    a, b = R.globule(40, 0), R.globule(40, 10)
    whole = R.parse(np.concatenate([a, b[:39] + far]).astype(np.float32))            # n = 2 min_size - 1: not examined
    assert whole["header"][0] == 1 and whole["splits"] == []
    split = R.parse(np.concatenate([a, b + far]).astype(np.float32))                 # n = 2 min_size: the one admissible size
    assert np.array_equal(split["labels"], np.repeat([0, 1], 40)) and split["splits"] == [(0, 1, 0, 40, 0, split["splits"][0][5])]
    ok = R.admissible(100, 40, 10)
    assert ok[10, 50] and not ok[9, 50] and ok[0, 40] and not ok[0, 39] and ok[0, 60] and not ok[0, 61]
    assert ok[50, 90] and not ok[50, 91] and ok[60, 100] and not ok[61, 100] and not ok[0, 100] and not ok[50, 50]
    assert not ok[10, 90]                                              # (the rest would be 20 residues)
    assert not R.admissible(79, 40, 10).any() and R.admissible(80, 40, 10).sum() == 23   # (size 40 only: I = 0, 10 .. 30, 40)
    # a cut needs contacts on both sides
    lone = _cliques([8, 8], [])
    lone[8:, 8:] = False
    assert R.best_cut(lone, np.arange(16), 8, 8) is None and R.best_cut(_cliques([8, 8], []), np.arange(16), 8, 8) == (0, 8, 0, 28)


def _blobs(count, size=8):
    rng = np.random.default_rng(5)
    return np.concatenate([rng.normal(0.0, 2.0, (size, 3)) + [100.0 * k, 0.0, 0.0] for k in range(count)]).astype(np.float32)


def test_four_levels_and_the_flag_of_level_four():
    """32 blobs of eight residues far apart: every cut between blobs has q = 0, the tie goes to (0, 8), so each level peels one
    blob off; the 224 residues left at level 4 are final although large enough to examine."""
    p = R.parse(_blobs(32), min_size=8, min_segment=2, tau_milli=1)
    assert p["header"][0] == 5 and p["header"][6] == 4 and p["header"][7] == 1
    assert p["table"][:, 0].tolist() == [8, 8, 8, 8, 224] and p["table"][:, 7].tolist() == [1, 2, 3, 4, 4]
    assert [s[:4] for s in p["splits"]] == [(0, 1, 0, 8), (1, 3, 0, 8), (2, 7, 0, 8), (3, 15, 0, 8)]
    p = R.parse(_blobs(5), min_size=8, min_segment=2, tau_milli=1)         # ... and 8 left: too small, no flag
    assert p["header"][0] == 5 and p["header"][7] == 0
    # sixteen domains: the cut in the middle wins when the blobs' contacts grow towards both ends
    assert R.parse(_blobs(3), min_size=8, min_segment=2)["header"][0] == 3


# ---------------------------------------------------------------------------------------------------- the block in the buffer
def test_layout_with_every_combination_of_the_other_blocks():
    L = 24
    for distmap, score, score_map, ss, exposure in itertools.product((False, True), repeat=5):
        for align_m, search, passes in itertools.product((None, 7), (None, (3, 40)), (None, 3)):
            kw = dict(align_m=align_m, search=search, max_L=64, passes=passes, ss=ss, exposure=exposure)
            off, on = S.Layout(L, distmap, score, score_map, **kw), S.Layout(L, distmap, score, score_map, domains=True, **kw)
            assert tuple(off) == tuple(on) and not off.domains and on.domains
            for name in ("info_off", "score_off", "mapscore_off", "pass_off", "ss_off", "exposure_off", "domains_off"):
                assert getattr(on, name) == getattr(off, name), name
            assert on.domains_off == off.align_off == on.exposure_off + (S.exposure_floats(L) if exposure else 0)
            shift = S.domains_floats(L)
            assert shift == 32 + 2 * L + 256
            for name in ("align_off", "align_end", "search_off", "search_end", "total"):
                assert getattr(on, name) == getattr(off, name) + shift, name
            assert on._replace(distmap=True).domains and not on._replace(domains=False).domains
            buf = np.arange(on.total, dtype=np.float64)
            out, plain = on.split(buf), off.split(buf[:off.total])
            assert out.domains_block[0] == on.domains_off and out.domains_block.size == shift and plain.domains_block is None
            assert on.domains_block(buf)[0] == on.domains_off and off.domains_block(buf) is None
            for f in S.Outputs._fields[1:4] + ("score_block", "map_block", "pass_block", "ss_block", "exposure_block"):
                a, b = getattr(out, f), getattr(plain, f)
                assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), f
            for f in ("align_block", "search_block"):
                a, b = getattr(out, f), getattr(plain, f)
                assert (a is None) == (b is None) and (a is None or (a[0] == b[0] + shift and a.size == b.size)), f
            pub = out.public()
            assert pub[-1] is out.domains_block and len(pub) == len(plain.public()) + 1
            assert len(out.public(domains=False)) == len(plain.public()) and len(out.public(blocks=False)) == len(plain.public(blocks=False))
            back = S.Outputs.of(pub, distmap, score, align_m is not None, search is not None, score_map and distmap and score or score_map,
                                passes is not None, ss, exposure, domains=True)
            assert back.domains_block is out.domains_block and back.confs is out.confs
    assert S.HANDOUT[-1] == "domains_block" and S.BLOCK["domains"].option == "domains" and [r.key for r in S.BLOCKS][-3:] == ["domains", "align", "search"]
    assert S.Outputs(1, 2)._replace(coords=None).domains_block is None and S.Outputs(1, 2, domains_block=3)._replace(coords=None).domains_block == 3


def test_unpack_domains_on_a_packed_block():
    trace, built = R.constructed("insertion")
    native = R.constructed("3x80")[0][:210]
    model, nat = R.parse(trace), R.parse(native)
    L = 210
    block = R.block(model, nat)
    assert block.shape == (S.domains_floats(L),)
    confs = np.linspace(0.0, 1.0, L).astype(np.float32)
    d = S.unpack_domains(block, L, coords=trace, confs=confs)
    assert d["domains"] == 2 and d["contacts"] == model["header"][1] and (d["tau_milli"], d["min_size"], d["min_segment"]) == (250, 40, 10)
    assert d["discontinuous"] == 1 and d["depth"] == 1 and d["unexamined"] is False and np.array_equal(d["labels"], built)
    first, second = d["table"]
    assert first["segment_list"] == [[0, 49], [140, 209]] and second["segment_list"] == [[50, 139]]
    assert (first["size"], first["segments"], first["first"], first["level"]) == (120, 2, 0, 1)
    x = trace.astype(np.float64)[built == 1]
    assert second["rg"] == pytest.approx(np.sqrt(((x - x.mean(0)) ** 2).sum(1).mean()), rel=1e-12)
    assert second["mean_conf"] == pytest.approx(confs[50:140].astype(np.float64).mean(), rel=1e-12)
    ext, den = model["splits"][0][4:]
    assert first["q"] == second["q"] == ext / den and d["splits"] == [{"level": 0, "ext": ext, "den": den, "q": ext / den}]
    assert d["has_native"] and d["native"]["domains"] == nat["header"][0] and np.array_equal(d["native"]["labels"], nat["labels"])
    assert "rg" not in d["native"]["table"][0] and [s["level"] for s in d["native"]["splits"]] == sorted(s[0] for s in nat["splits"])
    assert d["overlap"] == S.domains_overlap(built, nat["labels"]) and 0.0 < d["overlap"] < 1.0
    # coords as the (L, 5, 3) backbone; without a native leg; a block of NaN
    bb = np.zeros((L, 5, 3), dtype=np.float32)
    bb[:, 1] = trace
    assert S.unpack_domains(block, L, coords=bb)["table"][1]["rg"] == second["rg"]
    alone = S.unpack_domains(R.block(model), L)
    assert not alone["has_native"] and "native" not in alone and "rg" not in alone["table"][0]
    dead = S.unpack_domains(np.full(S.domains_floats(L), np.nan, dtype=np.float32), L)
    assert dead["domains"] == 0 and dead["table"] == [] and (dead["labels"] == -1).all() and not dead["has_native"]
    with pytest.raises(ValueError):
        S.unpack_domains(block[:-1], L)
    js = S.domains_json(d, arrays=True)
    assert json.loads(json.dumps(js)) == js and js["labels"] == built.tolist() and js["native"]["domains"] == 3 and "overlap" in js
    assert S.BLOCK["domains"].json(d) == S.domains_json(d)
    assert S.BLOCK["domains"].unpack(block, L, coords=trace, confs=confs, library=None, seq=None)["table"][1]["rg"] == second["rg"]


def test_overlap_matches_greedily():
    assert S.domains_overlap([0, 0, 1, 1], [1, 1, 0, 0]) == 1.0
    assert S.domains_overlap([0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 1]) == pytest.approx(5 / 6)
    assert S.domains_overlap([0, 0, 0, 0], [0, 0, 1, 1]) == 0.5 and np.isnan(S.domains_overlap([0, 1], [0]))


# ---------------------------------------------------------------------------------------------------- the plumbing
class _Stub:
    """get_option / set_option of an engine, every set recorded."""

    def __init__(self):
        self.options = {"domains": 0, "domains_tau_milli": 250, "domains_min_size": 40, "domains_min_segment": 10}
        self.sets = []

    def get_option(self, name):
        return self.options[name]

    def set_option(self, name, value):
        self.sets.append((name, value))
        self.options[name] = value


def test_engine_and_pipeline_set_the_four_options():
    assert P.domains_options() == (250, 40, 10) and P.domains_options(1.0, 8, 2) == (1000, 8, 2) and P.domains_options(0.0014, 8, 8)[0] == 1
    for bad in ((0.0, 40, 10), (1.001, 40, 10), (float("nan"), 40, 10), (0.25, 7, 1), (0.25, 1025, 10), (0.25, 40, 0), (0.25, 100, 65), (0.25, 8, 9)):
        with pytest.raises(ValueError):
            P.domains_options(*bad)
    stub = _Stub()
    before = dict(stub.options)
    with P.Engine.with_domains(stub, 0.3, 30, 5):
        assert stub.options == {"domains": 1, "domains_tau_milli": 300, "domains_min_size": 30, "domains_min_segment": 5}
        assert [name for name, _ in stub.sets][-1] == "domains"          # the parameters first: the option's hook sees them
    assert stub.options == before and len(stub.sets) == 8
    with pytest.raises(ValueError):
        with P.Engine.with_domains(stub, 0.3, 8, 9):
            pass
    assert len(stub.sets) == 8                                           # a bad value set nothing
    P.Engine.set_domains(stub, True, 0.5, 20, 4)
    assert stub.options == {"domains": 1, "domains_tau_milli": 500, "domains_min_size": 20, "domains_min_segment": 4}
    P.Engine.set_domains(stub, False)
    assert stub.options["domains"] == 0 and stub.options["domains_min_size"] == 20
    P.Pipeline.use_domains(stub, True)
    assert stub.options == {"domains": 1, "domains_tau_milli": 250, "domains_min_size": 40, "domains_min_segment": 10}
    assert "domains" in P.RESULT_DOCS and isinstance(P.Engine.domains, property) and isinstance(P.Engine.domains_block, property)
    assert P.agree([1, 1], "domains", "use_domains") is True
    with pytest.raises(RuntimeError, match="domains"):
        P.agree([1, 0], "domains", "use_domains")


def test_the_command_line_of_dmpfold():
    parser = P.dmpfold_parser()
    assert "domains" not in parser.format_help()                         # (hidden: an existing test records the help text)
    args = parser.parse_args(["-i", "x.aln"])
    assert not hasattr(args, "domains") and P.domains_arguments(parser, args) is None
    args = parser.parse_args("-i x.aln --domains".split())
    assert P.domains_arguments(parser, args) == (250, 40, 10) and not hasattr(args, "domains_file")
    args = parser.parse_args("-i x.aln --domains --domains-tau 0.4 --domains-min-size 30 --domains-min-segment 5 --domains-file d.json".split())
    assert P.domains_arguments(parser, args) == (400, 30, 5) and args.domains_file == "d.json"
    for bad in ("-i x.aln --domains-tau 0.4", "-i x.aln --domains-file d.json", "-i x.aln --domains --domains-tau 2",
                "-i x.aln --domains --domains-min-size 8 --domains-min-segment 9"):
        args = parser.parse_args(bad.split())
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            P.domains_arguments(parser, args)


def test_the_command_line_and_files_of_dmpfold_batch(tmp_path):
    import torch
    parser = batch.batch_parser()
    assert "domains" not in parser.format_help()
    assert not hasattr(parser.parse_args(["-o", "out"]), "domains")
    args = parser.parse_args("-o out --domains --domains-tau 0.4".split())
    assert args.domains is True and args.domains_tau == 0.4
    assert batch._DOMAINS is None
    with batch.batch_domains(0.4, 30, 5):
        assert batch._DOMAINS == (0.4, 30, 5)
    assert batch._DOMAINS is None
    with pytest.raises(ValueError):
        with batch.batch_domains(0.4, 8, 9):
            pass
    assert ("domains", "domains", batch.domains_summary) in batch.GATHERED
    # the files of one target
    trace, built = R.constructed("80+80")
    L = 160
    dom = S.unpack_domains(R.block(R.parse(trace)), L, coords=trace, confs=np.ones(L))
    coords = np.zeros((L, 5, 3), dtype=np.float32)
    coords[:, 1] = trace
    alnmat = np.zeros((1, L), dtype=np.uint8)
    for fmt in ("npz", "pdb", "ca"):
        out = tmp_path / fmt
        os.makedirs(out)
        path = batch.write_result(str(out), "some/t1.aln", torch.from_numpy(coords), torch.ones(L), alnmat, fmt, domains=dom)
        if fmt == "npz":
            with np.load(path) as z:
                assert np.array_equal(z["dom_label"], built) and z["dom_label"].dtype == np.int32
                assert z["dom_table"].shape == (2, 8) and z["dom_table"][:, 0].tolist() == [80, 80] and z["dom_table"].dtype == np.int32
        else:
            assert sorted(os.listdir(out)) == ["t1.domains.json", "t1.pdb"]
            with open(out / "t1.domains.json") as fh:
                line = json.loads(fh.read())
            assert list(line) == ["domains"] and line["domains"] == S.domains_json(dom)
    # the summary's part
    one = S.domains_json(S.unpack_domains(R.block(R.parse(R.globule(100, 0))), 100))
    part = batch.domains_summary({"a": S.domains_json(dom), "b": one, "c": one})
    assert part["domain_targets"] == 3 and part["mean_domains"] == pytest.approx(4 / 3) and part["median_domains"] == 1.0
    assert part["multi_domain_share"] == pytest.approx(1 / 3) and part["domains"]["a"] == {"domains": 2, "discontinuous": 0, "sizes": [80, 80]}
    assert batch.domains_summary({})["mean_domains"] is None


def test_no_new_entry_point():
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dmpfold_hip.h")) as fh:
        header = fh.read()
    assert "#define DMP_ABI_VERSION 5" in header
    for name in ('"domains"', '"domains_tau_milli"', '"domains_min_size"', '"domains_min_segment"', "32 + 2L + 256"):
        assert name in header, name
    with open(os.path.join(root, "dmpfold2_amd", "csrc", "api.hip")) as fh:
        api = fh.read()
    assert all(f'{{"{n}", TAIL(' in api for n in ("domains", "domains_tau_milli", "domains_min_size", "domains_min_segment"))
    assert "domains.hip" in __import__("dmpfold2_amd.build", fromlist=["SOURCES"]).SOURCES
