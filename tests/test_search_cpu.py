"""Host side of option "search_structures" (include/dmpfold_hip.h): the layout of the search block, the fold library and
its files, the JSON of the hits and the front ends' flags.  Nothing here needs a GPU."""
import itertools
import json

import numpy as np
import pytest

from dmpfold2_amd import score as S
from test_align_cpu import random_walk


def _library(ms=(5, 3, 9), seed=0):
    return S.Library.from_traces([random_walk(m, seed + k) for k, m in enumerate(ms)], [f"d{k}" for k in range(len(ms))])


def _write_pdb(path, ca, chain="A"):
    with open(path, "w") as fh:
        for k, xyz in enumerate(ca):
            fh.write("ATOM  %5d  CA  %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n"
                     % (k + 1, S.AA3[k % 20], chain, k + 1, xyz[0], xyz[1], xyz[2]))
        fh.write("TER\nEND\n")


def test_layout_functions():
    for L, K, M in ((8, 1, 3), (33, 7, 400), (257, 4096, 4096 * 3)):
        assert S.search_floats(L, K, M) == 26 * K + 2 * L * K + 3 * M
    L, max_L = 33, 257
    for emit, score in itertools.product((False, True), repeat=2):
        a0 = S.conf_floats(L, emit, score)
        assert a0 == L + (L * L + 3 if emit else 0) + (5 * L + 24 if score else 0)
        # no align block: B0 is the end of what the other options give
        assert S.search_offset(L, emit, score) == a0
        assert S.search_offset(L, emit, score, None, max_L) == a0
        # an align block with a valid m: behind its trace
        for m in (3, 40, 257):
            assert S.search_offset(L, emit, score, m, max_L) == a0 + 25 + 2 * L + 3 * m
        # an align block whose m the library does not accept counts as m' = 0
        for m in (0, 2, 2.5, 258, float("nan"), -4):
            assert S.search_offset(L, emit, score, m, max_L) == a0 + 25 + 2 * L, m
    assert S.align_m_rule(None, 9) == 0 and S.align_m_rule(9.0, 9) == 9 and S.align_m_rule(10, 9) == 0


def test_split_conf_buffer_places_the_search_block():
    L, K, M, m = 9, 3, 17, 5
    b0 = S.search_offset(L, True, True, m, 64)
    buf = np.arange(b0 + S.search_floats(L, K, M), dtype=np.float32)
    out = S.split_conf_buffer(buf, L, True, True, None, m, (K, M, 64))
    assert out.search_block[0] == b0 and out.search_block.shape == (S.search_floats(L, K, M),)
    assert out.align_block[0] == S.align_offset(L, True, True) and out.public()[-1] is out.search_block
    assert len(out.public(search=False)) == len(out.public()) - 1
    back = S.Outputs.of(out.public(), True, True, True, True)
    assert back.search_block is out.search_block and back.align_block is out.align_block
    with pytest.raises(ValueError):
        S.split_conf_buffer(buf[:-1], L, True, True, None, m, (K, M, 64))
    # without the option the old shape
    assert S.split_conf_buffer(buf, L).search_block is None and len(S.split_conf_buffer(buf, L).public()) == 2


def test_pack_and_unpack_round_trip():
    L = 9
    lib = _library()
    K, M = len(lib), lib.rows
    block = S.pack_library(lib, L)
    assert block.shape == (S.search_floats(L, K, M),) and block[:K].tolist() == [5.0, 3.0, 9.0]
    assert np.isnan(block[K:26 * K + 2 * L * K]).all()
    assert np.array_equal(block[26 * K + 2 * L * K:], lib.ca.reshape(-1))
    assert S.pack_library(lib, L, lengths=[5, 2.5, 9])[1] == 2.5
    un = S.unpack_search(block, L, lib.lengths)
    assert un["rank"].tolist() == [0, 1, 2] and len(un["hits"]) == K
    for k, h in enumerate(un["hits"]):
        assert h["n_ali"] == 0 and (h["ali"] == -1).all() and h["m"] == float(lib.lengths[k])
        assert np.array_equal(h["structure"], lib.entry(k))
    # a filled block: entry 1's header, ali and deviations come back where an align block has them
    hdr = np.arange(24, dtype=np.float32) + 1
    block[K:2 * K] = [1, 2, 0]
    block[2 * K + 24:2 * K + 48] = hdr
    block[26 * K + 2 * L:26 * K + 3 * L] = np.arange(L)
    block[26 * K + 3 * L:26 * K + 4 * L] = 0.5
    un = S.unpack_search(block, L, lib.lengths)
    h = un["hits"][1]
    assert un["rank"].tolist() == [1, 2, 0]
    assert h["n_ali"] == 1 and h["rmsd_ali"] == 2.0 and h["tm_model"] == 3.0 and h["tm_struct"] == 4.0
    assert np.array_equal(h["R"].reshape(-1), hdr[4:13]) and np.array_equal(h["t"], hdr[13:16])
    assert h["ali"].tolist() == list(range(L)) and (h["deviation"] == 0.5).all()
    single = S.unpack_alignment(np.concatenate([[3.0], hdr, np.arange(L), np.full(L, 0.5), lib.entry(1).reshape(-1)]).astype(np.float32), L)
    assert all(np.array_equal(np.asarray(h[k]), np.asarray(single[k])) for k in single)
    with pytest.raises(ValueError):
        S.unpack_search(block[:-1], L, lib.lengths)


def test_library_from_dir_save_and_load(tmp_path):
    d = tmp_path / "lib"
    d.mkdir()
    traces = {"zeta": random_walk(12, 1), "alpha": random_walk(7, 2), "mid": random_walk(30, 3)}
    for name, ca in traces.items():
        _write_pdb(str(d / f"{name}.pdb"), ca)
    (d / "notes.txt").write_text("not a structure\n")
    lib = S.Library.from_dir(str(d))
    assert lib.names == ["alpha", "mid", "zeta"] and lib.lengths.tolist() == [7, 30, 12]
    assert len(lib) == 3 and lib.rows == 49 and lib.max_m == 30 and lib.ca.dtype == np.float32
    for k, name in enumerate(lib.names):
        assert np.array_equal(lib.entry(k), S.read_native_ca(str(d / f"{name}.pdb"))[0])
    lib.save(str(tmp_path / "lib.npz"))
    with np.load(str(tmp_path / "lib.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == ["ca", "lengths", "names"]
    for back in (S.Library.load(str(tmp_path / "lib.npz")), S.Library.open(str(tmp_path / "lib.npz")), S.Library.open(str(d))):
        assert back.names == lib.names and np.array_equal(back.lengths, lib.lengths) and np.array_equal(back.ca, lib.ca)
    with pytest.raises(ValueError):
        S.Library.from_dir(str(tmp_path))


def test_make_library_tool(tmp_path):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "make_library", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_library.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = tmp_path / "lib"
    d.mkdir()
    _write_pdb(str(d / "a.pdb"), random_walk(5, 1))
    _write_pdb(str(d / "b.pdb"), random_walk(6, 2))
    assert mod.main([str(d), str(tmp_path / "o.npz")]) == 0
    assert S.Library.load(str(tmp_path / "o.npz")).names == ["a", "b"]
    assert mod.main([str(d)]) == 2


def test_entries_too_short_or_too_long_are_named():
    lib = S.Library.from_traces([random_walk(5, 1), random_walk(2, 2), random_walk(9, 3)], ["ok", "tiny", "long"])
    with pytest.raises(ValueError, match="tiny"):
        lib.check(64)
    lib = S.Library.from_traces([random_walk(5, 1), random_walk(9, 3)], ["ok", "long"])
    lib.check(9)
    with pytest.raises(ValueError, match="long"):
        lib.check(8)
    with pytest.raises(ValueError):
        S.Library(["a"], [3], np.zeros((4, 3)))
    with pytest.raises(ValueError):
        S.Library([], [], np.zeros((0, 3)))


def test_front_end_parsers_accept_the_new_flags():
    from dmpfold2_amd.batch import batch_parser
    from dmpfold2_amd.predict import dmpfold_parser
    p = dmpfold_parser()
    old = p.parse_args(["-i", "x.aln"])
    assert old.search is None and old.search_top == 10 and old.hits is None
    new = p.parse_args(["-i", "x.aln", "--search", "lib.npz", "--search-top", "3", "--hits", "h.json"])
    assert new.search == "lib.npz" and new.search_top == 3 and new.hits == "h.json"
    b = batch_parser()
    old = b.parse_args(["-i", "x.aln", "-o", "out"])
    assert old.library is None and old.search_top == 10
    new = b.parse_args(["-i", "x.aln", "-o", "out", "--library", "folds", "--search-top", "2"])
    assert new.library == "folds" and new.search_top == 2


def test_host_rank_and_hits_json_with_nan_and_a_tie():
    L = 8
    lib = _library((4, 4, 4, 4, 4))
    K = len(lib)
    block = S.pack_library(lib, L)
    tm = [0.25, np.nan, 0.5, 0.25, np.nan]
    want_rank = [2, 0, 3, 1, 4]                      # ties to the lower index, NaN last in index order
    assert S.host_rank(tm).tolist() == want_rank
    assert S.host_rank([np.nan, np.nan]).tolist() == [0, 1] and S.host_rank([1.0, 1.0, 2.0]).tolist() == [2, 0, 1]
    for k, v in enumerate(tm):
        if v == v:
            block[2 * K + 24 * k:2 * K + 24 * (k + 1)] = 0.0
            block[2 * K + 24 * k + 0] = 4.0          # n_ali
            block[2 * K + 24 * k + 2] = v            # tm_model
            block[2 * K + 24 * k + 3] = v / 2        # tm_struct
    block[K:2 * K] = want_rank
    un = S.unpack_search(block, L, lib.lengths)
    js = S.hits_json(un, lib.names, top=4)
    assert json.loads(json.dumps(js)) == js and js["entries"] == K
    assert [h["name"] for h in js["hits"]] == ["d2", "d0", "d3", "d1"] and [h["index"] for h in js["hits"]] == want_rank[:4]
    assert [h["tm_model"] for h in js["hits"]] == [0.5, 0.25, 0.25, None]
    assert js["hits"][0]["tm_struct"] == 0.25 and js["hits"][0]["n_ali"] == 4 and js["hits"][0]["rmsd_ali"] == 0.0
    assert js["hits"][3]["n_ali"] == 0 and js["hits"][3]["R"] == [[None] * 3] * 3 and js["hits"][3]["t"] == [None] * 3
    assert set(js["hits"][0]) == {"name", "index", "tm_model", "tm_struct", "rmsd_ali", "n_ali", "R", "t"}
    assert len(S.hits_json(un, lib.names)["hits"]) == K and S.hits_json(un, lib.names, top=0)["hits"] == []
    # a block whose rank the library answered with NaN (a latched fault) reads as index order
    block[K:2 * K] = np.nan
    assert S.unpack_search(block, L, lib.lengths)["rank"].tolist() == list(range(K))


def test_abi_is_unchanged():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5
