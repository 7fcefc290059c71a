"""Option "msa_report" on the host (no GPU, no library): tests/msa_report_ref.py on a hand-worked alignment and at the edges of
its definition, the layout arithmetic against the recorded tests/golden/conf_layout.json, score.unpack_msa_report /
msa_report_json on reference blocks, the hidden flags of both parsers, the batch summary's Neff bins.  On the parent commit the
layout, the unpacker and the flags do not exist and those tests fail."""
import importlib.util
import json
import os

import numpy as np
import pytest

import msa_report_ref as R

from dmpfold2_amd import score as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 20

# A R N D C Q = 0 .. 5.  Row 1 copies the query; column 2 is all gaps; the query has a gap in column 4.
HAND = np.array([[0, 1, G, 3, G, 5],
                 [0, 1, G, 3, G, 5],
                 [0, 2, G, 3, 4, G],
                 [1, 1, G, G, 21, 5]], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_hand_worked_alignment():
    """4 x 6, every entry written out.  cnt (gaps match gaps, 21 clamps to the gap):
         r0 r1 6 | r0 r2: cols 0, 2, 3 = 3 | r0 r3: cols 1, 2, 4, 5 = 4 | r2 r3: col 2 = 1.
       Thresholds float32(6 t) = 3.72, 4.8, 5.4: neighbours at 0.62 are r0 {r0, r1, r3}, r1 the same, r2 {r2}, r3 {r0, r1, r3};
       at 0.8 and 0.9 r0 {r0, r1}, r1 the same, r2 {r2}, r3 {r3}."""
    contacts = np.zeros((6, 6), dtype=np.float32)
    contacts[0, 5] = contacts[5, 0] = 0.5
    ref = R.report(HAND, contacts)
    h, c = ref["header"], ref["columns"]
    assert h[0] == 4 and h[1] == 6
    assert np.array_equal(ref["nbr"], [[3, 3, 1, 3], [2, 2, 1, 1], [2, 2, 1, 1]])
    assert h[2] == pytest.approx(1 / 3 + 1 / 3 + 1 + 1 / 3, abs=1e-15) and h[3] == 3.0 and h[4] == 3.0
    assert h[5] == 2 + 2 + 2 + 3 and h[6] == 2 and h[7] == 2 and not h[8:16].any()
    # identity to the query over its 4 letters: 4/4, 4/4, 2/4, 2/4 (r3: cols 1, 5) -> bins 19, 19, 10, 10
    assert h[16 + 19] == 2 and h[16 + 10] == 2 and h[16:36].sum() == 4
    # coverage 4/6, 4/6, 4/6, 3/6 -> bins 13, 13, 13, 10
    assert h[36 + 13] == 3 and h[36 + 10] == 1 and h[36:56].sum() == 4
    # nearest neighbour 6/6, 6/6, 3/6, 4/6 -> bins 19, 19, 10, 13
    assert h[56 + 19] == 2 and h[56 + 10] == 1 and h[56 + 13] == 1
    assert not h[76:126].any() and h[126] == 1 and h[127] == 0
    w = [0.5, 0.5, 1.0, 1.0]
    assert np.array_equal(ref["weights"], np.asarray(w, dtype=np.float32))
    assert c[0].tolist() == [0, 0, 4, 1, 3, 1]
    assert c[1].tolist() == [3.0, 3.0, 0.0, 2.0, 1.0, 2.0]
    ent = lambda *p: -sum(x * np.log(x) for x in p)
    assert c[2] == pytest.approx([ent(2 / 3, 1 / 3), ent(2 / 3, 1 / 3), 0.0, 0.0, 0.0, 0.0], abs=1e-15)
    assert c[3][[0, 1, 3, 4, 5]].tolist() == [0, 1, 3, 4, 5] and np.isnan(c[3][2]) and np.isnan(c[4][2])
    assert c[4][[0, 1, 3, 4, 5]] == pytest.approx([2 / 3, 2 / 3, 1.0, 1.0, 1.0], abs=1e-15)
    assert c[5][[0, 1, 3, 5]] == pytest.approx([2 / 3, 2 / 3, 1.0, 1.0], abs=1e-15) and np.isnan(c[5][[2, 4]]).all()
    # |j - l| >= 6 never holds at L = 6
    assert np.isnan(c[6]).all() and np.isnan(c[7]).all()


@pytest.mark.parametrize("L", [5, 6, 16, 50, 63, 64, 65, 67, 129, 300])
def test_rows_at_the_threshold_edges_fall_on_the_right_side(L):
    """A row with exactly floor(L t) matches is no neighbour, one with floor(L t) + 1 is, by the float32 comparison
    float32(cnt) > float32(float64(L) t) - at L = 5 and 0.8 the product 4.000000000000001 rounds to 4.0f, and 4 > 4 fails; at
    L = 50 and 0.62 the product 31.0 is exact."""
    query = np.arange(L, dtype=np.uint8) % 20
    for k, t in enumerate(R.THRESHOLDS):
        m = int(np.floor(L * t))
        rows = [query]
        for matches in (m, m + 1):
            if matches <= L:
                r = query.copy()
                r[:L - matches] = (r[:L - matches] + 1) % 20
                rows.append(r)
        a = np.stack(rows)
        cnt = R.pair_counts(R.clamp(a))
        assert cnt[0, 1] == m and (len(rows) == 2 or cnt[0, 2] == m + 1)
        nbr = R.report(a, np.zeros((L, L), dtype=np.float32))["nbr"][k]
        # the query's neighbours: itself and the row one match above the edge, never the row on it
        assert nbr[0] == len(rows) - 1 and not np.float32(m) > np.float32(float(L) * t)
    assert np.float32(5.0 * 0.8) == np.float32(4.0) and R.neighbour_counts(np.array([[5, 4], [4, 5]]), 5, 0.8).tolist() == [1, 1]


def test_bin_edges_and_empty_denominators():
    assert [R.bin20(n, 20) for n in (0, 1, 19, 20)] == [0, 1, 19, 19]
    assert [R.bin20(n, 40) for n in (1, 2, 3, 39, 40)] == [0, 1, 1, 19, 19] and R.bin20(3, 0) == 0
    assert S.hist_median([0] * 20) != S.hist_median([0] * 20) and S.hist_median([1] + [0] * 19) == 0.025
    assert S.hist_median([0] * 10 + [2] + [0] * 8 + [2]) == 0.525 and S.hist_median([0] * 19 + [3]) == 0.975
    # a query of gaps alone: den = 0, every row in bin 0
    a = np.full((3, 8), G, dtype=np.uint8)
    a[1:, :4] = 3
    ref = R.report(a, np.zeros((8, 8), dtype=np.float32))
    assert ref["header"][16] == 3 and ref["header"][7] == 8 and np.isnan(ref["columns"][5]).all()
    assert ref["columns"][3][:4].tolist() == [3] * 4 and np.isnan(ref["columns"][3][4:]).all() and not ref["columns"][1][4:].any()


def test_one_row():
    a = np.array([[0, 1, 2, G, 4, 5, 6, 7, 8, 9]], dtype=np.uint8)
    ref = R.report(a, None, np.zeros((10, 3), dtype=np.float32))
    h, c = ref["header"], ref["columns"]
    assert h[2:5].tolist() == [1, 1, 1] and h[6] == 0 and h[126] == 0 and h[127] == 1 and not h[56:126].any()
    assert h[16 + 19] == 1 and h[36 + 18] == 1 and np.isnan(c[6]).all() and np.isnan(c[7]).all()
    assert c[1].tolist() == [1, 1, 1, 0, 1, 1, 1, 1, 1, 1] and not c[2].any()


def test_the_descending_key():
    """Ties, +-0 and a NaN: strongest first, +0 in front of -0, the NaN last, ties to the lower (i, j)."""
    c = np.zeros((8, 8), dtype=np.float32)
    pairs = [(0, 6), (0, 7), (1, 7), (2, 3), (3, 4), (4, 5), (5, 6)]
    for (i, j), v in zip(pairs, [0.5, np.nan, 0.5, -0.0, 0.0, -1.0, np.inf]):
        c[i, j] = v
    assert R.ranked_pairs(c, pairs) == [(5, 6), (0, 6), (1, 7), (3, 4), (2, 3), (4, 5), (0, 7)]
    keys = R.rank_bits(np.array([np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf, np.nan, -np.nan], dtype=np.float32))
    assert (np.diff(keys[:6].astype(np.int64)) > 0).all() and keys[6] == keys[7] == 0xffffffff and keys[5] < 0xffffffff
    # dca_max takes the same order: the lowest partner among equals
    c = np.zeros((14, 14), dtype=np.float32)
    c[0, 8] = c[0, 11] = 0.25
    ref = R.report(np.zeros((2, 14), dtype=np.uint8), c)
    assert ref["columns"][7][0] == 8 and ref["columns"][6][0] == 0.25 and ref["columns"][7][7] == 0 and ref["columns"][7][6] == 0


def test_dca_against_a_native_by_hand():
    """A straight chain at 3.8 A: |i - j| = 2 is the last native contact (7.6 A), so no candidate is one; a hairpin adds (0, 7)."""
    L = 30
    native = np.zeros((L, 3), dtype=np.float32)
    native[:, 0] = 3.8 * np.arange(L)
    c = np.zeros((L, L), dtype=np.float32)
    c[0, 7] = 2.0
    c[1, 20] = 1.0
    out, n, ln = R.dca_vs_native(c, native)
    assert (n, ln) == (30, 30.0) and out[0] == sum(min(L, i + 12) - (i + 6) for i in range(L) if i + 6 < L) and out[1] == 0
    assert out[5:8].tolist() == [30, 15, 6] and out[12 + 5:12 + 8].tolist() == [30, 15, 6] and not out[2:5].any()
    assert out[36] == out[12] + out[24] and out[8:12].tolist() == [0] * 4
    native[7] = native[0] + np.float32([-6, 3, 0])       # 6.7 A from residue 0, 10.2 A from residue 1
    native[9] = np.nan
    out, n, ln = R.dca_vs_native(c, native, 12.0)
    assert (n, ln) == (29, 12.0) and out[1] == 1 and out[2:5].tolist() == [1, 1, 1] and out[5:8].tolist() == [12, 6, 2]


# ------------------------------------------------------------------------------------------------ the layout
def test_with_the_option_off_the_walk_is_the_recorded_one():
    with open(os.path.join(ROOT, "tests", "golden", "conf_layout.json")) as fh:
        rows = json.load(fh)
    spec = importlib.util.spec_from_file_location("record_conf_layout", os.path.join(ROOT, "tools", "record_conf_layout.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    seen = 0
    for L, distmap, score, score_map, align_m, max_L, search, floats, s0, m0, a0, b0, views in rows:
        if floats is None or search is not None:
            continue
        lay = S.Layout(L, distmap, score, score_map, rec.resolve(align_m, max_L), None, max_L, msa_report=0)
        assert lay.msa_report == 0 and (lay.total, lay.score_off, lay.mapscore_off, lay.align_off) == (floats, s0, m0, a0)
        assert lay.msa_report_off == lay.align_off and lay.msa_report_block(np.zeros(lay.total, dtype=np.float32)) is None
        for value in (1, 2):
            on = lay._replace(msa_report=value)
            q = S.msa_report_floats(L, value == 2)
            assert on.msa_report_off == a0 and on.align_off == a0 + q and on.total == floats + q and on.score_off == s0
        seen += 1
    assert seen > 50


def test_layout_arithmetic():
    for L in (8, 65, 300):
        assert S.msa_report_floats(L) == 128 + 8 * L and S.msa_report_floats(L, True) == 128 + 8 * L + L * L
        off = S.Layout(L, score=True, domains=True, score_domains=True, flex=True, align_m=7)
        for value in (1, 2):
            on = off._replace(msa_report=value)
            q = S.msa_report_floats(L, value == 2)
            assert on.msa_report == value and on.flex is True
            assert on.msa_report_off == off.align_off == off.flex_off + S.flex_floats(L)      # between flex and align
            assert on.align_off == on.msa_report_off + q and on.total == off.total + q
            for name in ("score_off", "mapscore_off", "ss_off", "exposure_off", "domains_off", "domain_score_off", "flex_off"):
                assert getattr(on, name) == getattr(off, name), name
            buf = np.arange(on.total, dtype=np.float32)
            out = on.split(buf)
            assert out.msa_report_block.shape == (q,) and out.msa_report_block[0] == on.msa_report_off
            assert out.flex_block[0] == on.flex_off and out.align_block[0] == on.align_off
            assert off.split(buf[:off.total]).msa_report_block is None
            assert np.array_equal(on.msa_report_block(buf), out.msa_report_block)
            assert out._replace(coords=None).msa_report_block is out.msa_report_block
        alone = S.Layout(L, msa_report=2)
        assert alone.msa_report_off == L and alone.total == L + 128 + 8 * L + L * L
    assert S.MSA_REPORT.option == "msa_report" and S.MSA_REPORT.field == "msa_report_block" and S.MSA_REPORT not in S.BLOCKS
    assert S.MSA_REPORT.floats(10, 1) == 208 and S.MSA_REPORT.floats(10, 2) == 308


# ------------------------------------------------------------------------------------------------ pack, unpack, JSON
def _block(a, contacts, native=None, with_map=True):
    ref = R.report(a, contacts, native)
    b = np.concatenate([ref["header"], ref["columns"].reshape(-1)] + ([np.asarray(contacts).reshape(-1)] if with_map else []))
    return ref, b.astype(np.float32)


def test_unpack_pack_and_json_round_trip():
    rng = np.random.default_rng(5)
    L, N = 40, 12
    a = rng.integers(0, 21, (N, L)).astype(np.uint8)
    a[1] = a[0]
    c = rng.normal(size=(L, L)).astype(np.float32)
    c = (c + c.T) / 2
    native = np.cumsum(rng.normal(size=(L, 3)) * 2.2, axis=0).astype(np.float32)
    ref, b = _block(a, c, native)
    confs = rng.random(L).astype(np.float32)
    seq = "".join(S.AA1[x] if x < 20 else "-" for x in a[0])
    rep = S.unpack_msa_report(b, L, confs=confs, seq=seq)
    assert rep["N"] == N and rep["L"] == L and rep["copies"] == 2 and rep["has_dca"] and rep["has_native"]
    assert rep["neff_80"] == float(np.float32(ref["header"][3])) and rep["neff_per_L"] == rep["neff_80"] / L
    assert rep["neff_per_sqrtL"] == rep["neff_80"] / np.sqrt(L) and rep["gap_share"] == ref["header"][5] / (N * L)
    assert np.array_equal(rep["hist_idq"], ref["header"][16:36].astype(np.int64)) and rep["hist_cov"].sum() == N
    assert rep["median_coverage"] == S.hist_median(rep["hist_cov"]) and 0 < rep["median_identity"] < 1
    assert np.array_equal(rep["dca_map"].view(np.uint32), c.view(np.uint32)) and rep["dca_map"].shape == (L, L)
    assert np.array_equal(rep["cons"][rep["cons"] >= 0], ref["columns"][3][~np.isnan(ref["columns"][3])].astype(np.int64))
    assert len(rep["cons_seq"]) == L and set(rep["r_conf"]) == {"neff_col", "entropy", "dca_max"} == set(rep["rho_conf"])
    assert rep["r_conf"]["entropy"] == pytest.approx(np.corrcoef(confs.astype(np.float64), rep["entropy"].astype(np.float64))[0, 1], abs=1e-12)
    for k, name in enumerate(S.MSA_CLASSES):
        cls, o = rep["classes"][name], ref["header"][76 + 12 * k:88 + 12 * k]
        assert (cls["candidates"], cls["native_contacts"]) == (o[0], o[1]) and cls["h"] == o[2:5].tolist() and cls["t"] == o[5:8].tolist()
        for d in range(3):
            want = o[2 + d] / o[5 + d] if o[5 + d] else float("nan")
            assert cls["precision"][d] == want or (want != want and cls["precision"][d] != cls["precision"][d])
            if o[1] and o[5 + d]:
                assert cls["enrichment"][d] == pytest.approx(want / (o[1] / o[0]), rel=1e-15)
    # pack is the inverse of the raw views
    header = {k: rep[k] for k in S.MSA_NEFF + S.MSA_HISTS + ("N", "gap_cells", "copies", "query_gaps", "n", "ln", "has_dca", "has_native")}
    header["classes"] = [rep["classes"][name] for name in S.MSA_CLASSES]
    again = S.pack_msa_report(L, header, rep["columns"], rep["dca_map"])
    assert np.array_equal(again.view(np.uint32), b.view(np.uint32))
    # the JSON form survives a round trip and never holds the map
    js = json.loads(json.dumps(S.msa_report_json(rep, arrays=True)))
    assert js["N"] == N and js["neff_80"] == rep["neff_80"] and "dca_map" not in js and js["classes"]["long"]["t"] == rep["classes"]["long"]["t"]
    assert js["cons"][:3] == [int(v) if v >= 0 else None for v in rep["cons"][:3]] and len(js["entropy"]) == L and js["cons_seq"] == rep["cons_seq"]
    assert "gaps" not in S.msa_report_json(rep) and S.MSA_REPORT.json(rep)["copies"] == 2
    # value 1: no map; no native: no classes; a faulted block: zero counts
    short = S.unpack_msa_report(b[:128 + 8 * L], L)
    assert "dca_map" not in short and "r_conf" not in short and short["classes"]["short"] == rep["classes"]["short"]
    _, plain = _block(a, c, None, with_map=False)
    assert "classes" not in S.unpack_msa_report(plain, L) and "classes" not in S.msa_report_json(S.unpack_msa_report(plain, L))
    nan = S.unpack_msa_report(np.full(128 + 8 * L, np.nan, dtype=np.float32), L)
    assert nan["N"] == 0 and not nan["has_dca"] and nan["hist_cov"].sum() == 0 and (nan["cons"] == -1).all()
    with pytest.raises(ValueError):
        S.unpack_msa_report(b[:-1], L)


def test_the_restatement_checks_itself_and_the_bounds_bite():
    rng = np.random.default_rng(9)
    a = rng.integers(0, 21, (30, 24)).astype(np.uint8)
    c = rng.normal(size=(24, 24)).astype(np.float32)
    ref, b = _block(a, c)
    assert not R.failed(R.check(ref, b, 24))
    for off, name in ((3, "neff_80"), (128 + 24 + 5, "neff_col"), (128 + 2 * 24 + 5, "entropy"), (128 + 4 * 24 + 5, "cons_freq")):
        bad = b.copy()
        bad[off] = np.nextafter(np.nextafter(bad[off], np.float32(np.inf)), np.float32(np.inf))
        assert R.failed(R.check(ref, bad, 24)) == [name], name
    bad = b.copy()
    bad[5] += 1
    assert R.failed(R.check(ref, bad, 24)) == ["header_exact"]
    bad = b.copy()
    bad[128 + 7 * 24 + 1] += 1
    assert R.failed(R.check(ref, bad, 24)) == ["dca_partner"]


# ------------------------------------------------------------------------------------------------ the front ends
def test_the_parsers_take_the_flags_and_their_help_does_not_mention_them():
    from dmpfold2_amd import batch
    from dmpfold2_amd import predict as P
    single, many = P.dmpfold_parser(), batch.batch_parser()
    for text in (single.format_help(), many.format_help()):
        assert "msa-report" not in text and "dca-map" not in text
    a = single.parse_args(["-i", "x.aln", "--msa-report", "--msa-report-file", "m.json", "--dca-map", "d.npy"])
    assert a.msa_report is True and a.msa_report_file == "m.json" and a.dca_map == "d.npy"
    assert not any(hasattr(single.parse_args(["-i", "x.aln"]), k) for k in ("msa_report", "msa_report_file", "dca_map"))
    assert hasattr(single.parse_args(["-i", "x.aln", "--dca-map", "d.npy"]), "dca_map")
    b = many.parse_args(["-i", "x.aln", "-o", "out", "--msa-report", "--dca-map"])
    assert b.msa_report is True and b.dca_map is True and not hasattr(many.parse_args(["-i", "x.aln", "-o", "out"]), "msa_report")
    import inspect
    for fn in (P.Engine.predict, P.aln_to_coords, P.Pipeline.__init__):
        assert not any("msa" in k or "dca" in k for k in inspect.signature(fn).parameters)
    assert "dca_map" in inspect.signature(P.aln_to_msa_report).parameters and callable(P.Engine.predict_msa_report)
    assert callable(P.Pipeline.use_msa_report) and callable(batch.batch_msa_report)


def test_the_batch_summary():
    from dmpfold2_amd import batch
    found = {"a": {"N": 5, "neff_80": 4.0, "median_coverage": 0.975}, "b": {"N": 3000, "neff_80": 1500.0, "median_coverage": 0.775},
             "c": {"N": 90, "neff_80": 50.0, "median_coverage": 0.875}, "d": {"N": 400, "neff_80": 300.0, "median_coverage": 0.925}}
    s = batch.msa_summary(found)
    assert s["msa_targets"] == 4 and s["msa"] is found and s["mean_msa_neff_80"] == 463.5 and s["median_msa_neff_80"] == 175.0
    assert s["median_msa_N"] == 245.0 and s["mean_msa_median_coverage"] == pytest.approx(0.8875)
    scores = {"a": {"tm": 0.2}, "b": {"tm": 0.9}, "c": {"tm": 0.6}, "d": {"tm": 0.5}, "e": {"tm": 0.1}}
    t = batch.neff_tm_summary(found, scores)
    assert t["neff_tm_targets"] == 4 and t["neff_tm_spearman"] == pytest.approx(0.8)
    assert t["neff_tm_bins"] == {"<10": {"targets": 1, "mean_tm": 0.2}, "10-100": {"targets": 1, "mean_tm": 0.6},
                                 "100-1000": {"targets": 1, "mean_tm": 0.5}, ">=1000": {"targets": 1, "mean_tm": 0.9}}
    scores["c"]["tm"] = None
    t = batch.neff_tm_summary(found, scores)
    assert t["neff_tm_targets"] == 3 and t["neff_tm_bins"]["10-100"] == {"targets": 0, "mean_tm": None} and t["neff_tm_spearman"] == 1.0
    assert batch.neff_tm_summary({"a": found["a"]}, scores)["neff_tm_spearman"] is None
    assert batch.msa_brief({"N": 1, "neff_80": 1.0, "median_coverage": 0.975, "L": 9}) == {"N": 1, "neff_80": 1.0, "median_coverage": 0.975}
    assert ("msa", "msa_report", batch.msa_summary) in batch.GATHERED and batch.GATHERED_AS["msa_report"][0] == "msa"


def test_write_result_takes_the_report(tmp_path):
    import torch
    from dmpfold2_amd import batch
    rng = np.random.default_rng(2)
    L = 12
    a = rng.integers(0, 20, (4, L)).astype(np.uint8)
    c = rng.normal(size=(L, L)).astype(np.float32)
    _, b = _block(a, c)
    rep = S.unpack_msa_report(b, L)
    coords, confs = torch.zeros(L, 5, 3), torch.full((L,), 0.5)
    path = batch.write_result(str(tmp_path), "x/t.aln", coords, confs, a, "npz", msa_report=rep)
    z = np.load(path)
    assert np.array_equal(z["msa_header"], b[:128]) and z["msa_columns"].shape == (8, L) and np.array_equal(z["dca_map"], c)
    batch.write_result(str(tmp_path), "x/t.aln", coords, confs, a, "pdb", msa_report=rep)
    assert json.loads((tmp_path / "t.msa.json").read_text()) == json.loads(json.dumps({"msa": S.msa_report_json(rep)}))
    assert np.array_equal(np.load(str(tmp_path / "t.dca_map.npy")), c)
