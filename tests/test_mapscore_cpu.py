"""Host side of option "score_map" (dmpfold2_amd/score.py) and the yardstick the GPU tests compare with.

The yardstick restates include/dmpfold_hip.h in NumPy (the reference has no such quantity): float64 throughout, float32
exactly where the definition says float32 - the native contact test, every operation rounded, and the predicted contact
test on the float32 map.  The contact side therefore has no near ties: both sides evaluate the same float32 expression
and compare integers.  The distance side compares float64 values with 0.5, 1, 2, 4 and 15 A; the yardstick returns the
smallest |value - cutoff| it met, and two float64 evaluations of the same formula differ by about 1e-13, so with a margin
of 1e-9 A or more every count is the same on both sides.

On the parent commit the tests of the host functions fail (score.mapscore_floats, unpack_map_scores, map_scores_json and
the `score_map` arguments are unknown, `dmpfold --score-map` is an unknown flag); the tests of the yardstick alone pass.
"""
import json

import numpy as np
import pytest

from dmpfold2_amd import score as S

NEAR_TIE = 1e-9
CLASSES = ((6, 11), (12, 23), (24, None), (12, None))
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


# ------------------------------------------------------------------------------------------------ the yardstick
def native_contacts(native):
    """(L, L) bool: (dx*dx + dy*dy) + dz*dz < 64 in float32, every operation rounded (NumPy float32 arithmetic does)."""
    q = np.asarray(native, dtype=np.float32)
    d = q[:, None, :] - q[None, :, :]
    with np.errstate(invalid="ignore"):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] < np.float32(64.0)


def yardstick(dm, native, lnorm=0.0):
    """(scores, margin): `scores` in the shape of score.unpack_map_scores (counts as ints, floats in float64, without the
    derived ratios), `margin` the smallest distance of any compared float64 value from its cutoff.  `dm` (L, L) float32,
    `native` (L, 3) float32 with NaN rows."""
    dm = np.asarray(dm, dtype=np.float32)
    native = np.asarray(native, dtype=np.float32)
    L = native.shape[0]
    present = ~np.isnan(native[:, 0])
    n = int(present.sum())
    lnorm = float(np.float32(lnorm))
    ln = lnorm if lnorm > 0 else float(n)
    nan = float("nan")
    out = {"n": n, "ln": ln, "pairs": 0, "map_lddt": nan, "map_mae": nan, "map_rmse": nan, "map_bias": nan,
           "map_lddt_res": np.where(present, 0.0, nan), "classes": {}}
    # ---- contacts and ranked lists: integers from float32 comparisons
    i, j = np.triu_indices(L, 1)
    ok = present[i] & present[j]
    i, j = i[ok], j[ok]
    sep = j - i
    nc = native_contacts(native)[i, j]
    v = dm[i, j]
    with np.errstate(invalid="ignore"):
        pc = v < np.float32(8.0)
    bits = np.ascontiguousarray(v).view(np.uint32).astype(np.uint64)
    for (lo, hi), cname in zip(CLASSES, S.MAP_CLASSES):
        m = (sep >= lo) & ((sep <= hi) if hi is not None else True)
        N = int(m.sum())
        order = np.lexsort((j[m], i[m], bits[m]))          # the key (bits, i, j), ascending
        ranked = nc[m][order]
        hits, taken = [], []
        for d in (1, 2, 5):
            t = min(max(1, int(np.floor(ln / d))), N)
            taken.append(t)
            hits.append(int(ranked[:t].sum()))
        out["classes"][cname] = {"candidates": N, "native_contacts": int(nc[m].sum()), "hits": hits, "taken": taken,
                                 "tp": int((nc[m] & pc[m]).sum()), "predicted": int(pc[m].sum())}
    # ---- distance agreement: float64 from the float32 coordinates, the pair set of score_native's lDDT
    margin = float("inf")
    if n < 2:
        return out, margin
    idx = np.nonzero(present)[0]
    Q = native[idx].astype(np.float64)
    d = Q[:, None, :] - Q[None, :, :]
    dn = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    off = ~np.eye(n, dtype=bool)
    margin = min(margin, float(np.abs(dn - 15.0)[off].min()))
    near = (dn < 15.0) & off
    e = dm[np.ix_(idx, idx)].astype(np.float64) - dn
    pres = np.zeros(n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for tau in THRESHOLDS:
            if near.any() and not np.isnan(e[near]).all():
                margin = min(margin, float(np.nanmin(np.abs(np.abs(e) - tau)[near])))
            pres += ((np.abs(e) < tau) & near).sum(1)
    part = near.sum(1)
    res = np.zeros(n)
    res[part > 0] = pres[part > 0] / (4.0 * part[part > 0])
    out["map_lddt_res"][idx] = res
    pairs = int(part.sum())
    out["pairs"] = pairs
    out["map_lddt"] = float(pres.sum() / (4.0 * pairs)) if pairs else 0.0
    if pairs:
        ee = e[near]
        out["map_mae"] = float(np.abs(ee).sum() / pairs)
        out["map_rmse"] = float(np.sqrt((ee * ee).sum() / pairs))
        out["map_bias"] = float(ee.sum() / pairs)
    return out, margin


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def compare_with_yardstick(got, want, margin, tag=""):
    """`got`: score.unpack_map_scores of the library's block; `want`, `margin`: yardstick().  Every count must be equal.
    map_lddt and its per-residue values are quotients of equal integers, formed in float64 and rounded once on both sides:
    equal too, and certainly within the one float32 ulp allowed here; map_mae, map_rmse and map_bias are float64 sums in
    different orders (relative difference about 1e-13), so only the final rounding can differ: one float32 ulp."""
    assert margin >= NEAR_TIE, f"{tag}: near tie (margin {margin:.3e} A): the caller draws another seed"
    assert (got["n"], got["pairs"]) == (want["n"], want["pairs"]), (tag, got["n"], got["pairs"], want["n"], want["pairs"])
    assert np.float32(got["ln"]) == np.float32(want["ln"]), (tag, got["ln"], want["ln"])
    for cname in S.MAP_CLASSES:
        for k, w in want["classes"][cname].items():
            assert got["classes"][cname][k] == w, (tag, cname, k, got["classes"][cname][k], w)
    seen = {}
    for name in S.MAP_NAMES + ("map_lddt_res",):
        g = np.asarray(got[name], dtype=np.float32).astype(np.float64).reshape(-1)
        w = np.asarray(want[name], dtype=np.float64).reshape(-1).astype(np.float32).astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, name, "NaN pattern", g, w)
        fin = ~np.isnan(w)
        ulps = np.abs(g[fin] - w[fin]) / ulp32(w[fin])
        seen[name] = float(ulps.max()) if ulps.size else 0.0
        assert bool((ulps <= 1.0).all()), (tag, name, "max ulps", seen[name], g[fin], w[fin])
    return seen


# ------------------------------------------------------------------------------------------------ helpers
def _walk(L, seed, step=3.8):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(L, 3))
    v = step * v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.cumsum(v, axis=0).astype(np.float32)


def _own_map(native):
    """The native's own distances as a float32 map (NaN rows give NaN entries), the diagonal poisoned: it is never used."""
    q = np.asarray(native, dtype=np.float64)
    d = q[:, None, :] - q[None, :, :]
    dm = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
    np.fill_diagonal(dm, 1e9)
    return dm


def pack_block(sc, L):
    """A map-score block as the library writes it, from a yardstick result."""
    b = np.zeros(S.mapscore_floats(L), dtype=np.float32)
    b[0], b[1], b[50] = sc["n"], sc["ln"], sc["pairs"]
    for c, cname in enumerate(S.MAP_CLASSES):
        cl = sc["classes"][cname]
        b[2 + 12 * c:2 + 12 * c + 10] = [cl["candidates"], cl["native_contacts"]] + cl["hits"] + cl["taken"] + [cl["tp"], cl["predicted"]]
    b[51:55] = [sc[k] for k in S.MAP_NAMES]
    b[64:] = sc["map_lddt_res"]
    return b


# ------------------------------------------------------------------------------------------------ the definition
def test_native_own_map_is_perfect():
    """A map equal to the native's own distances: map_lddt 1, map_mae 0, and every list holds as many native contacts as
    it can - the contacts sort first (a rounded distance below 8 A is a native contact unless the pair sits within a float32
    rounding of the threshold, which the test excludes)."""
    native = _walk(70, 1)
    dm = _own_map(native)
    i, j = np.triu_indices(70, 1)
    assert (native_contacts(native)[i, j] == (dm[i, j] < 8)).all()
    sc, _ = yardstick(dm, native)
    assert sc["n"] == 70 and sc["ln"] == 70.0 and sc["map_lddt"] == 1.0 and sc["map_mae"] < 1e-6 and sc["map_rmse"] < 1e-6
    assert (sc["map_lddt_res"] == 1.0).all() and sc["pairs"] > 0
    for cname in S.MAP_CLASSES:
        cl = sc["classes"][cname]
        assert cl["hits"] == [min(t, cl["native_contacts"]) for t in cl["taken"]], (cname, cl)
        assert cl["tp"] == cl["predicted"] == cl["native_contacts"]
    m = sc["classes"]
    assert m["medium_long"]["candidates"] == m["medium"]["candidates"] + m["long"]["candidates"]
    assert m["medium_long"]["native_contacts"] == m["medium"]["native_contacts"] + m["long"]["native_contacts"]


def test_class_boundaries():
    """Separations 5 / 6, 11 / 12 and 23 / 24: one predicted native contact at each, everything else far apart."""
    L = 40
    native = np.zeros((L, 3), dtype=np.float32)
    native[:, 0] = 100.0 * np.arange(L)
    for s, want in ((5, None), (6, "short"), (11, "short"), (12, "medium"), (23, "medium"), (24, "long")):
        nat = native.copy()
        nat[3 + s] = nat[3] + np.float32([1.0, 2.0, 2.0])            # 3 A from residue 3
        dm = np.full((L, L), 50.0, dtype=np.float32)
        dm[3, 3 + s] = dm[3 + s, 3] = 3.0
        sc, _ = yardstick(dm, nat)
        for cname in S.MAP_CLASSES:
            inside = cname == want or (cname == "medium_long" and want in ("medium", "long"))
            cl = sc["classes"][cname]
            assert (cl["native_contacts"], cl["tp"], cl["predicted"], cl["hits"][2]) == ((1, 1, 1, 1) if inside else (0, 0, 0, 0)), (s, cname, cl)
    sc, _ = yardstick(np.full((L, L), 50.0, dtype=np.float32), native)
    want_n = {"short": sum(L - s for s in range(6, 12)), "medium": sum(L - s for s in range(12, 24)),
              "long": sum(L - s for s in range(24, L))}
    want_n["medium_long"] = want_n["medium"] + want_n["long"]
    assert {c: sc["classes"][c]["candidates"] for c in S.MAP_CLASSES} == want_n


def test_list_rule():
    """ln from lnorm against ln from n; k_d = 1 when ln < d; t never exceeds the class."""
    native = _walk(30, 2)
    native[::6] = np.nan
    n = int((~np.isnan(native[:, 0])).sum())
    dm = _own_map(_walk(30, 3))
    a, _ = yardstick(dm, native, 0.0)
    b, _ = yardstick(dm, native, 60.0)
    c, _ = yardstick(dm, native, 3.0)
    d, _ = yardstick(dm, native, -4.0)                                # not positive: the rows present
    assert a["ln"] == float(n) == d["ln"] and b["ln"] == 60.0 and c["ln"] == 3.0
    for sc in (a, b, c):
        for cname in S.MAP_CLASSES:
            cl = sc["classes"][cname]
            ks = [max(1, int(sc["ln"] // dd)) for dd in (1, 2, 5)]
            assert cl["taken"] == [min(k, cl["candidates"]) for k in ks]
    assert c["classes"]["short"]["taken"] == [3, 1, 1]                 # floor(3 / 5) = 0 -> 1
    assert a["classes"]["long"]["candidates"] < n and a["classes"]["long"]["taken"][0] == a["classes"]["long"]["candidates"]


def test_tie_rule():
    """Equal map values: the lower (i, j) comes first.  Four short-class pairs share dm = 5; the native contacts are the
    second and the fourth in (i, j) order, so the top 1, 2, 3, 4 hold 0, 1, 1, 2 of them."""
    L = 20
    native = np.zeros((L, 3), dtype=np.float32)
    native[:, 0] = 100.0 * np.arange(L)
    tied = [(0, 7), (0, 9), (1, 7), (2, 10)]
    for k in (1, 3):
        i, j = tied[k]
        native[j] = native[i] + np.float32([0.0, 4.0, 0.0]) + np.float32([0.0, 0.0, 1.0]) * k
    dm = np.full((L, L), 50.0, dtype=np.float32)
    for i, j in tied:
        dm[i, j] = dm[j, i] = 5.0
    for ln, want in ((1.0, 0), (2.0, 1), (3.0, 1), (4.0, 2)):
        sc, _ = yardstick(dm, native, ln)
        cl = sc["classes"]["short"]
        assert cl["taken"][0] == int(ln) and cl["hits"][0] == want, (ln, cl)
    # a NaN sorts behind every number
    dm[0, 7] = dm[7, 0] = np.nan
    sc, _ = yardstick(dm, native, 1.0)
    assert sc["classes"]["short"]["hits"][0] == 1                     # (0, 9) is first now


def test_absent_rows():
    """An absent row takes no part: the figures are those of the chain with the row's pairs removed, at the same
    separations in alignment columns."""
    native = _walk(45, 4)
    dm = _own_map(_walk(45, 5))
    gone = native.copy()
    gone[[7, 20, 21]] = np.nan
    sc, _ = yardstick(dm, gone)
    assert sc["n"] == 42 and np.isnan(sc["map_lddt_res"][[7, 20, 21]]).all() and not np.isnan(np.delete(sc["map_lddt_res"], [7, 20, 21])).any()
    full, _ = yardstick(dm, native)
    lost = sum(1 for i in range(45) for j in range(i + 6, min(i + 12, 45)) if i in (7, 20, 21) or j in (7, 20, 21))
    assert sc["classes"]["short"]["candidates"] == full["classes"]["short"]["candidates"] - lost
    poisoned = dm.copy()
    poisoned[[7, 20, 21], :] = np.nan                                 # what an absent row's map says does not matter
    poisoned[:, [7, 20, 21]] = np.nan
    again, _ = yardstick(poisoned, gone)
    assert json.dumps(S.map_scores_json(S.unpack_map_scores(pack_block(again, 45), 45))) == \
        json.dumps(S.map_scores_json(S.unpack_map_scores(pack_block(sc, 45), 45)))


def test_empty_classes():
    """L = 8: 3 short candidates and no others.  L = 25: one long pair.  One row, none: no fault, NaN floats."""
    sc, _ = yardstick(_own_map(_walk(8, 6)), _walk(8, 6))
    assert [sc["classes"][c]["candidates"] for c in S.MAP_CLASSES] == [3, 0, 0, 0]
    assert sc["classes"]["short"]["taken"] == [3, 3, 1] and sc["classes"]["long"]["taken"] == [0, 0, 0]
    un = S.unpack_map_scores(pack_block(sc, 8), 8)
    assert all(np.isnan(v) for v in un["classes"]["long"]["precision"]) and np.isnan(un["classes"]["long"]["f1_8A"])
    sc, _ = yardstick(_own_map(_walk(25, 7)), _walk(25, 7))
    assert sc["classes"]["long"]["candidates"] == 1 and sc["classes"]["long"]["taken"] == [1, 1, 1]
    assert sc["classes"]["medium_long"]["candidates"] == sc["classes"]["medium"]["candidates"] + 1
    for keep in (0, 1):
        native = np.full((12, 3), np.nan, dtype=np.float32)
        native[5:5 + keep] = 1.0
        sc, margin = yardstick(_own_map(_walk(12, 8)), native)
        assert sc["n"] == keep and sc["pairs"] == 0 and np.isnan(sc["map_lddt"]) and np.isnan(sc["map_mae"]) and margin == float("inf")
        assert all(sc["classes"][c]["candidates"] == 0 and sc["classes"][c]["taken"] == [0, 0, 0] for c in S.MAP_CLASSES)
    far = np.zeros((9, 3), dtype=np.float32)
    far[:, 0] = 100.0 * np.arange(9)
    sc, _ = yardstick(_own_map(far), far)                              # rows, but no pair within 15 A
    assert sc["pairs"] == 0 and sc["map_lddt"] == 0.0 and np.isnan(sc["map_mae"]) and (sc["map_lddt_res"] == 0.0).all()


def test_near_tie_margin():
    """The margin reports how close a pair came to a threshold of the distance side."""
    native = np.zeros((3, 3), dtype=np.float32)
    native[1, 0], native[2, 0] = 5.0, 14.5
    dm = np.float32([[0, 5.5 + 1e-4, 20], [5.5 + 1e-4, 0, 9.5], [20, 9.5, 0]])
    _, margin = yardstick(dm, native)
    assert 5e-5 < margin < 2e-4                                        # |dm - dn| = 0.5001 against the 0.5 A threshold
    native[2, 0] = np.float32(15.0) - np.float32(1e-5)
    _, margin = yardstick(dm, native)
    assert margin < 2e-5                                               # dn against the 15 A radius
    with pytest.raises(AssertionError):
        compare_with_yardstick({}, {}, 1e-12, "near tie")


# ------------------------------------------------------------------------------------------------ the host functions
def test_offsets_with_the_flag_off_are_unchanged():
    """conf_floats, align_offset and search_offset with `score_map` off (the default) give the sums the layout had before
    the option existed, restated here; with it on everything behind the score block moves by 64 + L."""
    for L in (8, 33, 300, 2048):
        for distmap in (False, True):
            for score in (False, True):
                base = L + (L * L + 3 if distmap else 0) + (5 * L + 24 if score else 0)
                assert S.align_offset(L, distmap, score) == base == S.conf_floats(L, distmap, score)
                assert S.search_offset(L, distmap, score) == base
                for m in (0, 3, 40):
                    assert S.conf_floats(L, distmap, score, m) == base + 25 + 2 * L + 3 * m
                    assert S.search_offset(L, distmap, score, m, 64) == base + 25 + 2 * L + 3 * m
                    assert S.search_offset(L, distmap, score, m, 64, True) == base + 64 + L + 25 + 2 * L + 3 * m
                assert S.align_offset(L, distmap, score, True) == base + 64 + L == S.conf_floats(L, distmap, score, None, True)
        assert S.mapscore_floats(L) == 64 + L and S.mapscore_offset(L) == L + L * L + 3 + 5 * L + 24


def test_split_conf_buffer_and_outputs():
    L, m = 10, 5
    n = S.conf_floats(L, True, True, m, True)
    buf = np.arange(n, dtype=np.float32)
    out = S.split_conf_buffer(buf, L, True, True, "coords", m, None, True)
    assert out.map_block[0] == S.mapscore_offset(L) and out.map_block.shape == (64 + L,)
    assert out.align_block[0] == S.mapscore_offset(L) + 64 + L and out.align_block[-1] == n - 1
    assert out.score_block[-1] == out.map_block[0] - 1
    plain = S.split_conf_buffer(buf, L, True, True, "coords", m)
    assert plain.map_block is None and plain.align_block[0] == S.mapscore_offset(L)
    pub = out.public()
    assert len(pub) == 7 and pub[-1] is out.map_block and len(out.public(score_map=False)) == 6
    back = S.Outputs.of(pub, True, True, True, False, True)
    assert back.map_block is out.map_block and back.align_block is out.align_block and back.search_block is None
    assert S.Outputs.of(plain.public(), True, True, True).map_block is None
    with pytest.raises(ValueError):
        S.split_conf_buffer(buf[:n - 1], L, True, True, None, m, None, True)


def test_pack_unpack_json():
    native = _walk(50, 9)
    native[::8] = np.nan
    dm = _own_map(_walk(50, 10))
    sc, _ = yardstick(dm, native, 48.0)
    un = S.unpack_map_scores(pack_block(sc, 50), 50)
    assert un["n"] == sc["n"] and un["ln"] == 48.0 and un["pairs"] == sc["pairs"]
    assert np.array_equal(un["map_lddt_res"], sc["map_lddt_res"].astype(np.float32), equal_nan=True)
    for cname in S.MAP_CLASSES:
        cl, w = un["classes"][cname], sc["classes"][cname]
        assert all(cl[k] == w[k] for k in w)
        assert cl["precision"] == [h / t for h, t in zip(w["hits"], w["taken"])]
        if w["predicted"] and w["native_contacts"]:
            p, r = w["tp"] / w["predicted"], w["tp"] / w["native_contacts"]
            assert cl["precision_8A"] == p and cl["recall_8A"] == r
            assert abs(cl["f1_8A"] - (2 * p * r / (p + r) if p + r else 0.0)) < 1e-12
    js = S.map_scores_json(un)
    text = json.dumps(js)
    assert "NaN" not in text and json.loads(text) == js
    assert js["short"]["precision"]["L5"] == un["classes"]["short"]["precision"][2] and js["map_lddt"] == un["map_lddt"]
    flat = S.map_scores_flat(js)
    assert flat["long_L2"] == js["long"]["precision"]["L2"] and len(flat) == 16
    nanblock = np.full(S.mapscore_floats(50), np.nan, dtype=np.float32)           # a latched fault
    un = S.unpack_map_scores(nanblock, 50)
    assert un["n"] == 0 and np.isnan(un["map_lddt"]) and un["classes"]["long"]["hits"] == [0, 0, 0]
    assert S.map_scores_json(un)["map_lddt"] is None and S.map_scores_json(un)["long"]["precision"]["L"] is None
    with pytest.raises(ValueError):
        S.unpack_map_scores(nanblock[:-1], 50)


def test_cli_argument_errors(tmp_path, capsys):
    """`dmpfold --score-map` and `dmpfold-batch --score-map` are errors without the native(s); nothing is predicted."""
    from dmpfold2_amd import batch
    from dmpfold2_amd.predict import aln_to_coords, dmpfold_parser, run_dmpfold
    assert dmpfold_parser().parse_args(["-i", "x.aln", "--native", "x.pdb", "--score-map"]).score_map is True
    assert dmpfold_parser().parse_args(["-i", "x.aln"]).score_map is False
    with pytest.raises(SystemExit) as exc:
        run_dmpfold(["-i", str(tmp_path / "x.aln"), "--score-map"])
    assert exc.value.code == 2 and "--native" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        batch.main(["-i", str(tmp_path), "-o", str(tmp_path / "out"), "--score-map"])
    assert exc.value.code == 2 and "--natives" in capsys.readouterr().err
    with pytest.raises(ValueError, match="native"):
        aln_to_coords(str(tmp_path / "x.aln"), return_map_scores=True)
    with pytest.raises(ValueError, match="natives"):
        batch.run_batch([], str(tmp_path / "out"), score_map=True)


def test_batch_summary_and_files(tmp_path):
    """score_summary forms means and medians of the map's figures over the targets that have them; write_result puts the
    key "map" into <stem>.scores.json and the map_* arrays into the npz."""
    import torch
    from dmpfold2_amd import batch
    scores = {}
    blocks = {}
    for stem, seed in (("a", 11), ("b", 12)):
        sc, _ = yardstick(_own_map(_walk(40, seed)), _walk(40, seed + 100))
        blocks[stem] = S.unpack_map_scores(pack_block(sc, 40), 40)
        scores[stem] = {"tm": 0.5, "gdt_ts": 0.4, "gdt_ha": 0.3, "rmsd": 2.0, "lddt": 0.6, "map": S.map_scores_json(blocks[stem])}
    scores["c"] = {"tm": 0.7, "gdt_ts": 0.4, "gdt_ha": 0.3, "rmsd": 2.0, "lddt": 0.6}
    summ = batch.score_summary(scores)
    assert summ["scored_targets"] == 3 and summ["map_scored_targets"] == 2
    vals = [scores[s]["map"]["map_lddt"] for s in ("a", "b")]
    assert summ["mean_map_lddt"] == float(np.mean(vals)) and summ["median_map_lddt"] == float(np.median(vals))
    assert "mean_short_L5" in summ and "median_medium_long_L" in summ
    assert "map_scored_targets" not in batch.score_summary({"c": scores["c"]})
    sc = {"n_pairs": 40, "lnorm": 0.0, "rmsd": 1.0, "tm": 0.5, "gdt_ts": 0.5, "gdt_ha": 0.5, "lddt": 0.5, "counts": [1, 2, 3, 4, 5],
          "R": np.eye(3), "t": np.zeros(3), "lddt_res": np.zeros(40), "deviation": np.zeros(40)}
    coords, confs, alnmat = torch.zeros(40, 5, 3), torch.zeros(40), np.zeros((1, 40), dtype=np.uint8)
    batch.write_result(str(tmp_path), "a.aln", coords, confs, alnmat, "pdb", scores=sc, map_scores=blocks["a"])
    assert json.loads((tmp_path / "a.scores.json").read_text())["map"] == scores["a"]["map"]
    batch.write_result(str(tmp_path), "b.aln", coords, confs, alnmat, "pdb", scores=sc)
    assert "map" not in json.loads((tmp_path / "b.scores.json").read_text())
    batch.write_result(str(tmp_path), "a.aln", coords, confs, alnmat, "npz", scores=sc, map_scores=blocks["a"])
    z = np.load(str(tmp_path / "a.npz"))
    assert z["map_counts"].shape == (4, 10) and int(z["map_counts"][0, 0]) == blocks["a"]["classes"]["short"]["candidates"]
    assert float(z["map_lddt"]) == blocks["a"]["map_lddt"] and z["map_lddt_res"].shape == (40,) and int(z["map_n"]) == 40
