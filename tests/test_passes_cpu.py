"""Host side of option "score_passes" (include/dmpfold_hip.h): where the pass block lies (score.Layout with `passes`), how it
is taken apart (unpack_pass_scores, pass_scores_json) and what a convergence stop would have done with a full-depth table
(simulate_converge, batch.pass_summary).  No GPU, no library."""
import importlib.util
import itertools
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


def _views(out, fields):
    return [[f, int(getattr(out, f).reshape(-1)[0]), int(getattr(out, f).size)] for f in fields if getattr(out, f) is not None]


# ---- the layout ---------------------------------------------------------------------------------------------------------
def test_layout_positional_order_is_unchanged():
    lay = S.Layout(82.0, 1, 1, 0, 61)
    assert lay[:7] == (82, True, True, False, 61, None, None) and lay.passes is None
    assert S.Layout._fields == ("L", "distmap", "score", "score_map", "align_m", "search", "max_L", "passes", "ss", "exposure")
    assert S.Outputs._fields == ("coords", "confs", "distmap", "info", "score_block", "align_block", "search_block", "map_block", "pass_block",
                                 "ss_block", "exposure_block")
    assert S.pass_floats(1) == 24 and S.pass_floats(128) == 16 + 8 * 128
    assert [S.pass_rows(n) for n in (-3, 0, 10, 127, 128, 5000)] == [1, 1, 11, 128, 128, 128]


def test_without_passes_a_layout_reproduces_every_recorded_row():
    bufs = {}
    for L, distmap, score, score_map, align_m, max_L, search, floats, s0, m0, a0, b0, views in ROWS:
        m = REC.resolve(align_m, max_L)
        row = (L, distmap, score, score_map, align_m, max_L, search)
        lay = S.Layout(L, distmap, score, score_map, m, search, max_L, passes=None)
        assert lay.passes is None and lay.pass_off == lay.align_off == a0, row
        assert lay.score_off == s0 and S.Layout(L, distmap, score, passes=None).mapscore_off == m0, row
        if floats is None:
            with pytest.raises(ValueError):
                S.Layout(L, distmap, score, score_map, m, passes=None).total
        else:
            assert S.Layout(L, distmap, score, score_map, m, passes=None).total == floats, row
        if b0 is None:
            with pytest.raises(ValueError):
                lay.search_off
        else:
            assert lay.search_off == b0, row
        if views is None:
            with pytest.raises(ValueError):
                lay.split(np.zeros(1 << 10))
            continue
        need = max(o + n for _, o, n in views)
        if need not in bufs:
            bufs[need] = np.arange(need, dtype=np.float64)
        out = lay.split(bufs[need])
        assert out.pass_block is None and _views(out, REC.FIELDS) == views, row


@pytest.mark.parametrize("L", [8, 2048])
@pytest.mark.parametrize("R", [1, 11, 128])
def test_with_passes_everything_behind_the_block_moves_by_its_size(L, R):
    for distmap, score_map, align_m, search in itertools.product((False, True), (False, True), (None, 3, 61), (None, (3, 120))):
        if score_map and not distmap:
            continue                                        # "score_map" needs "emit_distmap"
        for max_L in (None, 2048):
            off = S.Layout(L, distmap, True, score_map, align_m, search, max_L)
            on = off._replace(passes=R)
            tag = (L, R, distmap, score_map, align_m, search, max_L)
            assert on.passes == R and on.pass_off == off.pass_off == off.align_off, tag
            assert on.pass_off == on.mapscore_off + (S.mapscore_floats(L) if score_map else 0), tag
            assert (on.score_off, on.mapscore_off) == (off.score_off, off.mapscore_off), tag
            assert on.align_off - off.align_off == 16 + 8 * R and on.search_off - off.search_off == 16 + 8 * R, tag
            assert on.total - off.total == 16 + 8 * R, tag
            buf = np.arange(on.total, dtype=np.float64)
            got, base = on.split(buf), off.split(buf[:off.total])
            assert _views(got, ("pass_block",)) == [["pass_block", on.pass_off, 16 + 8 * R]], tag
            want = [[f, o + (16 + 8 * R if f in ("align_block", "search_block") else 0), n] for f, o, n in _views(base, REC.FIELDS)]
            assert _views(got, REC.FIELDS) == want, tag
            ends = sorted((o, o + n) for _, o, n in _views(got, REC.FIELDS + ("pass_block",)))
            assert ends[0][0] == 0 and ends[-1][1] == on.total and all(a[1] == b[0] for a, b in zip(ends, ends[1:])), tag
            with pytest.raises(ValueError):
                on.split(buf[:-1])


def test_public_puts_the_pass_block_last():
    parts = {name: object() for name in S.Outputs._fields[:9]}          # (of the blocks of its day)
    out = S.Outputs(**parts)
    pub = out.public()
    assert pub[-1] is out.pass_block and pub[-2] is out.map_block and len(pub) == 9
    assert out.public(passes=False) == pub[:-1] and out.public(blocks=False) == pub[:4]
    back = S.Outputs.of(pub, True, True, True, True, True, True)
    assert all(a is b for a, b in zip(back, out))
    none = out._replace(pass_block=None)
    assert none.public() == pub[:-1] and S.Outputs.of(pub[:-1], True, True, True, True, True).pass_block is None


# ---- the block ----------------------------------------------------------------------------------------------------------
def _block(R, rows, rng):
    b = np.full(S.pass_floats(R), np.nan, dtype=np.float32)
    b[:16] = 0.0
    table = b[16:].reshape(R, 8)
    table[:rows] = rng.normal(size=(rows, 8)).astype(np.float32)
    table[:rows, 7] = 0.0
    table[0, 1] = np.inf
    tm, lddt = table[:rows, 2], table[:rows, 6]
    b[:6] = [rows, min(1, rows - 1), int(np.argmax(tm)), int(np.argmax(lddt)), 0.0, 0.0]
    b[4] = tm.max() - tm[int(b[1])]
    b[5] = lddt.max() - lddt[int(b[1])]
    return b


@pytest.mark.parametrize("R,rows", [(1, 1), (11, 11), (11, 4), (128, 128)])
def test_unpack_and_json_round_trip(R, rows):
    b = _block(R, rows, np.random.default_rng(R * 1000 + rows))
    ps = S.unpack_pass_scores(b, R)
    assert ps["R"] == R and ps["rows"] == rows and ps["best_pass"] == int(b[1]) and ps["tm_pass"] == int(b[2])
    assert ps["lddt_pass"] == int(b[3]) and np.float32(ps["regret_tm"]) == b[4] and np.float32(ps["regret_lddt"]) == b[5]
    table = b[16:].reshape(R, 8)
    for k, name in enumerate(S.PASS_COLUMNS):
        assert ps[name].dtype == np.float32 and np.array_equal(ps[name], table[:, k], equal_nan=True), name
        assert np.isnan(ps[name][rows:]).all()
    assert np.isinf(ps["delta"][0])
    js = S.pass_scores_json(ps)
    text = json.dumps(js, allow_nan=False)                      # strict JSON: no NaN, no Infinity
    back = S.pass_scores_from_json(json.loads(text))
    assert set(back) == set(ps)
    for k, v in ps.items():
        if isinstance(v, np.ndarray):
            assert back[k].dtype == np.float32 and np.array_equal(back[k].view(np.uint32) & 0x7fffffff == 0x7fc00000,
                                                                  v.view(np.uint32) & 0x7fffffff == 0x7fc00000), k
            assert np.array_equal(back[k], v, equal_nan=True), k
        else:
            assert back[k] == v or (v != v and back[k] != back[k]), k
    assert js["delta"][0] == "inf" and js["tm"][rows:] == [None] * (R - rows)
    with pytest.raises(ValueError):
        S.unpack_pass_scores(b[:-1], R)
    with pytest.raises(ValueError):
        S.unpack_pass_scores(b, R + 1)


def test_a_block_of_nan_reads_as_no_pass():
    ps = S.unpack_pass_scores(np.full(S.pass_floats(5), np.nan, dtype=np.float32), 5)
    assert ps["rows"] == 0 and ps["best_pass"] is None and ps["tm_pass"] is None and ps["lddt_pass"] is None
    assert ps["regret_tm"] != ps["regret_tm"] and np.isnan(ps["tm"]).all()
    js = S.pass_scores_json(ps)
    assert js["best_pass"] is None and js["regret_tm"] is None and js["conf_mean"] == [None] * 5
    from dmpfold2_amd import batch
    assert batch.pass_summary({"x": js}) == {"pass_scored_targets": 0}


# ---- simulate_converge ----------------------------------------------------------------------------------------------------
def _brute_force(conf, delta, tol_angstrom):
    """The library's rule restated: recycle_delta compares (float)d_p <= (float)tol_mA * 1e-3f after every pass p >= 1 and
    the run ends behind the first pass where that holds (never with the option 0); select_best keeps pass p if p == 0 or
    its float32 mean is strictly above the best so far."""
    conf = [np.float32(v) for v in conf]
    delta = [np.float32(v) for v in delta]
    while conf and conf[-1] != conf[-1]:
        conf.pop()
    tol_mA = 0 if tol_angstrom is None else int(round(float(tol_angstrom) * 1000.0))
    tol = np.float32(np.float32(tol_mA) * np.float32(1e-3))
    ran, best, best_mean = 0, None, None
    for p in range(len(conf)):
        ran = p + 1
        if p == 0 or conf[p] > best_mean:
            best, best_mean = p, conf[p]
        if tol_mA > 0 and p >= 1 and bool(delta[p] <= tol):
            break
    return ran, best


F32 = np.float32
AT_TOL = float(F32(250) * F32(1e-3))           # the library's float32 tolerance of 250 mA, as a double
TABLES = {
    "plain": ([0.1, 0.3, 0.2, 0.5, 0.4], [np.inf, 2.0, 0.9, 0.3, 0.1]),
    "exactly at the tolerance": ([0.1, 0.2, 0.3, 0.4], [np.inf, 1.0, AT_TOL, 0.01]),
    "one float32 above the tolerance": ([0.1, 0.2, 0.3, 0.4], [np.inf, 1.0, float(np.nextafter(F32(AT_TOL), F32(1))), 0.01]),
    "a NaN delta is no stop": ([0.1, 0.2, 0.3, 0.4], [np.inf, np.nan, np.nan, 0.2]),
    "equal means keep the earlier pass": ([0.5, 0.5, 0.5, 0.4], [np.inf, 0.6, 0.2, 0.1]),
    "equal means behind a rise": ([0.1, 0.7, 0.7, 0.2], [np.inf, 3.0, 0.24, 0.1]),
    "never converges": ([0.3, 0.2, 0.1, 0.6, 0.0], [np.inf, 9.0, 8.0, 7.5, 7.4]),
    "one pass": ([0.3], [np.inf]),
    "stopped table with NaN rows": ([0.3, 0.4, np.nan, np.nan], [np.inf, 0.2, np.nan, np.nan]),
    "a NaN mean is never taken": ([0.3, np.nan, 0.2, 0.35], [np.inf, 1.0, 0.5, 0.2]),
}
TOLS = [None, 0.0, 0.0004, 0.05, 0.1, 0.2, 0.25, 0.2504, 0.3, 0.5, 0.9, 1.0, 8.0, 100.0]


@pytest.mark.parametrize("name", list(TABLES))
def test_simulate_converge_is_the_brute_force_rule(name):
    conf, delta = TABLES[name]
    for tol in TOLS:
        assert S.simulate_converge(conf, delta, tol) == _brute_force(conf, delta, tol), (name, tol)


def test_simulate_converge_by_hand():
    conf, delta = TABLES["exactly at the tolerance"]
    assert S.simulate_converge(conf, delta, 0.25) == (3, 2)                 # <=: a delta at the tolerance stops
    conf, delta = TABLES["one float32 above the tolerance"]
    assert S.simulate_converge(conf, delta, 0.25) == (4, 3)                 # the next float32 does not
    assert S.simulate_converge(*TABLES["a NaN delta is no stop"], 0.5) == (4, 3)
    assert S.simulate_converge(*TABLES["equal means keep the earlier pass"], 0.3) == (3, 0)
    assert S.simulate_converge(*TABLES["equal means behind a rise"], 0.25) == (3, 1)
    assert S.simulate_converge(*TABLES["never converges"], 1.0) == (5, 3)
    assert S.simulate_converge(*TABLES["never converges"], None) == (5, 3)
    assert S.simulate_converge(*TABLES["stopped table with NaN rows"], None) == (2, 1)
    # the float32 product, not the double one: 0.3 A is 300 mA, float32(300) * float32(1e-3) = 0.3000000119...
    t32 = float(F32(300) * F32(1e-3))
    assert t32 > 0.3 and S.simulate_converge([0.0, 1.0, 2.0], [np.inf, t32, 0.0], 0.3) == (2, 1)
    with pytest.raises(ValueError):
        S.simulate_converge([0.0], [np.inf], -1.0)


def test_random_tables_against_the_brute_force_rule():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 12))
        conf = np.round(rng.normal(size=n), 1).astype(np.float32)             # rounded: ties happen
        delta = np.abs(rng.normal(size=n)).astype(np.float32)
        delta[0] = np.inf
        delta[rng.random(n) < 0.1] = np.nan
        tol = float(rng.choice([0.0, 0.05, 0.1, 0.2, 0.5, 1.0, float(delta[int(rng.integers(n))])]))
        if tol != tol or tol == np.inf:
            tol = 0.3
        assert S.simulate_converge(conf, delta, tol) == _brute_force(conf, delta, tol)


# ---- the batch summary ----------------------------------------------------------------------------------------------------
def test_pass_summary_is_simulate_converge_on_every_table():
    from dmpfold2_amd import batch
    rng = np.random.default_rng(11)
    tables, raw = {}, {}
    for k, (R, rows) in enumerate([(7, 7), (7, 7), (7, 5), (3, 3)]):
        b = _block(R, rows, rng)
        b[16:].reshape(R, 8)[1:rows, 1] = np.abs(b[16:].reshape(R, 8)[1:rows, 1])       # deltas are not negative
        b[1] = S.simulate_converge(b[16:].reshape(R, 8)[:, 0], b[16:].reshape(R, 8)[:, 1], None)[1]
        b[4] = b[16:].reshape(R, 8)[int(b[2]), 2] - b[16:].reshape(R, 8)[int(b[1]), 2]
        raw[f"t{k}"] = S.unpack_pass_scores(b, R)
        tables[f"t{k}"] = S.pass_scores_json(raw[f"t{k}"])
    out = batch.pass_summary(tables)
    assert out["pass_scored_targets"] == 4
    assert out["best_is_tm_pass"] == np.mean([t["best_pass"] == t["tm_pass"] for t in raw.values()])
    assert out["mean_regret_tm"] == float(np.mean([t["regret_tm"] for t in raw.values()]))
    assert out["median_regret_lddt"] == float(np.median([t["regret_lddt"] for t in raw.values()]))
    assert len(out["mean_tm_by_pass"]) == 7
    for p in range(7):
        vals = [float(t["tm"][p]) for t in raw.values() if p < t["rows"]]
        assert out["mean_tm_by_pass"][p] == float(np.mean(vals)), p
    assert [s["tol"] for s in out["converge_sweep"]] == list(batch.CONVERGE_SWEEP) == [0.05, 0.1, 0.2, 0.5, 1.0]
    for s in out["converge_sweep"]:
        runs, lost = [], []
        for t in raw.values():
            run, best = S.simulate_converge(t["conf_mean"], t["delta"], s["tol"])
            runs.append(run)
            lost.append(float(t["tm"][t["best_pass"]]) - float(t["tm"][best]))
        assert s["mean_passes"] == float(np.mean(runs)) and s["mean_tm_lost"] == float(np.mean(lost)), s
    # the summary of --natives carries it beside the scores
    scores = {k: {"tm": 0.5, "gdt_ts": 0.4, "gdt_ha": 0.3, "rmsd": 2.0, "lddt": 0.6, "passes": v} for k, v in tables.items()}
    whole = batch.score_summary(scores)
    assert whole["converge_sweep"] == out["converge_sweep"] and whole["scored_targets"] == 4
    assert "converge_sweep" not in batch.score_summary({k: {kk: vv for kk, vv in v.items() if kk != "passes"} for k, v in scores.items()})


# ---- the front ends' arguments ----------------------------------------------------------------------------------------------
def test_the_flags_exist_and_need_a_native():
    from dmpfold2_amd import batch
    from dmpfold2_amd.predict import dmpfold_parser, Engine, Extras, agree_passes
    assert dmpfold_parser().parse_args(["-i", "x.aln", "--native", "x.pdb", "--score-passes"]).score_passes is True
    assert dmpfold_parser().parse_args(["-i", "x.aln"]).score_passes is False
    assert batch.batch_parser().parse_args(["-o", "out", "--natives", "d", "--score-passes"]).score_passes is True
    with pytest.raises(ValueError):
        batch.run_batch([], "out", score_passes=True)
    assert Extras._fields == ("distmap", "native", "structure", "library", "score_map", "score_passes", "ss", "exposure") and Extras().score_passes is False
    assert agree_passes([0, 0], True, 10) is None and agree_passes([1, 1], True, 10) == 11 and agree_passes([1], True, 500) == 128
    for bad in ([1, 0], [0, 1]):
        with pytest.raises(RuntimeError):
            agree_passes(bad, True, 3)
    with pytest.raises(RuntimeError):
        agree_passes([1, 1], False, 3)

    class Stub:
        def __init__(self, **o):
            self.options, self.sets = dict({"score_native": 0, "score_passes": 0}, **o), []

        def get_option(self, name):
            return self.options[name]

        def set_option(self, name, value):
            self.sets.append((name, value))
            self.options[name] = value

    stub = Stub()
    with Engine._call_options(stub, None, Extras(native=np.zeros((8, 3), np.float32), score_passes=True)):
        assert stub.sets == [("score_native", 1), ("score_passes", 1)]            # the option it needs first
    assert stub.options == {"score_native": 0, "score_passes": 0} and stub.sets[2:] == [("score_passes", 0), ("score_native", 0)]
    with pytest.raises(ValueError):
        with Engine._call_options(stub, None, Extras(score_passes=True)):
            raise AssertionError("the body ran")


def test_abi_is_unchanged():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5
