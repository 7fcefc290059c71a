"""Every recycling pass scored against the native on the GPU (option "score_passes"; include/dmpfold_hip.h).

Row p of the pass block is what "score_native" gives for ca_pass[p]: it is compared with the float64 yardstick of
tests/test_score_cpu.py under the rule of tests/test_gpu_score.py (integer-derived outputs exactly, the others within one
float32 ulp), and with the score block of the same call bit for bit where the final trace is ca_pass[best_pass].  Its delta
is pass_delta[p] of option "recycle_tol_mA", bit for bit.  One-row synthetic alignments on the module's synthetic weights.
"""
import contextlib
import io
import json
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_rows
from test_score_cpu import compare_with_yardstick, yardstick
from test_gpu_score import GUARD, LENGTHS, _bits, _one_row, _perturbed_copy, _random_walk, _tensors, _write_pdb

pytestmark = pytest.mark.gpu

from dmpfold2_amd import score as S  # noqa: E402

SCORES = ("tm", "gdt_ts", "gdt_ha", "rmsd", "lddt")
DMP_ERR_ARG = -1


@pytest.fixture(scope="module")
def eng(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 300, 64)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


def _table(eng, aln, native, iterations, **kw):
    """One prediction with the pass table: (public outputs, the pass block's floats, unpack_pass_scores of it)."""
    out = eng.predict(aln, None, iterations, 0, native=native, score_passes=True, **kw)
    eng.sync_check()
    assert eng.get_option("score_passes") == 0 and eng.get_option("score_native") == 0
    block = eng.pass_block.cpu().numpy().copy()
    assert block.shape == (16 + 8 * min(iterations + 1, 128),)
    return out, block, eng.pass_scores


def _header_from_rows(block, rows, best_pass):
    """The header restated from the stored floats: float32 comparisons and one float32 subtraction."""
    R = (block.shape[0] - 16) // 8
    table = block[16:].reshape(R, 8)
    want = np.zeros(16, dtype=np.float32)
    want[0], want[1] = rows, best_pass
    for q, col in enumerate((2, 6)):
        top = None
        for p in range(rows):
            v = table[p, col]
            if v == v and (top is None or v > table[top, col]):
                top = p
        want[2 + q] = np.nan if top is None else top
        vb = table[best_pass, col] if best_pass < rows else np.float32(np.nan)
        want[4 + q] = np.float32(table[top, col] - vb) if top is not None and vb == vb else np.nan
    return want


def _check_header(block, rows, best_pass, tag):
    want = _header_from_rows(block, rows, best_pass)
    assert np.array_equal(block[:16], want, equal_nan=True), (tag, block[:16], want)
    table = block[16:].reshape(-1, 8)
    assert np.isnan(table[rows:]).all() and (table[:rows, 7] == 0.0).all() and (block[6:16] == 0.0).all(), tag
    assert np.isinf(table[0, 1]) and table[0, 1] > 0, tag


# ------------------------------------------------------------------------------------------------ 1. rows against the yardstick
_PLAIN = {}


def _plain_model(eng, L):
    if L not in _PLAIN:
        aln = _one_row(L)
        coords, confs = eng.predict(aln, None, 2, 0)
        eng.sync_check()
        _PLAIN[L] = (aln, coords.clone(), confs.clone())
    return _PLAIN[L]


@pytest.mark.parametrize("kind", ["perturbed_copy", "random_walk"])
@pytest.mark.parametrize("L", LENGTHS)
def test_rows_against_the_yardstick(eng, L, kind):
    """nloops = 2: three rows, each the yardstick's answer for the trace ca_pass holds for that pass (fetched through
    dmp_debug_fetch), under compare_with_yardstick and its margin rule - the fields a row does not carry are handed over
    from the yardstick itself, so the function compares exactly the five scores.  conf_mean is conf_means[p], bit for bit.
    The perturbed copies run with lnorm 0, the random walks with a given lnorm."""
    aln, coords0, confs0 = _plain_model(eng, L)
    model = coords0[:, 1].cpu().numpy()
    native = _perturbed_copy(model, 100 + L) if kind == "perturbed_copy" else _random_walk(L, 200 + L)
    lnorm = 0.0 if kind == "perturbed_copy" else float(L + 3)
    (coords, confs), block, ps = _table(eng, aln, (native, lnorm), 2)
    assert torch.equal(coords, coords0) and torch.equal(confs, confs0)
    ca_pass = eng.fetch("ca_pass", 3 * L * 3).cpu().numpy().reshape(3, L, 3)
    conf_means = eng.fetch("conf_means", 3).cpu().numpy()
    assert ps["rows"] == 3 and ps["R"] == 3 and eng.passes_run == 3
    assert np.array_equal(_bits(ps["conf_mean"]), _bits(conf_means))
    for p in range(3):
        want, margin = yardstick(ca_pass[p], native, lnorm)
        got = dict(want)
        got.update({name: float(ps[name][p]) for name in SCORES})
        seen = compare_with_yardstick(got, want, margin, f"L={L} {kind} pass {p}")
        print(f"L={L} {kind} pass {p}: margin {margin:.2e} A, tm {ps['tm'][p]:.6f}, ulps", {k: seen[k] for k in ("tm", "rmsd")},
              file=sys.stderr)
    best = S.simulate_converge(conf_means, ps["delta"], None)[1]
    assert ps["best_pass"] == best
    _check_header(block, 3, best, (L, kind))


# ------------------------------------------------------------------------------------------------ 2. row = score block
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_row_of_the_kept_pass_is_the_score_block(eng, precision):
    """minsteps = 0: predict_end_refine does nothing, the final trace is ca_pass[best_pass] (asserted, not assumed), and the
    row of that pass has the bits of the score block of the same call."""
    L = 65
    aln = _one_row(L)
    native = _random_walk(L, 21)
    native[::9] = np.nan
    eng.set_option("precision", precision)
    try:
        (coords, confs), block, ps = _table(eng, aln, native, 3)
        sblock = eng.score_block.cpu().numpy().copy()
        ca_pass = eng.fetch("ca_pass", 4 * L * 3).cpu().numpy().reshape(4, L, 3)
    finally:
        eng.set_option("precision", 2)
    b = ps["best_pass"]
    assert ps["rows"] == 4 and 0 <= b < 4
    assert np.array_equal(_bits(coords[:, 1].contiguous()), _bits(ca_pass[b])), "the final trace is not ca_pass[best_pass]"
    h = sblock[3 * L:]
    want = np.array([h[3], h[4], h[5], h[2], h[6]], dtype=np.float32)          # tm, gdt_ts, gdt_ha, rmsd, lddt
    got = block[16 + 8 * b + 2:16 + 8 * b + 7]
    assert not np.isnan(want).any()
    assert np.array_equal(_bits(got), _bits(want)), (precision, b, got, want)
    _check_header(block, 4, b, precision)


# ------------------------------------------------------------------------------------------------ 3. delta
def test_delta_is_the_convergence_options(eng):
    L = 64
    aln = _one_row(L)
    native = _random_walk(L, 31)
    _, block1, ps1 = _table(eng, aln, native, 4, converge=1e-3)                # "recycle_tol_mA" = 1
    assert eng.passes_run == 5, "the run stopped early: raise nloops or lower the tolerance in this test"
    delta = eng.fetch("pass_delta", 5).cpu().numpy()
    assert delta.shape == (5,) and np.isinf(delta[0]) and (delta[1:] > 0).all()
    assert np.array_equal(_bits(ps1["delta"]), _bits(delta)), (ps1["delta"], delta)
    _, block0, ps0 = _table(eng, aln, native, 4)                                # the tolerance 0: recycle_delta never ran
    assert eng.fetch("pass_delta", 5).numel() == 0
    assert np.array_equal(_bits(ps0["delta"]), _bits(delta))
    assert np.array_equal(_bits(block0), _bits(block1))


# ------------------------------------------------------------------------------------------------ 4. simulate_converge
def test_simulate_converge_predicts_a_real_stop(eng):
    L, nloops = 96, 6
    aln = _one_row(L)
    native = _random_walk(L, 41)
    _, full, ps = _table(eng, aln, native, nloops)
    assert ps["rows"] == nloops + 1
    inner = np.sort(np.unique(ps["delta"][1:nloops].astype(np.float64)))       # passes 1 .. nloops - 1: a stop strictly inside
    assert inner.size >= 2, ps["delta"]
    tol_mA = int(round(0.5 * (inner[0] + inner[1]) * 1000.0))
    assert inner[0] < tol_mA * 1e-3 < inner[1] and tol_mA >= 1, (inner, tol_mA)
    tol = tol_mA * 1e-3
    run, best = S.simulate_converge(ps["conf_mean"], ps["delta"], tol)
    assert 2 <= run <= nloops, (run, ps["delta"], tol)
    (coords, confs, dm, info), stopped, ps2 = _table(eng, aln, native, nloops, converge=tol, distmap=True)
    print("deltas", ps["delta"], "tolerance", tol, "predicted", (run, best), "ran", eng.passes_run, info.tolist(), file=sys.stderr)
    assert eng.passes_run == run and int(info[1].item()) == run and int(info[0].item()) == best
    assert ps2["rows"] == run and ps2["best_pass"] == best and stopped.shape == full.shape
    assert np.array_equal(_bits(stopped[16:16 + 8 * run]), _bits(full[16:16 + 8 * run]))
    assert np.isnan(stopped[16 + 8 * run:]).all()
    _check_header(stopped, run, best, "stopped")


# ------------------------------------------------------------------------------------------------ 5. chunks
def test_chunk_boundaries_change_no_bit(eng):
    L = 33
    aln = _one_row(L)
    native = _perturbed_copy(_plain_model(eng, L)[1][:, 1].cpu().numpy(), 51)
    blocks = []
    try:
        for chunk in (0, 1, 2, 5):
            eng.set_option("score_passes_chunk", chunk)
            assert eng.get_option("score_passes_chunk") == chunk
            blocks.append(_table(eng, aln, native, 4)[1])
    finally:
        eng.set_option("score_passes_chunk", 0)
    assert not np.isnan(blocks[0][16:].reshape(5, 8)[:, :7][:, [0, 2, 3, 4, 5, 6]]).any()
    for b in blocks[1:]:
        assert np.array_equal(_bits(b), _bits(blocks[0]))


# ------------------------------------------------------------------------------------------------ 6. the cap
def test_more_passes_than_rows(eng):
    """131 passes, 128 rows: nothing is written behind 16 + 8 * 128 floats (a guard pattern lies there)."""
    L, nloops = 8, 130
    aln = _one_row(L)
    native = _random_walk(L, 61)
    lay = S.Layout(L, True, True, passes=S.pass_rows(nloops))
    assert lay.passes == 128 and lay.total == lay.pass_off + 16 + 8 * 128
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.zeros((L, 5, 3), dtype=torch.float32, device=eng.device)
    buf = torch.full((lay.total + GUARD,), 7.0, dtype=torch.float32, device=eng.device)
    buf[lay.score_off:lay.mapscore_off] = torch.from_numpy(S.pack_native(native, 0.0, L)).to(eng.device)
    for k in ("emit_distmap", "score_native", "score_passes"):
        eng.set_option(k, 1)
    try:
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, nloops, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
        assert rc == 0, eng.lib.dmp_last_error()
        eng.sync_check()
    finally:
        for k in ("score_passes", "score_native", "emit_distmap"):
            eng.set_option(k, 0)
    h = buf.cpu().numpy()
    assert (h[lay.total:] == 7.0).all(), "a write went past the pass block"
    out = lay.split(h[:lay.total])
    assert out.info[1] == 131.0 and eng.passes_run == 131
    ps = S.unpack_pass_scores(out.pass_block, 128)
    best = int(out.info[0])
    assert ps["rows"] == 128 and out.pass_block[1] == out.info[0] and not np.isnan(out.pass_block[16:].reshape(128, 8)[:, 2]).any()
    if best >= 128:
        assert np.isnan(ps["regret_tm"]) and np.isnan(ps["regret_lddt"]) and ps["tm_pass"] is not None
    else:
        assert ps["regret_tm"] >= 0.0 and ps["regret_lddt"] >= 0.0
    _check_header(out.pass_block, 128, best, "cap")


# ------------------------------------------------------------------------------------------------ 7. off means off
def test_off_means_off(eng, synth_sd):
    from dmpfold2_amd.predict import Engine
    L = 65
    aln = _one_row(L)
    native = _random_walk(L, 71)
    native[::8] = np.nan
    structure = _random_walk(70, 72)
    library = S.Library.from_traces([_random_walk(m, 73 + m) for m in (40, 65, 70)])
    kw = dict(distmap=True, native=native, structure=structure, library=library, score_map=True)
    fields = ("confs", "distmap", "info", "score_block", "map_block", "pass_block", "align_block", "search_block")

    def run(passes):
        eng.predict(aln, None, 2, 0, score_passes=passes, **kw)
        eng.sync_check()
        out = eng._last.out
        return {f: getattr(out, f).cpu().numpy().reshape(-1).copy() for f in fields if getattr(out, f) is not None}

    mib0 = eng.get_option("device_mib")
    off1, on, off2 = run(False), run(True), run(False)
    assert "pass_block" not in off1 and on["pass_block"].shape == (16 + 8 * 3,)
    lay = S.Layout(L, True, True, True, 70, (3, library.rows), eng.max_L)
    assert sum(v.size for v in off1.values()) == lay.total and sum(v.size for v in on.values()) == lay._replace(passes=3).total
    for f in off1:
        assert np.array_equal(_bits(off1[f]), _bits(off2[f])), f
        assert np.array_equal(_bits(off1[f]), _bits(on[f])), f
    assert not np.isnan(on["pass_block"][16:].reshape(3, 8)[:, :7]).any()
    # the scratch: allocated when the option first became 1 on this context, counted, and never on a context that did not
    assert eng.get_option("device_mib") >= mib0
    other = Engine("cuda:0", 65, 1)
    try:
        other.set_weights(_tensors(synth_sd))
        before = other.get_option("device_mib")
        other.predict(aln, None, 1, 0, native=native)
        other.sync_check()
        assert other.get_option("device_mib") == before
        other.set_option("score_passes", 1)
        assert other.get_option("device_mib") > before
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------ 8. errors, degenerate natives
def test_errors_and_degenerate_natives(eng):
    from dmpfold2_amd import _lib
    for bad in (2, -1):
        with pytest.raises(_lib.DmpError):
            eng.set_option("score_passes", bad)
    with pytest.raises(_lib.DmpError):
        eng.set_option("score_passes_chunk", -1)
    assert eng.get_option("score_passes") == 0
    L = 33
    aln = _one_row(L)
    eng.set_option("score_passes", 1)
    try:
        d_msa = torch.from_numpy(aln).to(eng.device)
        coords = torch.zeros((L, 5, 3), dtype=torch.float32, device=eng.device)
        buf = torch.zeros((S.Layout(L, False, True, passes=2).total,), dtype=torch.float32, device=eng.device)
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 1, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
        message = eng.lib.dmp_last_error().decode()
        assert rc == DMP_ERR_ARG and "score_native" in message and "score_passes" in message, (rc, message)
        with pytest.raises(RuntimeError):                              # the Python layer says so before the library is asked
            eng.predict(aln, None, 1, 0)
    finally:
        eng.set_option("score_passes", 0)
    assert eng.sync_faults() == 0 and not bool(buf.any())
    walk = _random_walk(L, 81)
    _, full, ps_full = _table(eng, aln, walk, 2)
    few = np.full((L, 3), np.nan, dtype=np.float32)
    few[4:6] = walk[4:6]
    _, block, ps = _table(eng, aln, few, 2)
    assert eng.scores["n_pairs"] == 2
    table = block[16:].reshape(3, 8)
    assert np.isnan(table[:, 2:7]).all() and np.isnan(block[2:6]).all() and block[0] == 3.0 and (table[:, 7] == 0).all()
    assert np.array_equal(_bits(table[:, :2]), _bits(full[16:].reshape(3, 8)[:, :2]))
    assert ps["tm_pass"] is None and ps["best_pass"] == ps_full["best_pass"]


# ------------------------------------------------------------------------------------------------ 9. software-latched fault
def test_latched_fault_gives_nan_in_the_whole_block(eng):
    """A residue code of 22 raises the device-side flag DMP_FAULT_BAD_CODE (a software flag, not a GPU fault)."""
    from dmpfold2_amd.predict import FAULT_BAD_CODE
    L = 33
    aln = _one_row(L).copy()
    aln[0, 5] = 22
    native = _random_walk(L, 8)
    lay = S.Layout(L, False, True, passes=2)
    eng.set_option("score_native", 1)
    eng.set_option("score_passes", 1)
    try:
        d_msa = torch.from_numpy(aln).to(eng.device)
        coords = torch.zeros((L, 5, 3), dtype=torch.float32, device=eng.device)
        buf = torch.zeros((lay.total + GUARD,), dtype=torch.float32, device=eng.device)
        buf[lay.total:] = 7.0
        buf[lay.score_off:lay.score_off + 3 * L + 1] = torch.from_numpy(S.pack_native(native, 40.0, L)[:3 * L + 1]).to(eng.device)
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 1, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
        assert rc == 0
        assert eng.sync_faults() == FAULT_BAD_CODE
        h = buf.cpu().numpy()
        assert np.isnan(h[lay.pass_off:lay.total]).all() and lay.total - lay.pass_off == 32
        assert (h[lay.total:] == 7.0).all(), "the NaN fill went past the pass block"
    finally:
        eng.set_option("score_passes", 0)
        eng.set_option("score_native", 0)
    _, block, ps = _table(eng, _one_row(L), native, 1)               # the next prediction on the engine is whole again
    assert ps["rows"] == 2 and not np.isnan(block[16:].reshape(2, 8)[:, :7]).any()


# ------------------------------------------------------------------------------------------------ 10. pipeline
def test_pipeline(synth_sd):
    """Four submissions of different depth and length through two streams: every ticket's pass block has its own R and is
    bit for bit the lone engine's."""
    from dmpfold2_amd.predict import Engine, Pipeline
    depths, lengths = [0, 1, 3, 3], [8, 63, 64, 96]
    alns = [_one_row(L) for L in lengths]
    natives = []
    for k, L in enumerate(lengths):
        nat = _random_walk(L, 400 + k)
        nat[k + 1::6] = np.nan
        natives.append((nat, float(L + k)))
    dev = torch.device("cuda:0")
    sdt = _tensors(synth_sd)
    single = Engine(dev, 96, 1)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 96, 1, sdt, streams=2, precision=2, score_passes=True)
    try:
        assert all(e.get_option("score_passes") == 1 and e.get_option("score_native") == 1 for e in pipe.engines)
        refs = []
        for aln, nat, n in zip(alns, natives, depths):
            c, f = single.predict(aln, None, n, 0, native=nat, score_passes=True)
            single.sync_check()
            refs.append((c.clone(), f.clone(), single.score_block.clone(), single.pass_block.clone()))
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), n, 0, native=nat) for a, nat, n in zip(alns, natives, depths)]
        res = pipe.collect(tickets)
        for t, ref, L, n in zip(tickets, refs, lengths, depths):
            assert not isinstance(res[t], Exception), res[t]
            coords, confs, sblock, pblock = res[t]
            assert tuple(pblock.shape) == (16 + 8 * (n + 1),) and tuple(sblock.shape) == (5 * L + 24,)
            assert torch.equal(coords, ref[0]) and torch.equal(confs, ref[1])
            assert np.array_equal(_bits(sblock), _bits(ref[2])) and np.array_equal(_bits(pblock), _bits(ref[3])), (L, n)
            assert S.unpack_pass_scores(pblock, n + 1)["rows"] == n + 1
        pipe.set_score_passes(False)
        t = pipe.submit(torch.from_numpy(alns[1]).to(dev), 1, 0, native=natives[1])
        out = pipe.collect([t])[t]
        assert len(out) == 3 and np.array_equal(_bits(out[2]), _bits(refs[1][2]))
    finally:
        pipe.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 11. front ends
def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --native --score-passes`: stdout byte for byte the run's without the flag, the JSON line gains "passes";
    aln_to_coords(return_pass_scores=True); `dmpfold-batch --natives --score-passes`: the summary's tables, its aggregates
    and its convergence sweep are what simulate_converge gives on the per-target tables."""
    import dmpfold2_amd.predict as P
    from dmpfold2_amd import aln_to_coords, run_dmpfold
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        paths, queries = [], {}
        for name, stem in (("pf10963_n3_m0", "pf"), ("synth_L40_N64_n2_m0", "s40")):
            rows = golden_rows(load_golden(name))
            p = tmp_path / f"{stem}.aln"
            p.write_text("\n".join(rows) + "\n")
            paths.append(str(p))
            queries[stem] = rows[0]
        natives = tmp_path / "natives"
        natives.mkdir()
        for stem, seed in (("pf", 77), ("s40", 78)):
            q = queries[stem]
            seq = q[2:30] + q[33:]
            _write_pdb(str(natives / f"{stem}.pdb"), seq, _random_walk(len(seq), seed))
        kw = dict(device="cuda:0", iterations=3, minsteps=0, weights_file=weights_file)
        plain = aln_to_coords(paths[0], **kw)
        c, f, sc, ps = aln_to_coords(paths[0], native=str(natives / "pf.pdb"), return_scores=True, return_pass_scores=True, **kw)
        assert torch.equal(c, plain[0]) and torch.equal(f, plain[1])
        assert ps["rows"] == 4 and ps["R"] == 4 and not np.isnan(ps["tm"]).any()
        assert np.float32(ps["tm"][ps["best_pass"]]) == np.float32(sc["tm"])          # minsteps 0: the kept pass's row
        with pytest.raises(ValueError):
            aln_to_coords(paths[0], return_pass_scores=True, **kw)
        want = dict(S.scores_json(sc), passes=S.pass_scores_json(ps))
        args = ["-i", paths[0], "-d", "cuda:0", "-n", "3", "-m", "0", "-w", weights_file, "--native", str(natives / "pf.pdb")]
        texts, errs = [], []
        for extra in ([], ["--score-passes"]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1]
        assert "passes" not in json.loads(errs[0].strip().split("\n")[-1])
        assert json.loads(errs[1].strip().split("\n")[-1]) == want
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i"] + paths + ["-o", str(out_dir), "-n", "3", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--natives", str(natives), "--score-passes"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["scored_targets"] == 2 and summary["pass_scored_targets"] == 2
            assert set(summary["scores"]["pf"]) == set(want) and set(summary["scores"]["pf"]["passes"]) == set(want["passes"])
            tables = {stem: S.pass_scores_from_json(summary["scores"][stem]["passes"]) for stem in ("pf", "s40")}
            assert summary["best_is_tm_pass"] == np.mean([t["best_pass"] == t["tm_pass"] for t in tables.values()])
            assert summary["mean_regret_tm"] == float(np.mean([t["regret_tm"] for t in tables.values()]))
            assert summary["median_regret_lddt"] == float(np.median([t["regret_lddt"] for t in tables.values()]))
            assert summary["mean_tm_by_pass"] == [float(np.mean([float(t["tm"][p]) for t in tables.values()])) for p in range(4)]
            assert [s["tol"] for s in summary["converge_sweep"]] == [0.05, 0.1, 0.2, 0.5, 1.0]
            for s in summary["converge_sweep"]:
                sims = [S.simulate_converge(t["conf_mean"], t["delta"], s["tol"]) for t in tables.values()]
                assert s["mean_passes"] == float(np.mean([run for run, _ in sims]))
                assert s["mean_tm_lost"] == float(np.mean([float(t["tm"][t["best_pass"]]) - float(t["tm"][best])
                                                           for t, (_, best) in zip(tables.values(), sims)]))
            for stem, t in tables.items():
                assert t["rows"] == 4 and t["R"] == 4 and not np.isnan(t["tm"]).any()
                if fmt == "pdb":
                    assert json.loads((out_dir / f"{stem}.scores.json").read_text()) == summary["scores"][stem]
                else:
                    z = np.load(str(out_dir / f"{stem}.npz"))
                    assert int(z["pass_rows"]) == 4 and int(z["pass_best"]) == t["best_pass"] and int(z["pass_tm_best"]) == t["tm_pass"]
                    for name in S.PASS_COLUMNS:
                        assert np.array_equal(_bits(z["pass_" + name]), _bits(t[name])), name
                    assert np.float32(z["pass_regret_tm"]) == np.float32(t["regret_tm"])
                    assert np.float32(z["tm"]) == t["tm"][t["best_pass"]]          # minsteps 0: the kept pass's row
    finally:
        P._ENGINES.clear()
