"""The predicted distance map scored against the native on the GPU (option "score_map"; include/dmpfold_hip.h).

Every number is compared with the yardstick of tests/test_mapscore_cpu.py, fed the float32 map the GPU returned and the
same native: every count exactly, map_lddt, map_mae, map_rmse, map_bias and the per-residue values within one float32
ulp (why: compare_with_yardstick there).  Before a comparison the native's near-tie margin is checked on the CPU and
another seed drawn if a pair lies within it - twice at the most.

On the parent commit every test here fails: the option "score_map" and the `score_map` arguments are unknown.
"""
import contextlib
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_score import GUARD, _bits, _one_row, _perturbed_copy, _random_walk, _tensors
from test_mapscore_cpu import NEAR_TIE, compare_with_yardstick, yardstick

pytestmark = pytest.mark.gpu

from dmpfold2_amd import score as S  # noqa: E402

LENGTHS = [8, 25, 33, 64, 65, 257]
# the tie-heavy head: resnet.17.weight times 2^-shrink, the distance channel's bias 5.  profiles/mapscore.txt has the sweep
# these were chosen from: every shrink up to 2^-30 gives a finite prediction; 30, the largest, leaves ONE map value - every
# candidate tied, the lists are decided by (i, j) alone; 16 leaves 371 values shared by 91 % of the candidates - ties and
# distinct values side by side in every list
TIE_SHRINKS = [30, 16]


@pytest.fixture(scope="module")
def eng(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 300, 256)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


@contextlib.contextmanager
def _precision(eng, p):
    eng.set_option("precision", p)
    try:
        yield
    finally:
        eng.set_option("precision", 2)


def _map_scored(eng, aln, native, iterations=0, minsteps=0, **kw):
    """((coords, confs, dm, info), map scores) of a prediction with `native` and `score_map`; the options are off afterwards."""
    out = eng.predict(aln, None, iterations, minsteps, distmap=True, native=native, score_map=True, **kw)
    eng.sync_check()
    assert [eng.get_option(k) for k in ("emit_distmap", "score_native", "score_map")] == [0, 0, 0]
    return out, eng.map_scores


def _native_clear_of_ties(dm, make, seed, tag):
    """make(seed + 1000 k), k = 0, 1, 2: the first whose margin against `dm` is not a near tie."""
    for k in range(3):
        native = make(seed + 1000 * k)
        want, margin = yardstick(dm, native[0] if isinstance(native, tuple) else native,
                                 native[1] if isinstance(native, tuple) else 0.0)
        if margin >= NEAR_TIE:
            return native, want, margin
        print(tag, "near tie, margin %.3e A: another seed" % margin, file=sys.stderr)
    pytest.fail(f"{tag}: three natives in a row with a pair within {NEAR_TIE} A of a threshold")


def _check(ms, dm, native, lnorm, want, margin, tag):
    again, m2 = yardstick(dm.cpu().numpy(), native, lnorm)          # the map the GPU returned is the one the native was chosen on
    assert m2 == margin and again["pairs"] == want["pairs"]
    seen = compare_with_yardstick(ms, again, margin, tag)
    print(tag, "margin %.2e A, largest differences in float32 ulps:" % margin, seen, "map_lddt %.4f mae %.3f" %
          (ms["map_lddt"], ms["map_mae"]), {c: (ms["classes"][c]["hits"], ms["classes"][c]["taken"]) for c in S.MAP_CLASSES},
          file=sys.stderr)


_PLAIN = {}


def _plain(eng, L, precision=2):
    """The prediction of the one-row alignment of length L with the map alone, made once: (aln, coords, confs, dm, info)."""
    if (L, precision) not in _PLAIN:
        aln = _one_row(L)
        with _precision(eng, precision):
            out = eng.predict(aln, None, 0, 0, distmap=True)
            eng.sync_check()
        _PLAIN[(L, precision)] = (aln,) + tuple(x.clone() for x in out)
    return _PLAIN[(L, precision)]


# ------------------------------------------------------------------------------------------------ 1. length sweep
def _sweep(eng, L, kind, precision):
    aln, coords0, confs0, dm0, info0 = _plain(eng, L, precision)
    model = coords0[:, 1].cpu().numpy()
    make = (lambda s: _perturbed_copy(model, s)) if kind == "perturbed_copy" else (lambda s: _random_walk(L, s))
    tag = f"sweep L={L} {kind} p{precision}"
    native, want, margin = _native_clear_of_ties(dm0.cpu().numpy(), make, 100 + L, tag)
    with _precision(eng, precision):
        (coords, confs, dm, info), ms = _map_scored(eng, aln, native)
    for a, b in ((coords, coords0), (confs, confs0), (dm, dm0), (info, info0)):
        assert torch.equal(a, b)
    _check(ms, dm, native, 0.0, want, margin, tag)
    assert ms["n"] == int((~np.isnan(native[:, 0])).sum())
    assert np.array_equal(np.isnan(ms["map_lddt_res"]), np.isnan(native[:, 0]))
    blk = eng.map_score_block.cpu().numpy()
    assert tuple(blk.shape) == (64 + L,) and (blk[55:64] == 0).all() and all((blk[12 + 12 * c:14 + 12 * c] == 0).all() for c in range(4))


@pytest.mark.parametrize("kind", ["perturbed_copy", "random_walk"])
@pytest.mark.parametrize("L", LENGTHS)
def test_length_sweep(eng, L, kind):
    """L = 8: three short candidates and nothing else; 25: one long pair; 33, 64, 65: one to four workgroups of the
    counting pass, the folded triangle of the long class with an odd and an even number of rows; 257: more rows than a
    workgroup has threads, more candidates than one batch of the selection."""
    _sweep(eng, L, kind, 2)


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_three_precisions_L65(eng, precision):
    _sweep(eng, 65, "perturbed_copy", precision)


# ------------------------------------------------------------------------------------------------ 2. recycling
def test_recycling_scores_the_chosen_pass(eng):
    """PF10963 at -n 3: the best-of rule takes pass 1 of 4; the scored map is that pass's - the one a run of -n 1 ends with -
    and lnorm is honoured."""
    aln = np.ascontiguousarray(load_golden("pf10963_n3_m0")["alnmat"])
    L = aln.shape[1]
    c1, f1, dm1, info1 = eng.predict(aln, None, 1, 0, distmap=True)
    eng.sync_check()
    dm1 = dm1.clone()
    make = lambda s: (np.where((np.arange(L) % 11 == 3)[:, None], np.nan, _random_walk(L, s)).astype(np.float32), float(L + 9))
    native, want, margin = _native_clear_of_ties(dm1.cpu().numpy(), make, 40, "pf10963 -n 3")
    (coords, confs, dm, info), ms = _map_scored(eng, aln, native, 3, 0)
    assert info[:2].tolist() == [1.0, 4.0] and eng.fetch("best_pass", 1).tolist() == [1.0] and eng.passes_run == 4
    assert torch.equal(dm, dm1) and torch.equal(eng.fetch("best_dm", L * L).view(L, L), dm)
    _check(ms, dm, native[0], native[1], want, margin, "pf10963 -n 3")
    assert ms["ln"] == float(L + 9) and ms["classes"]["long"]["taken"][0] == min(L + 9, ms["classes"]["long"]["candidates"])
    assert eng.scores["lnorm"] == float(L + 9)


# ------------------------------------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("shrink", TIE_SHRINKS)
def test_tie_heavy_map(synth_sd, shrink):
    """A head whose distance channel is 5 plus a term shrunk to a few float32 steps: the plain prediction is finite, at
    least a quarter of the candidates share their map value with another pair, and every list is still the yardstick's -
    the lower (i, j) first."""
    from dmpfold2_amd.predict import Engine
    L = 64
    sd = dict(synth_sd)
    w = np.array(sd["resnet.17.weight"], dtype=np.float32) * np.float32(2.0 ** -shrink)
    b = np.array(sd["resnet.17.bias"], dtype=np.float32)
    b[0] = 5.0
    sd["resnet.17.weight"], sd["resnet.17.bias"] = w, b
    e = Engine("cuda:0", L, 1)
    try:
        e.set_weights(_tensors(sd))
        e.set_option("precision", 2)
        aln = _one_row(L)
        coords0, confs0, dm0, _ = e.predict(aln, None, 0, 0, distmap=True)
        e.sync_check()
        assert bool(torch.isfinite(coords0).all()) and bool(torch.isfinite(confs0).all()) and bool(torch.isfinite(dm0).all())
        h = dm0.cpu().numpy()
        i, j = np.triu_indices(L, 6)
        _, counts = np.unique(h[i, j], return_counts=True)
        shared = int(counts[counts > 1].sum()) / i.size
        print(f"tie-heavy map, shrink 2^-{shrink}: {shared:.3f} of {i.size} candidates share their value, "
              f"{counts.size} distinct values, range [{h[i, j].min()}, {h[i, j].max()}]", file=sys.stderr)
        assert shared >= 0.25
        # natives with contacts at every separation: a compact walk
        make = lambda s: (_random_walk(L, s, step=2.0, clash=1.5), 0.0)
        native, want, margin = _native_clear_of_ties(h, make, 7, f"ties 2^-{shrink}")
        (coords, confs, dm, info), ms = _map_scored(e, aln, native)
        assert torch.equal(dm, dm0) and torch.equal(coords, coords0)
        _check(ms, dm, native[0], 0.0, want, margin, f"ties 2^-{shrink}")
        assert ms["classes"]["medium_long"]["native_contacts"] > 0 and ms["classes"]["short"]["predicted"] > 0
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. invariance
def test_invariance_and_raw_buffer(eng):
    """With the option on the coordinates, confidences, map, info and score block are bit for bit those of the run without
    it; with "align_structure" and "search_structures" on as well, so are their blocks; two runs give the same bits; a raw
    dmp_predict writes conf_floats(L, True, True, None, True) floats and not one more."""
    L = 65
    aln, coords0, confs0, dm0, info0 = _plain(eng, L)
    native = _random_walk(L, 21)
    native[::9] = np.nan
    structure = _random_walk(40, 22)
    library = S.Library.from_traces([_random_walk(m, 23 + m) for m in (12, 30, 57)])
    kw = dict(distmap=True, native=(native, 70.0), structure=structure, library=library)
    ref = eng.predict(aln, None, 0, 0, **kw)
    eng.sync_check()
    ref_blocks = [x.clone() for x in (eng.score_block, eng.align_block, eng.search_block)]
    assert eng.map_scores is None and eng.map_score_block is None
    runs = []
    for _ in range(2):
        out = eng.predict(aln, None, 0, 0, score_map=True, **kw)
        eng.sync_check()
        for a, b in zip(out, (coords0, confs0, dm0, info0)):
            assert torch.equal(a, b)
        for name, a, b in zip(("score", "align", "search"), (eng.score_block, eng.align_block, eng.search_block), ref_blocks):
            assert np.array_equal(_bits(a), _bits(b)), name
        base = out[1].data_ptr()
        assert eng.map_score_block.data_ptr() == base + 4 * S.mapscore_offset(L)
        assert eng.align_block.data_ptr() == base + 4 * S.align_offset(L, True, True, True)
        assert eng.search_block.data_ptr() == base + 4 * S.search_offset(L, True, True, 40, eng.max_L, True)
        runs.append(eng.map_score_block.clone())
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
    assert [eng.get_option(k) for k in ("emit_distmap", "score_native", "score_map", "align_structure", "search_structures")] == [0] * 5
    want, margin = yardstick(dm0.cpu().numpy(), native, 70.0)
    compare_with_yardstick(S.unpack_map_scores(runs[0], L), want, margin, "invariance L=65")
    # the raw call into a poisoned buffer
    n_out = S.conf_floats(L, True, True, None, True)
    d_msa = torch.from_numpy(aln).to(eng.device)
    raw_c = torch.full((15 * L + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    buf = torch.full((n_out + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    s0 = S.score_offset(L, True)
    buf[s0:s0 + S.score_floats(L)] = torch.from_numpy(S.pack_native(native, 70.0, L)).to(eng.device)
    for k in ("emit_distmap", "score_native", "score_map"):
        eng.set_option(k, 1)
    try:
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 0, 0, raw_c.data_ptr(), buf.data_ptr(), eng.stream())
        assert rc == 0, eng.lib.dmp_last_error()
        eng.sync_check()
    finally:
        for k in ("score_map", "score_native", "emit_distmap"):
            eng.set_option(k, 0)
    assert bool(torch.isnan(buf[n_out:]).all()) and bool(torch.isnan(raw_c[15 * L:]).all()), "a guard float was written"
    whole = np.concatenate([_bits(x) for x in (confs0, dm0, info0, ref_blocks[0], runs[0])])
    assert whole.size == n_out and np.array_equal(_bits(buf[:n_out]), whole)


def test_too_few_rows(eng):
    """No row and one row present: the counts are 0, offsets 51 .. 54 NaN, the per-residue values NaN where the row is
    absent and 0 where the one row is, no fault; two rows six columns apart are a short candidate."""
    L = 33
    aln = _plain(eng, L)[0]
    walk = _random_walk(L, 5)
    for keep in (0, 1):
        native = np.full((L, 3), np.nan, dtype=np.float32)
        native[4:4 + keep] = walk[4:4 + keep]
        _, ms = _map_scored(eng, aln, native)
        blk = eng.map_score_block.cpu().numpy()
        assert blk[0] == float(keep) == blk[1] and (blk[2:51] == 0).all() and np.isnan(blk[51:55]).all() and (blk[55:64] == 0).all()
        assert np.array_equal(np.isnan(blk[64:]), np.isnan(native[:, 0])) and (blk[64:][~np.isnan(native[:, 0])] == 0).all()
    native = np.full((L, 3), np.nan, dtype=np.float32)
    native[[4, 10]] = walk[[4, 5]]
    (_, _, dm, _), ms = _map_scored(eng, aln, native)
    want, margin = yardstick(dm.cpu().numpy(), native)
    assert margin >= NEAR_TIE and want["classes"]["short"]["candidates"] == 1 and want["pairs"] == 2
    compare_with_yardstick(ms, want, margin, "two rows")


# ------------------------------------------------------------------------------------------------ 5. pipeline
def test_pipeline_ticket_equals_engine(synth_sd):
    """Four targets of mixed length through a two-stream pipeline with `score_map`: every part of every ticket is bit for
    bit the lone engine's ("tridiag_cluster" 0, as the scheduler's engines); set_score_map turns the two options it needs
    on; a target without a native reads n = 0; with the option off `result` has its old shape."""
    from dmpfold2_amd.predict import Engine, Pipeline
    lengths = [40, 25, 64, 33]
    alns = [_one_row(L) for L in lengths]
    natives = []
    for k, L in enumerate(lengths):
        nat = _random_walk(L, 300 + k)
        nat[k::6] = np.nan
        natives.append((nat, float(L + k)))
    dev, sdt = torch.device("cuda:0"), _tensors(synth_sd)
    single = Engine(dev, 64, 1)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 64, 1, sdt, streams=2, precision=2, score_map=True)
    try:
        assert all([e.get_option(k) for k in ("emit_distmap", "score_native", "score_map")] == [1, 1, 1] for e in pipe.engines)
        refs = []
        for aln, nat in zip(alns, natives):
            out = single.predict(aln, None, 1, 0, distmap=True, native=nat, score_map=True)
            single.sync_check()
            refs.append(tuple(x.clone() for x in out) + (single.score_block.clone(), single.map_score_block.clone()))
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), 1, 0, native=n) for a, n in zip(alns, natives)]
        res = pipe.collect(tickets)
        for t, ref, L in zip(tickets, refs, lengths):
            assert not isinstance(res[t], Exception), res[t]
            assert [tuple(x.shape) for x in res[t]] == [(L, 5, 3), (L,), (L, L), (3,), (5 * L + 24,), (64 + L,)]
            for name, a, b in zip(("coords", "confs", "distmap", "info", "score block", "map-score block"), res[t], ref):
                assert np.array_equal(_bits(a), _bits(b)), (L, name)
        t = pipe.submit(torch.from_numpy(alns[1]).to(dev), 1, 0)
        pipe.drain()
        pipe.sync_check()
        ms = S.unpack_map_scores(pipe.result(t)[-1], lengths[1])
        assert ms["n"] == 0 and np.isnan(ms["map_lddt"]) and ms["classes"]["short"]["candidates"] == 0
        pipe.set_score_map(False)
        assert all([e.get_option(k) for k in ("emit_distmap", "score_native", "score_map")] == [1, 1, 0] for e in pipe.engines)
        out = pipe.run([torch.from_numpy(alns[2]).to(dev)], 1, 0)
        pipe.sync_check()
        assert len(out[0]) == 5 and np.array_equal(_bits(out[0][2]), _bits(refs[2][2]))
    finally:
        pipe.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_and_abi(eng):
    """"score_map" takes 0 or 1; a prediction begun with it on and "emit_distmap" or "score_native" off fails with
    DMP_ERR_ARG and names the missing option; nothing was added to the C interface."""
    from dmpfold2_amd import _lib
    for bad in (2, -1):
        with pytest.raises(_lib.DmpError, match="score_map"):
            eng.set_option("score_map", bad)
    assert eng.get_option("score_map") == 0
    aln = _plain(eng, 33)[0]
    eng.set_option("score_map", 1)
    try:
        assert eng.get_option("score_map") == 1
        with pytest.raises(_lib.DmpError, match="emit_distmap"):
            eng.predict(aln, None, 0, 0)
        eng.set_option("emit_distmap", 1)
        with pytest.raises(_lib.DmpError, match="score_native"):
            eng.predict(aln, None, 0, 0)
        eng.set_option("emit_distmap", 0)
        eng.set_option("score_native", 1)
        with pytest.raises(_lib.DmpError, match="emit_distmap"):
            eng.predict(aln, None, 0, 0)
    finally:
        for k in ("score_map", "score_native", "emit_distmap"):
            eng.set_option(k, 0)
    with pytest.raises(ValueError, match="native"):
        eng.predict(aln, None, 0, 0, score_map=True)
    coords, confs = eng.predict(aln, None, 0, 0)                       # the engine is whole afterwards
    eng.sync_check()
    assert torch.equal(coords, _plain(eng, 33)[1]) and eng.map_scores is None
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5 and eng.lib.dmp_abi_version() == 5


# ------------------------------------------------------------------------------------------------ 7. software-latched fault
def test_latched_fault_gives_nan_in_every_slot(eng):
    """A residue code of 22 raises the device-side flag DMP_FAULT_BAD_CODE (a software flag, not a GPU fault), as in
    test_gpu_score.py: every slot of the map-score block is NaN, the score block's inputs are as the caller wrote them,
    the guard stays; the next prediction on the engine is whole."""
    from dmpfold2_amd.predict import FAULT_BAD_CODE
    L = 33
    aln = _one_row(L).copy()
    aln[0, 5] = 22
    native = _random_walk(L, 8)
    native[3] = np.nan
    n_out = S.conf_floats(L, True, True, None, True)
    s0, m0 = S.score_offset(L, True), S.mapscore_offset(L)
    inputs = S.pack_native(native, 40.0, L)[:3 * L + 1]
    for k in ("emit_distmap", "score_native", "score_map"):
        eng.set_option(k, 1)
    try:
        d_msa = torch.from_numpy(aln).to(eng.device)
        coords = torch.zeros((L, 5, 3), dtype=torch.float32, device=eng.device)
        buf = torch.zeros((n_out + GUARD,), dtype=torch.float32, device=eng.device)
        buf[n_out:] = 7.0
        buf[s0:s0 + 3 * L + 1] = torch.from_numpy(inputs).to(eng.device)
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 1, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
        assert rc == 0
        assert eng.sync_faults() == FAULT_BAD_CODE
        h = buf.cpu().numpy()
        assert bool(torch.isnan(coords).all()) and np.isnan(h[:s0]).all()
        assert np.array_equal(h[s0:s0 + 3 * L + 1], inputs, equal_nan=True), "the inputs were touched"
        assert np.isnan(h[s0 + 3 * L + 1:m0]).all() and np.isnan(h[m0:n_out]).all() and m0 + 64 + L == n_out
        assert (h[n_out:] == 7.0).all(), "the NaN fill went past the map-score block"
    finally:
        for k in ("score_map", "score_native", "emit_distmap"):
            eng.set_option(k, 0)
    (_, _, dm, _), ms = _map_scored(eng, _one_row(L), native)
    want, margin = yardstick(dm.cpu().numpy(), native)
    compare_with_yardstick(ms, want, margin, "after a fault L=33")
    assert ms["n"] == L - 1


# ------------------------------------------------------------------------------------------------ 8. front ends
def test_front_ends(tmp_path, weights_file, monkeypatch):
    """aln_to_coords(native=, return_map_scores=True) and `dmpfold --native --score-map`: the model on standard output is
    byte for byte the run's without the flag, the JSON line gains the key "map" with the numbers of Engine.map_scores;
    `dmpfold-batch --natives --score-map`: the summary, the npz arrays and <stem>.scores.json carry the same numbers."""
    import io
    import json
    import dmpfold2_amd.predict as P
    from conftest import golden_rows
    from dmpfold2_amd import aln_to_coords, batch, run_dmpfold
    from test_gpu_score import _write_pdb
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        rows = golden_rows(load_golden("synth_L40_N64_n2_m0"))
        path = tmp_path / "s40.aln"
        path.write_text("\n".join(rows) + "\n")
        natives = tmp_path / "natives"
        natives.mkdir()
        seq = rows[0][1:31] + rows[0][33:]
        _write_pdb(str(natives / "s40.pdb"), seq, _random_walk(len(seq), 77, step=3.0, clash=2.0))
        kw = dict(device="cuda:0", iterations=1, minsteps=0, weights_file=weights_file)
        plain = aln_to_coords(str(path), native=str(natives / "s40.pdb"), return_scores=True, **kw)
        c, f, dm, sc, ms = aln_to_coords(str(path), native=str(natives / "s40.pdb"), return_scores=True, return_distmap=True,
                                         return_map_scores=True, **kw)
        assert torch.equal(c, plain[0]) and torch.equal(f, plain[1]) and S.scores_json(sc) == S.scores_json(plain[2])
        assert [P._ENGINES[0].get_option(k) for k in ("emit_distmap", "score_native", "score_map")] == [0, 0, 0]
        rows_nat, lnorm = S.native_from_pdb(rows[0], str(natives / "s40.pdb"))
        want, margin = yardstick(dm.cpu().numpy(), rows_nat, lnorm)
        assert ms["n"] == len(seq) and ms["ln"] == float(len(seq))
        compare_with_yardstick(ms, want, margin, "front end s40")
        js = S.map_scores_json(ms)
        args = ["-i", str(path), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file, "--native", str(natives / "s40.pdb")]
        texts, errs = [], []
        for extra in ([], ["--score-map"]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(json.loads(err.getvalue().strip().split("\n")[-1]))
        assert texts[0] == texts[1] and "map" not in errs[0] and errs[1]["map"] == js
        assert {k: v for k, v in errs[1].items() if k != "map"} == errs[0] == S.scores_json(sc)
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i", str(path), "-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--natives", str(natives), "--score-map"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["scored_targets"] == 1 == summary["map_scored_targets"] and summary["scores"]["s40"]["map"] == js
            assert summary["mean_map_lddt"] == js["map_lddt"] == summary["median_map_lddt"]
            if fmt == "pdb":
                assert (out_dir / "s40.pdb").read_text() == texts[0] and not (out_dir / "s40.distmap.npy").exists()
                assert json.loads((out_dir / "s40.scores.json").read_text())["map"] == js
            else:
                z = np.load(str(out_dir / "s40.npz"))
                assert float(z["map_lddt"]) == ms["map_lddt"] and "distmap" not in z.files
                assert np.array_equal(z["map_lddt_res"], ms["map_lddt_res"], equal_nan=True)
                assert list(z["map_counts"][2][2:5]) == ms["classes"]["long"]["hits"]
    finally:
        P._ENGINES.clear()
