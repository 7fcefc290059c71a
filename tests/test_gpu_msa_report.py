"""Alignment depth, conservation and DCA contacts on the GPU (option "msa_report"; include/dmpfold_hip.h).

The library's report block is compared with tests/msa_report_ref.py, the NumPy restatement of the header's definition, which
takes the DCA contact map as an input (the map the block hands out with value 2): every integer and every copied float exactly,
the Neff sums, neff_col, the entropy and the frequencies within the bounds that module derives from the number formats.  Every
test prints its largest error / bound per check.  The library takes no alignment shorter than 8 columns, so the sweep's
shortest is 8; tests/test_msa_report_cpu.py holds the restatement at L = 5 and 6.  On the parent commit the option and the
names do not exist and every test here fails."""
import sys

import numpy as np
import pytest
import torch

import domains_ref as D
import msa_report_ref as R
from test_align_cpu import random_walk

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

# N: one row, the pair tile's edge of 64 and a third tile row; L: the word tail, the 64-column K chunk and its successor
SHAPES = [(2, 8), (2, 16), (63, 63), (64, 64), (65, 65), (63, 67), (65, 16), (64, 129), (130, 67), (130, 129)]
WORST = {}                           # check -> (ratio, where): the largest over every comparison of this module


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float32)).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def eng(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 136, 130)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


def alignment(N, L, seed=0):
    """Mutated copies of a seed row with gaps: a gap in the query (column 4), an all-gap column (2), a copy of the query
    (row 1), rows with exactly floor(L t) and floor(L t) + 1 matches with the query at t = 0.62, 0.8, 0.9 (rows 2 .. 7), an
    unknown residue (code 21, which clamps to the gap)."""
    rng = np.random.default_rng(1000 * N + L + seed)
    query = rng.integers(0, 20, L).astype(np.uint8)
    query[4] = 20
    query[2] = 20
    a = np.tile(query, (N, 1))
    free = np.setdiff1d(np.arange(L), [2, 4])            # (the two gap columns always match: they are never changed)
    for n in range(2, N):
        if 2 <= n < 8 and N >= 8:
            t = R.THRESHOLDS[(n - 2) // 2]
            keep = min(L, int(np.floor(L * t)) + (n - 2) % 2)
        else:
            keep = int(rng.integers(L // 3, L + 1))
        change = rng.permutation(free)[:L - keep]
        a[n, change] = np.where(query[change] < 20, (query[change] + 1 + rng.integers(0, 18, change.size)) % 20, rng.integers(0, 20, change.size))
        if n >= 8:
            gaps = rng.random(L) < 0.15
            a[n, gaps] = 20
    if N > 8:
        a[N - 1, 1] = 21
    assert (a[:, 2] == 20).all()
    return np.ascontiguousarray(a)


def _held(ref, block, L, tag):
    res = R.check(ref, block, L)
    print(tag, {k: (round(r, 4), note) for k, (r, note) in res.items()}, file=sys.stderr)
    for k, (r, note) in res.items():
        if r >= WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (r, f"{tag}: {note}")
    assert not R.failed(res), (tag, {k: res[k] for k in R.failed(res)})
    return res


def _run(eng, aln, native=None, value=2, **kw):
    """One prediction with the option on -> (block as a float32 array, coords, confs)."""
    coords, confs = eng.predict_msa_report(aln, None, 0, 0, dca_map=value == 2, native=native, **kw)
    eng.sync_check()
    assert eng.get_option("msa_report") == 0
    L = aln.shape[1]
    assert tuple(eng.msa_report_block.shape) == (S.msa_report_floats(L, value == 2),)
    return eng.msa_report_block.cpu().numpy().copy(), coords, confs


# ------------------------------------------------------------------------------------------------ 1. shape sweep
@pytest.mark.parametrize("N,L", SHAPES)
def test_shape_sweep(eng, N, L):
    aln = alignment(N, L)
    blk, coords, confs = _run(eng, aln)
    hdr, cols, dmap = R.split(blk, L)
    assert dmap is not None and hdr[126] == 1.0 and hdr[127] == 0.0 and not hdr[8:16].any() and not hdr[76:126].any()
    contacts = eng.fetch("contacts", L * L).cpu().numpy().reshape(L, L)
    assert np.array_equal(_bits(dmap), _bits(contacts))                  # the map the stem was given, bit for bit
    ref = R.report(aln, dmap)
    _held(ref, blk, L, f"sweep N={N} L={L}")
    # neff_80's neighbour counts are the weights' own: 1 / w rounds to the count
    w = eng.fetch("w", N).cpu().numpy().astype(np.float64)
    assert np.array_equal(np.rint(1.0 / w).astype(np.int64), ref["nbr"][1]) and np.array_equal(_bits(w.astype(np.float32)), _bits(ref["weights"]))
    if N >= 8:
        # the edge rows: exactly floor(L t) matches with the query is no neighbour of it at t, floor(L t) + 1 is
        cnt = R.pair_counts(R.clamp(aln))
        for k, t in enumerate(R.THRESHOLDS):
            m = int(np.floor(L * t))
            on, above = 2 + 2 * k, 3 + 2 * k
            assert cnt[0, on] == m and cnt[0, above] == min(L, m + 1), (t, cnt[0, on], cnt[0, above])
            near = cnt[0].astype(np.float32) > np.float32(float(L) * t)
            assert not near[on] and near[above]
        print(f"N={N} L={L}: neff {hdr[2:5].tolist()} copies {hdr[6]} gap cells {hdr[5]}", file=sys.stderr)
        assert hdr[6] >= 2 and hdr[7] == 2
    # value 1: the same block without the map
    short, _, _ = _run(eng, aln, value=1)
    assert np.array_equal(_bits(short), _bits(blk[:128 + 8 * L]))
    rep = eng.msa_report
    assert rep["N"] == N and rep["L"] == L and "dca_map" not in rep and "r_conf" in rep and rep["neff_80"] == float(hdr[3])
    assert np.array_equal(rep["hist_cov"], hdr[36:56].astype(np.int64)) and rep["hist_idq"].sum() == N


# ------------------------------------------------------------------------------------------------ 2. with a native
@pytest.mark.parametrize("N,L", [(64, 40), (130, 64)])
@pytest.mark.parametrize("holes", [False, True])
def test_with_a_native(eng, N, L, holes):
    aln = alignment(N, L, 7)
    native = D.globule(L, 0).astype(np.float32)
    if holes:
        native[[3, 17, L - 2]] = np.nan
    blk, _, _ = _run(eng, aln, native, score_map=True)
    hdr, cols, dmap = R.split(blk, L)
    ref = R.report(aln, dmap, native)
    _held(ref, blk, L, f"native N={N} L={L} holes={holes}")
    n = L - (3 if holes else 0)
    assert hdr[124] == n and hdr[125] == n and hdr[126] == 1.0 and hdr[127] == 1.0
    ms = eng.map_score_block.cpu().numpy()
    assert ms[0] == hdr[124] and ms[1] == hdr[125]
    for c in range(4):
        assert np.array_equal(ms[2 + 12 * c:4 + 12 * c], hdr[76 + 12 * c:78 + 12 * c]), c      # one candidate definition
        assert not hdr[84 + 12 * c:88 + 12 * c].any()
    rep = eng.msa_report
    assert rep["has_native"] and rep["classes"]["long"]["t"][0] == int(hdr[76 + 24 + 5]) and rep["n"] == n
    print("classes", {k: (v["candidates"], v["native_contacts"], v["h"], v["t"]) for k, v in rep["classes"].items()}, file=sys.stderr)
    assert hdr[76] > 0 and hdr[77] > 0 and hdr[100] > 0


# ------------------------------------------------------------------------------------------------ 3. one row
def test_one_row(eng):
    L = 16
    aln = alignment(1, L)
    blk, _, _ = _run(eng, aln, D.globule(L, 0).astype(np.float32))
    hdr, cols, dmap = R.split(blk, L)
    ref = R.report(aln, None, D.globule(L, 0))
    _held(ref, blk, L, "one row")
    assert hdr[126] == 0.0 and hdr[127] == 1.0 and hdr[2:5].tolist() == [1.0, 1.0, 1.0] and not hdr[76:126].any()
    assert np.isnan(cols[6]).all() and np.isnan(cols[7]).all() and not dmap.any()
    assert hdr[16:36].sum() == 1 and hdr[16 + 19] == 1 and hdr[36:56].sum() == 1 and not hdr[56:76].any()


# ------------------------------------------------------------------------------------------------ 4. nothing else moves
def test_alone_and_beside_every_other_block_engine_and_pipeline(synth_sd):
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, Pipeline
    L, N, ITERATIONS, MINSTEPS = 24, 4, 1, 5
    OTHERS = ("score_block", "align_block", "search_block", "map_score_block", "pass_block", "ss_block", "exposure_block")
    MORE = ("domains_block", "domain_score_block", "flex_block")
    FORCED = dict(tau=1.0, min_size=8, min_segment=2)
    aln = np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, N, 1024)))
    native = random_walk(L, 1).astype(np.float32)
    structure = random_walk(12, 2).astype(np.float32)
    library = S.Library.from_traces([random_walk(8, 3), random_walk(12, 4)])
    everything = dict(distmap=True, native=native, structure=structure, library=library, score_map=True, score_passes=True, ss=True,
                      exposure=True)
    dev, sdt = torch.device("cuda:0"), _tensors(synth_sd)
    eng = Engine(dev, L, N)
    eng.set_weights(sdt)
    eng.set_option("precision", 2)
    eng.set_option("tridiag_cluster", 0)                  # (the form a pipeline of several engines takes: see test_gpu_flex.py)
    pipe = Pipeline(dev, L, N, sdt, streams=2, precision=2, distmap=True, score=True, align=True, search=library, score_map=True,
                    score_passes=True, ss=True, exposure=True)
    try:
        with eng.with_domains(**FORCED), eng.with_score_domains(), eng.with_flex():
            without = [x.clone() for x in eng.predict(aln, None, ITERATIONS, MINSTEPS, **everything)]
            eng.sync_check()
            blocks = {name: getattr(eng, name).clone() for name in OTHERS + MORE}
            assert eng.msa_report_block is None and eng.msa_report is None
        for value in (1, 2):
            # alone
            coords, confs = eng.predict_msa_report(aln, None, ITERATIONS, MINSTEPS, dca_map=value == 2)
            eng.sync_check()
            alone = eng.msa_report_block.clone()
            assert np.array_equal(_bits(coords), _bits(without[0])) and np.array_equal(_bits(confs), _bits(without[1]))
            assert all(getattr(eng, name) is None for name in OTHERS + MORE)
            assert alone[127].item() == 0.0 and alone.shape[0] == S.msa_report_floats(L, value == 2)
            # beside all ten
            with eng.with_domains(**FORCED), eng.with_score_domains(), eng.with_flex():
                full = [x.clone() for x in eng.predict_msa_report(aln, None, ITERATIONS, MINSTEPS, dca_map=value == 2, **everything)]
                eng.sync_check()
                beside = eng.msa_report_block.clone()
                for name in OTHERS + MORE:
                    assert np.array_equal(_bits(getattr(eng, name)), _bits(blocks[name])), (value, name)
            assert len(full) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(full, without))
            assert beside[127].item() == 1.0
            keep = np.r_[0:76, 126:127, 128:beside.shape[0]]
            assert np.array_equal(_bits(beside)[keep], _bits(alone)[keep])
            ref = R.report(aln, eng.fetch("contacts", L * L).cpu().numpy().reshape(L, L), native)
            _held(ref, beside.cpu().numpy(), L, f"beside, value {value}")
        # the pipeline without the option: what it has always handed out
        ticket = pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure)
        res = pipe.collect([ticket])[ticket]
        assert not isinstance(res, Exception), res
        assert len(res) == 4 + len(OTHERS)
        # ... and with it: the same tuple, the same bits, the report block on the target's Outputs
        pipe.use_msa_report(True, dca_map=True)
        tickets = [pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure) for _ in range(2)]
        got = pipe.collect(tickets)
        for t in tickets:
            assert not isinstance(got[t], Exception), got[t]
            assert len(got[t]) == 4 + len(OTHERS)
            for name, a, b in zip(("coords", "confs", "distmap", "info") + OTHERS, got[t], without + [blocks[n] for n in OTHERS]):
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), name
            assert np.array_equal(_bits(pipe.collected[t].msa_report_block), _bits(beside))
        pipe.engines[1].set_option("msa_report", 1)
        with pytest.raises(RuntimeError, match="msa_report"):
            pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS)
        pipe.use_msa_report(False)
    finally:
        pipe.close()
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. repeats
def test_two_runs_give_the_same_bits_and_a_small_target_after_a_large_one(eng):
    big, small = alignment(130, 129, 3), alignment(5, 24, 3)
    native = D.globule(129, 0).astype(np.float32)
    first, _, _ = _run(eng, big, native)
    second, _, _ = _run(eng, big, native)
    assert np.array_equal(_bits(first), _bits(second))
    blk, _, _ = _run(eng, small)
    _held(R.report(small, R.split(blk, 24)[2]), blk, 24, "small after large")
    alone, _, _ = _run(eng, small)
    assert np.array_equal(_bits(alone), _bits(blk))


# ------------------------------------------------------------------------------------------------ 6. option errors
def test_option_errors(eng):
    for bad in (3, -1):
        with pytest.raises(Exception, match="msa_report must be 0, 1 or 2"):
            eng.set_option("msa_report", bad)
        assert eng.get_option("msa_report") == 0
    assert eng.lib.dmp_ctx_set_option(eng._ctx, b"msa_report", 3) == -1       # DMP_ERR_ARG
    eng.set_msa_report(True, dca_map=True)
    assert eng.get_option("msa_report") == 2
    eng.set_msa_report(True)
    assert eng.get_option("msa_report") == 1
    aln = alignment(5, 24)
    eng.predict(aln, None, 0, 0)                          # value 1 without "score_native" works, has_native 0
    eng.sync_check()
    assert eng.msa_report_block[127].item() == 0.0 and eng.msa_report_block[126].item() == 1.0 and not eng.msa_report["has_native"]
    eng.set_msa_report(False)
    assert eng.get_option("msa_report") == 0


# ------------------------------------------------------------------------------------------------ 7. front ends
def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --msa-report [...]` and `dmpfold-batch --msa-report [...]`: stdout byte for byte the run's without the option, the
    JSON line the dict of aln_to_msa_report, the batch's files and summary carry the same figures."""
    import contextlib
    import io
    import json
    import dmpfold2_amd.predict as P
    from dmpfold2_amd import aln_to_coords, run_dmpfold, synth
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        p = tmp_path / "t48.aln"
        synth.write_aln(str(p), synth.synth_msa(48, 6, 48))
        kw = dict(device="cuda:0", iterations=1, minsteps=0, weights_file=weights_file)
        plain = aln_to_coords(str(p), **kw)
        c, f, alnmat, rep = P.aln_to_msa_report(str(p), return_alnmat=True, **kw, dca_map=True)
        assert c.shape[0] == 48 and torch.equal(c, plain[0]) and torch.equal(f, plain[1])
        assert P._ENGINES[0].get_option("msa_report") == 0
        assert rep["N"] == 6 and rep["L"] == 48 and rep["dca_map"].shape == (48, 48) and "rho_conf" in rep and len(rep["cons_seq"]) == 48
        ref = R.report(np.asarray(alnmat), rep["dca_map"])
        assert abs(rep["neff_80"] - ref["header"][3]) <= ref["bound_header"][3] and np.array_equal(rep["gaps"], ref["columns"][0].astype(np.int64))
        want = json.loads(json.dumps({"msa": S.msa_report_json(rep)}))
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file]
        texts, errs = [], []
        for extra in ([], ["--msa-report"], ["--msa-report", "--msa-report-file", str(tmp_path / "msa.json"), "--dca-map", str(tmp_path / "dca.npy")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        assert json.loads(errs[1].strip().split("\n")[-1]) == want and "\"msa\"" not in errs[0] and "\"msa\"" not in errs[2]
        assert json.loads((tmp_path / "msa.json").read_text()) == want
        assert np.array_equal(_bits(np.load(str(tmp_path / "dca.npy"))), _bits(rep["dca_map"]))
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "1", "--msa-report", "--dca-map"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 1 and summary["msa_targets"] == 1 and batch._MSA_REPORT is None
            brief = summary["msa"]["t48"]
            assert brief["N"] == 6 and brief["neff_80"] == want["msa"]["neff_80"] == summary["mean_msa_neff_80"] == summary["median_msa_neff_80"]
            assert brief["median_coverage"] == want["msa"]["median_coverage"]
            if fmt == "pdb":
                assert (out_dir / "t48.pdb").read_text() == texts[0]
                assert json.loads((out_dir / "t48.msa.json").read_text()) == want
                assert np.array_equal(_bits(np.load(str(out_dir / "t48.dca_map.npy"))), _bits(rep["dca_map"]))
            else:
                z = np.load(str(out_dir / "t48.npz"))
                assert np.array_equal(z["coords"], c.cpu().numpy())
                assert z["msa_header"].shape == (128,) and z["msa_columns"].shape == (8, 48)
                assert z["msa_header"][3] == np.float32(rep["neff_80"]) and np.array_equal(_bits(z["dca_map"]), _bits(rep["dca_map"]))
        # with --natives: the summary joins the depth with the accuracy
        from test_gpu_score import _random_walk, _write_pdb
        natives = tmp_path / "natives"
        natives.mkdir()
        query = synth.synth_msa(48, 6, 48)[0]
        _write_pdb(str(natives / "t48.pdb"), query, _random_walk(48, 7))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rc = batch.main(["-i", str(p), "-o", str(tmp_path / "out_nat"), "-n", "1", "-m", "0", "-w", weights_file, "--format", "pdb",
                             "--streams", "1", "--msa-report", "--natives", str(natives)])
        assert rc == 0, buf.getvalue()
        summary = json.loads(buf.getvalue().strip().split("\n")[-1])
        assert summary["scored_targets"] == 1 and summary["msa_targets"] == 1 and summary["neff_tm_targets"] == 1
        assert summary["neff_tm_spearman"] is None and sum(b["targets"] for b in summary["neff_tm_bins"].values()) == 1
        name = "<10" if summary["msa"]["t48"]["neff_80"] < 10 else "10-100"
        assert summary["neff_tm_bins"][name] == {"targets": 1, "mean_tm": summary["scores"]["t48"]["tm"]}
        js = json.loads((tmp_path / "out_nat" / "t48.msa.json").read_text())["msa"]
        assert js["has_native"] and js["n"] == 48 and set(js["classes"]) == set(S.MSA_CLASSES)
        assert not (tmp_path / "out_nat" / "t48.dca_map.npy").exists()
    finally:
        P._ENGINES.clear()


def test_worst_ratios():
    """The largest error / bound per float check over every comparison above (pytest -s prints it; the README records it)."""
    print("msa_report: largest error / bound per check:", {k: (round(r, 4), where) for k, (r, where) in sorted(WORST.items())}, file=sys.stderr)
    assert WORST and all(r <= 1.0 for r, _ in WORST.values())
