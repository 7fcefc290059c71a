"""The final refinement restrained to the predicted distance map on the GPU (options "restrain_milli" / "restrain_cut_mA",
include/dmpfold_hip.h).

The reference has no such term, so the yardstick is the definition itself: tests/restrain_ref.py restates the step in NumPy,
and the kernels' result after m steps is compared with the float64 restatement started from the very trace and map the GPU
held ("best_ca", "best_dm" of dmp_debug_fetch).  The bound is max(1e-5 A, 4 x max|restatement_f32 - restatement_f64|) from the
same inputs - the restatement's own rounding spread, times 4 because the kernels add a residue's partners in T slices, the
same kind of difference.  Everything else is an invariance: bits that must not move.

Targets are synth_msa(L, N, 1000 + L) with the seed-0 weights.  N = 1 except L = 65 (N = 8) and L = 129 (N = 4): with these
the CPU oracle's chosen map restrains at least 92 % of the pairs at every length used here (1.00 up to L = 33, 0.98 at 64 and
65, 0.925 at 129, 0.93 at 257), well above the half every swept case must reach.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import restrain_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

LENGTHS = [8, 31, 32, 33, 64, 65, 257]      # 31 | 32: one workgroup -> cluster; 33: five workgroups own nothing; 257: Lg 17, T 30
STEPS = [1, 3, 10]
DEPTH = {65: 8, 129: 4}                     # N of the target; 1 elsewhere
OPTS = ("restrain_milli", "restrain_cut_mA", "emit_distmap", "refine_single", "cluster_local", "recycle_tol_mA")


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float32)).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def eng(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 300, 3000)
    e.set_weights(_tensors(synth_sd))
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _options_as_they_were(request):
    """Every test leaves the engine's options as it found them."""
    if "eng" not in request.fixturenames:
        yield
        return
    e = request.getfixturevalue("eng")
    before = {k: e.get_option(k) for k in OPTS + ("precision",)}
    yield
    for k, v in before.items():
        e.set_option(k, v)


_ALN = {}


def _target(L):
    from dmpfold2_amd import synth
    if L not in _ALN:
        _ALN[L] = np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, DEPTH.get(L, 1), 1000 + L)))
    return _ALN[L]


def _predict(eng, L, m, iterations=1, **kw):
    """-> the call's tensors, cloned, after a fault check."""
    out = eng.predict(_target(L), None, iterations, m, **kw)
    eng.sync_check()
    return tuple(x.clone() for x in out)


def _fetch(eng, name, *shape):
    return eng.fetch(name, int(np.prod(shape))).cpu().numpy().reshape(shape)


# ------------------------------------------------------------------------------------------------ 1. the step
def _parity(eng, L, m, tag):
    coords, confs, dm, info = _predict(eng, L, m, distmap=True, restrain=1.0)
    assert [eng.get_option(k) for k in OPTS[:3]] == [0, 15000, 0]             # set for the call only
    start = _fetch(eng, "best_ca", L, 3)
    kept = _fetch(eng, "best_dm", L, L)
    assert np.array_equal(_bits(kept), _bits(dm)) and np.array_equal(kept, kept.T)
    far = np.triu(np.ones((L, L), dtype=bool), 2)
    share = float((kept[far] < np.float32(15.0)).mean())
    assert share >= 0.5, (tag, "restrained share of the pairs", share)
    r64 = R.refine(start, m, kept, 1.0, 15.0, np.float64)
    r32 = R.refine(start, m, kept, 1.0, 15.0, np.float32)
    bound = max(1e-5, 4.0 * float(np.abs(r32.astype(np.float64) - r64).max()))
    got = coords[:, 1].cpu().numpy()
    dev = float(np.abs(got.astype(np.float64) - r64).max())
    moved = float(np.abs(r64 - R.refine(start, m, None, 0.0, 15.0, np.float64)).max())
    print(f"restrain parity {tag} L={L} m={m}: deviation {dev:.3e} A  bound {bound:.3e} A  restrained share {share:.3f}  "
          f"restraints moved the trace by {moved:.3e} A", file=sys.stderr)
    assert moved > 10 * bound, (tag, "the restraints do nothing here", moved)
    assert dev <= bound, (tag, L, m, dev, bound)
    return coords


@pytest.mark.parametrize("L", LENGTHS)
def test_step_parity(eng, L):
    for m in STEPS:
        _parity(eng, L, m, "default form")


@pytest.mark.parametrize("L", LENGTHS)
def test_step_parity_single_workgroup(eng, L):
    """ "refine_single" = 1: refine_kernel at every length (the default form uses it below L = 32 only)."""
    eng.set_option("refine_single", 1)
    for m in STEPS:
        _parity(eng, L, m, "refine_single")


@pytest.mark.parametrize("L", [65, 257])
def test_same_bits_whichever_way_the_cluster_publishes_and_on_every_run(eng, L):
    runs = []
    for local in (0, 1, 1):
        eng.set_option("cluster_local", local)
        runs.append(_predict(eng, L, 10, restrain=1.0))
    for r in runs[1:]:
        assert np.array_equal(_bits(r[0]), _bits(runs[0][0])) and np.array_equal(_bits(r[1]), _bits(runs[0][1]))


# ------------------------------------------------------------------------------------------------ 2. bit identity
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("L", [31, 65])
def test_no_cutoff_is_the_plain_refinement(eng, L, precision):
    """ "restrain_cut_mA" = 0 with the force on: the RESTRAIN instantiation runs, no pair qualifies, the plain bits come out."""
    eng.set_option("precision", precision)
    plain = _predict(eng, L, 100)
    none = _predict(eng, L, 100, restrain=1.0, restrain_cutoff=0.0)
    assert np.array_equal(_bits(none[0]), _bits(plain[0])) and np.array_equal(_bits(none[1]), _bits(plain[1]))
    assert _fetch(eng, "best_dm", L, L).shape == (L, L)                         # the map was kept for it
    some = _predict(eng, L, 100, restrain=1.0)
    assert not np.array_equal(_bits(some[0]), _bits(plain[0])) and np.array_equal(_bits(some[1]), _bits(plain[1]))


def test_off_after_on_restores_the_plain_bits(eng):
    L = 65
    plain = _predict(eng, L, 10)
    assert eng.fetch("best_dm", L * L).numel() == 0 and eng.restrain is None
    eng.set_option("restrain_milli", 1000)
    on = _predict(eng, L, 10)
    assert len(on) == 2 and not np.array_equal(_bits(on[0]), _bits(plain[0]))
    assert eng.fetch("best_dm", L * L).numel() == L * L                         # kept without "emit_distmap"
    assert eng.restrain["restrained_pairs"] is None and eng.restrain["clashes"] >= 0
    eng.set_option("restrain_milli", 0)
    off = _predict(eng, L, 10)
    assert np.array_equal(_bits(off[0]), _bits(plain[0])) and np.array_equal(_bits(off[1]), _bits(plain[1]))
    assert eng.fetch("best_dm", L * L).numel() == 0 and eng.restrain is None


@pytest.mark.parametrize("L", [31, 65])
def test_no_steps_nothing_runs(eng, L):
    plain = _predict(eng, L, 0)
    on = _predict(eng, L, 0, restrain=1.0)
    assert np.array_equal(_bits(on[0]), _bits(plain[0])) and np.array_equal(_bits(on[1]), _bits(plain[1]))


# ------------------------------------------------------------------------------------------------ 3. what must not move
def test_only_the_final_trace_moves(eng):
    """L = 65, three recycling passes, m = 10, the convergence measure recorded (a tolerance no pass meets): the confidences,
    the pass chosen, its map, every pass's trace, every delta and the pass count have the bits of the run without restraints."""
    L, it, m = 65, 3, 10
    runs = []
    for k in (None, 1.0):
        coords, confs, dm, info = _predict(eng, L, m, it, distmap=True, converge=0.001, restrain=k)
        runs.append(dict(coords=coords, confs=confs, dm=dm, best_pass=info[0].item(), passes_run=eng.passes_run,
                         info_passes=info[1].item(), ca_pass=_fetch(eng, "ca_pass", it + 1, L, 3),
                         pass_delta=eng.fetch("pass_delta", it + 1).cpu().numpy(), start=_fetch(eng, "best_ca", L, 3)))
    off, on = runs
    assert off["passes_run"] == on["passes_run"] == it + 1 == int(on["info_passes"]) and off["best_pass"] == on["best_pass"]
    for name in ("confs", "dm", "ca_pass", "pass_delta", "start"):
        assert np.array_equal(_bits(on[name]), _bits(off[name])), name
    assert len(on["pass_delta"]) == it + 1
    assert not np.array_equal(_bits(on["coords"]), _bits(off["coords"]))


# ------------------------------------------------------------------------------------------------ 4. the effect
@pytest.mark.parametrize("L", [65, 129])
def test_map_rms_falls(eng, L):
    """m = 100, k = 1: map_rms restrained < 0.8 x map_rms plain (the restatement alone gives 0.57 at L = 65 and 0.62 at 129;
    the two arithmetics' 100-step trajectories differ by up to 1e-2 A, which moves an RMS of 7 - 12 A by far less), and both
    are the float64 map_rms of the returned map and trace."""
    values = []
    for k in (None, 1.0):
        coords, confs, dm, info = _predict(eng, L, 100, distmap=True, restrain=k)
        want = R.map_rms(dm.cpu().numpy(), coords[:, 1].cpu().numpy())
        assert abs(info[2].item() - want) <= 1e-6 * want, (L, k, info[2].item(), want)
        values.append(info[2].item())
        if k:
            rep = eng.restrain
            far = np.triu(np.ones((L, L), dtype=bool), 2)
            assert rep["map_rms"] == info[2].item() and (rep["k"], rep["cutoff"], rep["steps"]) == (1.0, 15.0, 100)
            assert rep["restrained_pairs"] == int((dm.cpu().numpy()[far] < np.float32(15.0)).sum())
            print(f"restrain effect L={L}: map_rms plain {values[0]:.4f} restrained {values[1]:.4f} ratio {values[1] / values[0]:.3f}  "
                  f"report {rep}", file=sys.stderr)
        else:
            assert eng.restrain is None
    assert values[1] < 0.8 * values[0], (L, values)


# ------------------------------------------------------------------------------------------------ 5. every other extra
def test_beside_every_other_extra(eng):
    """The score, SS, align and search blocks are functions of the returned - restrained - coordinates: each against its CPU
    restatement.  The map-score block (a function of the map and the native) and the pass block (of the recorded passes)
    keep the bits of the run without restraints."""
    from test_align_cpu import compare_alignment, indel_copy, moved, random_walk
    from test_align_cpu import yardstick as align_yardstick
    from test_score_cpu import compare_with_yardstick
    from test_score_cpu import yardstick as score_yardstick
    from test_gpu_ss import _model_leg
    L, m = 65, 10
    aln = _target(L)
    plain, _ = _predict(eng, L, m)
    model = plain[:, 1].cpu().numpy()
    lib = S.Library.from_traces([indel_copy(model, 51, m=61)[0], random_walk(30, 5), moved(model, 3)[2]])
    native = moved(model, 4)[2]
    structure = indel_copy(model, 52, m=70)[0]
    kw = dict(distmap=True, native=native, structure=structure, library=lib, score_map=True, score_passes=True, ss=True)
    names = ("score_block", "map_score_block", "pass_block", "align_block", "search_block", "ss_block")
    off = _predict(eng, L, m, **kw)
    blocks_off = {n: getattr(eng, n).clone() for n in names}
    assert np.array_equal(_bits(off[0]), _bits(plain))
    on = _predict(eng, L, m, restrain=1.0, **kw)
    blocks_on = {n: getattr(eng, n).clone() for n in names}
    scores, alignment, hits = eng.scores, eng.alignment, eng.hits
    coords = on[0]
    alone = _predict(eng, L, m, restrain=1.0)
    assert np.array_equal(_bits(coords), _bits(alone[0])) and not np.array_equal(_bits(coords), _bits(plain))
    assert np.array_equal(_bits(on[1]), _bits(off[1])) and np.array_equal(_bits(on[2]), _bits(off[2]))      # confidences, map
    for n in ("map_score_block", "pass_block"):
        assert np.array_equal(_bits(blocks_on[n]), _bits(blocks_off[n])), n
    for n in ("score_block", "align_block", "search_block", "ss_block"):
        assert not np.array_equal(_bits(blocks_on[n]), _bits(blocks_off[n])), n
    trace = coords[:, 1].cpu().numpy()
    want, margin = score_yardstick(trace, native, 0.0)
    compare_with_yardstick(scores, want, margin, "restrained, every extra: score block")
    want, margin = align_yardstick(trace, structure)
    compare_alignment(alignment, want, margin, "restrained, every extra: align block")
    for k in range(len(lib)):
        want, margin = align_yardstick(trace, lib.entry(k))
        compare_alignment(hits["hits"][k], want, margin, f"restrained, every extra: search entry {k}")
    _model_leg(blocks_on["ss_block"], coords, aln[0], "restrained, every extra")


# ------------------------------------------------------------------------------------------------ 6. pipeline
def test_pipeline(synth_sd):
    from dmpfold2_amd.predict import Engine, Pipeline
    from dmpfold2_amd import synth
    lengths = [40, 24, 64]
    alns = [np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L))) for L in lengths]
    dev, sdt = torch.device("cuda:0"), _tensors(synth_sd)
    single = Engine(dev, 64, 1)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 64, 1, sdt, streams=2, precision=2, restrain=1.0)
    try:
        assert all([e.get_option(k) for k in OPTS[:3]] == [1000, 15000, 1] for e in pipe.engines)
        refs, plains = [], []
        for aln in alns:
            out = single.predict(aln, None, 1, 10, distmap=True, restrain=1.0)
            single.sync_check()
            refs.append(tuple(x.clone() for x in out))
            out = single.predict(aln, None, 1, 10)
            single.sync_check()
            plains.append(tuple(x.clone() for x in out))
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), 1, 10) for a in alns]
        res = pipe.collect(tickets)
        for t, ref, plain, L in zip(tickets, refs, plains, lengths):
            assert not isinstance(res[t], Exception), res[t]
            assert len(res[t]) == 4
            for got, want in zip(res[t], ref):
                assert np.array_equal(_bits(got), _bits(want)), L
            assert not np.array_equal(_bits(res[t][0]), _bits(plain[0])), L
        with pytest.raises(ValueError):
            pipe.set_restrain(-1.0)
        with pytest.raises(ValueError):
            pipe.set_restrain(1.0, cutoff=1000.0)
        assert all([e.get_option(k) for k in OPTS[:3]] == [1000, 15000, 1] for e in pipe.engines)
        pipe.set_restrain(0.5, cutoff=8.0)
        assert all([e.get_option(k) for k in OPTS[:2]] == [500, 8000] for e in pipe.engines)
        pipe.set_restrain(None)
        pipe.set_distmap(False)
        out = pipe.run([torch.from_numpy(alns[0]).to(dev)], 1, 10)
        pipe.sync_check()
        assert len(out[0]) == 2 and np.array_equal(_bits(out[0][0]), _bits(plains[0][0]))
    finally:
        pipe.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 7. the options
@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_options", os.path.join(ROOT, "tools", "record_options.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,default", [("restrain_milli", 0), ("restrain_cut_mA", 15000)])
def test_option_answers(recorder, name, default):
    """The scheme of tools/record_options.py over its PROBES: a fresh context reads the default, 0 .. 100000 is accepted and
    read back, the rest is refused with the one message and leaves the value as it was."""
    from dmpfold2_amd import _lib
    lib = _lib.load()
    rec = recorder.probe(lib, name)
    assert rec["fresh"] == [0, default, ""]
    held = default
    for value, rc, err, after in rec["set"]:
        if 0 <= value <= 100000:
            assert (rc, err) == (0, ""), (name, value, rc, err)
            held = value
        else:
            assert rc < 0 and err == f"{name} must be 0 .. 100000, got {value}", (name, value, rc, err)
        assert after == [0, held, ""], (name, value, after)
    assert [r[0] for r in rec["set"]] == list(recorder.PROBES) and any(r[1] < 0 for r in rec["set"])
    # the upper end, which PROBES does not reach, and "device_mib", which the options must not move
    ctx = C.c_void_p()
    assert lib.dmp_ctx_create(0, recorder.MAX_L, recorder.MAX_N, C.byref(ctx)) == 0
    try:
        def get(which):
            v = C.c_int(recorder.UNTOUCHED)
            assert lib.dmp_ctx_get_option(ctx, which.encode(), C.byref(v)) == 0
            return v.value
        mib = get("device_mib")
        assert lib.dmp_ctx_set_option(ctx, name.encode(), 100000) == 0 and get(name) == 100000
        assert lib.dmp_ctx_set_option(ctx, name.encode(), 100001) < 0
        assert lib.dmp_last_error().decode() == f"{name} must be 0 .. 100000, got 100001" and get(name) == 100000
        for other in ("restrain_milli", "restrain_cut_mA"):
            assert lib.dmp_ctx_set_option(ctx, other.encode(), 1000) == 0
        assert get("device_mib") == mib
    finally:
        lib.dmp_ctx_destroy(ctx)


# ------------------------------------------------------------------------------------------------ 8. front ends
def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold -r K [--restrain-cutoff A]` and `dmpfold-batch --restrain K`: without the flag stdout is what it was; with it
    REMARK CONF stays, the body is the restrained model's, and the report - one JSON line on stderr, the batch's files and
    summary - is the dict of aln_to_coords(..., return_restrain=True)."""
    import contextlib
    import io
    import json
    from conftest import golden_rows, load_golden
    import dmpfold2_amd.predict as P
    from dmpfold2_amd import aln_to_coords, run_dmpfold
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        p = tmp_path / "pf.aln"
        p.write_text("\n".join(golden_rows(load_golden("pf10963_n3_m0"))) + "\n")
        kw = dict(device="cuda:0", iterations=1, minsteps=10, weights_file=weights_file)
        plain = aln_to_coords(str(p), **kw)
        L = plain[0].shape[0]
        with pytest.raises(ValueError):
            aln_to_coords(str(p), restrain=-1.0, **kw)
        c, f, dm, rep = aln_to_coords(str(p), return_distmap=True, restrain=1.0, restrain_cutoff=12.0, return_restrain=True, **kw)
        assert [P._ENGINES[0].get_option(k) for k in OPTS[:3]] == [0, 15000, 0]
        assert torch.equal(f, plain[1]) and not torch.equal(c, plain[0])
        far = np.triu(np.ones((L, L), dtype=bool), 2)
        assert (rep["k"], rep["cutoff"], rep["steps"]) == (1.0, 12.0, 10)
        assert rep["restrained_pairs"] == int((dm.cpu().numpy()[far] < np.float32(12.0)).sum()) > 0
        want = R.map_rms(dm.cpu().numpy(), c[:, 1].cpu().numpy())
        assert abs(rep["map_rms"] - want) <= 1e-6 * want
        d = R.distances(c[:, 1].cpu().numpy())
        assert rep["clashes"] == int((d[far] < 3.0).sum())
        assert abs(rep["bond_dev_max"] - np.abs(np.diagonal(d, 1) - 3.78).max()) < 1e-12
        assert aln_to_coords(str(p), return_restrain=True, **kw)[-1] is None
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "10", "-w", weights_file]
        texts, errs = [], []
        for extra in ([], ["-r", "1", "--restrain-cutoff", "12"], ["--restrain", "0"]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0] == P.pdb_text(plain[0], plain[1], P.encode_aln(P.read_aln(str(p)))) == texts[2]
        assert "restrain" not in errs[0] and "restrain" not in errs[2]
        remark = texts[0].split("\n")[0]
        assert remark.startswith("REMARK  CONF") and texts[1].split("\n")[0] == remark and texts[1] != texts[0]
        assert texts[1] == P.pdb_text(c, f, P.encode_aln(P.read_aln(str(p))))
        assert json.loads(errs[1].strip().split("\n")[-1]) == {"restrain": rep}
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "10", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--restrain", "1", "--restrain-cutoff", "12"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 1 and summary["restrained_targets"] == 1 and summary["restrain"] == {"pf": rep}
            assert summary["mean_map_rms"] == summary["median_map_rms"] == rep["map_rms"] and summary["mean_clashes"] == rep["clashes"]
            if fmt == "pdb":
                assert sorted(os.listdir(out_dir)) == ["pf.pdb", "pf.restrain.json"]
                assert (out_dir / "pf.pdb").read_text() == texts[1]
                assert json.loads((out_dir / "pf.restrain.json").read_text()) == {"restrain": rep}
            else:
                z = np.load(str(out_dir / "pf.npz"))
                assert np.array_equal(z["coords"], c.cpu().numpy()) and "distmap" not in z.files
                assert int(z["restrain_restrained_pairs"]) == rep["restrained_pairs"] and int(z["restrain_clashes"]) == rep["clashes"]
                assert float(z["restrain_map_rms"]) == np.float32(rep["map_rms"]) and int(z["restrain_steps"]) == 10
        out_dir = tmp_path / "out_plain"
        with contextlib.redirect_stdout(io.StringIO()):
            assert batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "10", "-w", weights_file, "--streams", "2"]) == 0
        assert sorted(os.listdir(out_dir)) == ["pf.pdb"] and (out_dir / "pf.pdb").read_text() == texts[0]
    finally:
        P._ENGINES.clear()
