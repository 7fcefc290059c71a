"""Solvent exposure of the predicted backbone on the GPU (option "exposure"; include/dmpfold_hip.h).

The library's exposure block is compared with tests/exposure_ref.py, the NumPy restatement of the header's definition,
evaluated on the float32 coordinates the same call returned and with the sphere points the device holds (dmp_debug_fetch
"exposure_points").  Every output is an integer count: every comparison is exact, bit for bit; there is no tolerance anywhere.
On the parent commit the option is unknown and every test here fails."""
import sys

import numpy as np
import pytest
import torch

import exposure_ref as X
from test_ss_cpu import backbone, flat_hairpin, ideal_helix, native_3fgx

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

LENGTHS = [8, 63, 64, 65, 255, 256, 257]
MODEL = 7                            # header floats 1 .. 7 and arrays 0 .. 7 are the model's leg


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float32)).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def eng(synth_sd):
    """One engine (seed-0 weights, precision 2) for the single-engine tests."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 300, 64)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def points(eng):
    """The 768 floats the device holds; they are the committed table's bits."""
    p = eng.fetch("exposure_points", 768).cpu().numpy().reshape(256, 3)
    assert p.shape == (256, 3) and np.array_equal(_bits(p), _bits(S.exposure_points()))
    with pytest.raises(Exception):
        eng.fetch("exposure_points", 767)
    return p


def _one_row(L):
    from dmpfold2_amd import synth
    return np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L)))


_TRACES = {}


def _trace(eng, L):
    """The plain prediction of the one-row alignment of length L, made once: (aln, coords, confs)."""
    if L not in _TRACES:
        aln = _one_row(L)
        coords, confs = eng.predict(aln, None, 0, 0)
        eng.sync_check()
        _TRACES[L] = (aln, coords.clone(), confs.clone())
    return _TRACES[L]


def _model_leg(block, coords, first_row, points, tag):
    """The model's leg of an exposure block against the restatement on the returned coordinates, bit for bit."""
    L = coords.shape[0]
    want = X.exposure(coords.cpu().numpy(), first_row, points)
    b = block.cpu().numpy()
    got = b[32:32 + 8 * L].reshape(8, L)
    diff = int((got != X.arrays_of(want)).sum())
    print(tag, "area %.1f" % X.area(want["n"]), "sums", want["sums"], "buried", want["buried_atoms"], "hse", float(want["hse_up"].mean()),
          float(want["hse_down"].mean()), "cn10", float(want["cn10"].mean()), "entries that differ:", diff, file=sys.stderr)
    assert np.array_equal(_bits(got), _bits(X.arrays_of(want))), tag
    assert b[0] == 256.0 and np.array_equal(_bits(b[1:8]), _bits(X.header_of(want))), tag
    assert np.array_equal(_bits(b[16:32]), np.zeros(16, dtype=np.uint32)), tag
    return want


def _no_native(block, L):
    b = block.cpu().numpy()
    assert b[8] == 0.0 and np.array_equal(_bits(b[9:16]), np.zeros(7, dtype=np.uint32)) and np.isnan(b[32 + 8 * L:]).all()
    assert b.shape == (32 + 16 * L,)


# ------------------------------------------------------------------------------------------------ 1. length sweep
@pytest.mark.parametrize("L", LENGTHS)
def test_length_sweep(eng, points, L):
    """Synthetic weights, one-row alignments, -n 0 -m 0: collapsed models, hundreds of candidates per atom."""
    aln, coords0, confs0 = _trace(eng, L)
    coords, confs = eng.predict(aln, None, 0, 0, exposure=True)
    eng.sync_check()
    assert eng.get_option("exposure") == 0
    assert torch.equal(coords, coords0) and torch.equal(confs, confs0) and tuple(confs.shape) == (L,)
    assert tuple(eng.exposure_block.shape) == (32 + 16 * L,) and eng.ss_block is None
    want = _model_leg(eng.exposure_block, coords, aln[0], points, f"sweep L={L}")
    _no_native(eng.exposure_block, L)
    ex = eng.exposure
    assert np.array_equal(ex["n"], want["n"]) and ex["atoms"] == want["atoms"] and not ex["has_native"]
    eng.predict(aln, None, 0, 0)
    eng.sync_check()
    assert eng.exposure is None and eng.exposure_block is None


# ------------------------------------------------------------------------------------------------ 2. glycines
def test_glycines(eng, points):
    L = 65
    aln = _one_row(L).copy()
    aln[0, [0, 7, 8, 31, 64]] = 7
    plain = eng.predict(aln, None, 0, 0)
    eng.sync_check()
    plain = [x.clone() for x in plain]
    coords, confs = eng.predict(aln, None, 0, 0, exposure=True)
    eng.sync_check()
    assert torch.equal(coords, plain[0]) and torch.equal(confs, plain[1])
    want = _model_leg(eng.exposure_block, coords, aln[0], points, "glycines")
    gly = aln[0] == 7
    b = eng.exposure_block.cpu().numpy()
    assert gly.sum() >= 5 and np.all(b[32 + 4 * L:32 + 5 * L][gly] == -1.0) and np.all(b[32 + 4 * L:32 + 5 * L][~gly] >= 0.0)
    assert b[1] == 5 * L - gly.sum() == want["atoms"]
    # no atom sees less than with those CB atoms in place
    none = X.exposure(coords.cpu().numpy(), np.zeros(L), points)
    assert (want["n"][~gly] >= none["n"][~gly]).all() and (want["n"][:, :4] >= none["n"][:, :4]).all()


# ------------------------------------------------------------------------------------------------ 3. the native leg
def _blob():
    return (np.random.default_rng(20260101).standard_normal((128, 3)) * 3.0).astype(np.float32)


NATIVES = {"helix": lambda: ideal_helix(64), "hairpin": flat_hairpin, "3fgx": native_3fgx, "blob": _blob}
_NATIVE_RUNS = {}


def _native_run(eng, name):
    """One prediction with the trace as native, made once: (aln, trace, block, the device's rebuilt backbone)."""
    if name not in _NATIVE_RUNS:
        trace = np.ascontiguousarray(NATIVES[name](), dtype=np.float32)
        L = trace.shape[0]
        aln, coords0, _ = _trace(eng, L)
        coords, _ = eng.predict(aln, None, 0, 0, native=trace, exposure=True)
        eng.sync_check()
        assert torch.equal(coords, coords0)
        _NATIVE_RUNS[name] = (aln, trace, eng.exposure_block.clone(), eng.fetch("exposure_native_backbone", 15 * L).cpu().numpy().reshape(L, 5, 3))
    return _NATIVE_RUNS[name]


def _native_leg(block, bb, first_row, points, tag):
    L = bb.shape[0]
    want = X.exposure(bb, first_row, points)
    b = block.cpu().numpy()
    got = b[32 + 8 * L:].reshape(8, L)
    print(tag, "area %.1f" % X.area(want["n"]), "sums", want["sums"], "buried", want["buried_atoms"], "entries that differ:",
          int((got != X.arrays_of(want)).sum()), "of", got.size, file=sys.stderr)
    assert b[8] == 1.0 and np.array_equal(_bits(got), _bits(X.arrays_of(want))), tag
    assert np.array_equal(_bits(b[9:16]), _bits(X.header_of(want))), tag
    return want


@pytest.mark.parametrize("name", list(NATIVES))
def test_native_leg_is_a_stage_entry(eng, points, name):
    """A trace fed as native: its leg equals the restatement on the NumPy `backbone` of that trace."""
    aln, trace, block, _ = _native_run(eng, name)
    want = _native_leg(block, backbone(trace), aln[0], points, f"native {name}")
    if name == "blob":
        cand = np.sqrt(((trace[:, None] - trace[None]) ** 2).sum(-1))
        print("blob: residues within 7 A of a residue, at most", int((cand < 7.0).sum(axis=1).max()), "buried atoms", want["buried_atoms"], file=sys.stderr)
        assert want["buried_atoms"] > 100                    # collapsed: the long candidate lists


@pytest.mark.parametrize("name", list(NATIVES))
def test_native_leg_on_the_backbone_the_device_rebuilt(eng, points, name):
    """The same leg against the restatement on the backbone the library itself rebuilt from the trace (dmp_debug_fetch
    "exposure_native_backbone"): no other code's arithmetic between the kernel and its yardstick."""
    aln, trace, block, bb = _native_run(eng, name)
    assert np.array_equal(_bits(bb[:, 1]), _bits(trace))
    _native_leg(block, bb, aln[0], points, f"native {name} (device backbone)")


# ------------------------------------------------------------------------------------------------ 4. chunking
@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunk_boundaries_change_no_bit(eng, chunk):
    aln, trace, block, _ = _native_run(eng, "blob")
    try:
        for bad in (-1, -2):
            with pytest.raises(Exception, match="exposure_chunk must be >= 0, got %d" % bad):
                eng.set_option("exposure_chunk", bad)
        eng.set_option("exposure_chunk", chunk)
        eng.predict(aln, None, 0, 0, native=trace, exposure=True)
        eng.sync_check()
        assert eng.get_option("exposure_chunk") == chunk
        assert np.array_equal(_bits(eng.exposure_block), _bits(block))
    finally:
        eng.set_option("exposure_chunk", 0)


# ------------------------------------------------------------------------------------------------ 5. has_native
def test_missing_native_row(eng, points):
    L = 65
    aln, coords0, _ = _trace(eng, L)
    native = ideal_helix(L)
    native[17] = np.nan
    eng.predict(aln, None, 0, 0, native=native)
    eng.sync_check()
    score0 = eng.score_block.clone()
    eng.predict(aln, None, 0, 0, exposure=True)
    eng.sync_check()
    alone = eng.exposure_block.clone()
    coords, _ = eng.predict(aln, None, 0, 0, native=native, exposure=True)
    eng.sync_check()
    assert torch.equal(coords, coords0)
    _no_native(eng.exposure_block, L)
    assert np.array_equal(_bits(eng.exposure_block), _bits(alone)) and np.array_equal(_bits(eng.score_block), _bits(score0))
    assert not eng.exposure["has_native"] and "native" not in eng.exposure


def test_the_models_own_trace_as_native(eng, points):
    L = 64
    aln, coords0, _ = _trace(eng, L)
    eng.predict(aln, None, 0, 0, exposure=True)
    eng.sync_check()
    alone = eng.exposure_block.cpu().numpy()
    native = coords0[:, 1].cpu().numpy().copy()
    coords, _ = eng.predict(aln, None, 0, 0, native=native, exposure=True)
    eng.sync_check()
    assert torch.equal(coords, coords0)
    b = eng.exposure_block.cpu().numpy()
    assert b[8] == 1.0 and np.array_equal(_bits(b[32:32 + 8 * L]), _bits(b[32 + 8 * L:])) and np.array_equal(_bits(b[1:8]), _bits(b[9:16]))
    # the model's leg does not depend on the native
    assert np.array_equal(_bits(b[:8]), _bits(alone[:8])) and np.array_equal(_bits(b[32:32 + 8 * L]), _bits(alone[32:32 + 8 * L]))
    other = eng.predict(aln, None, 0, 0, native=ideal_helix(L), exposure=True)
    eng.sync_check()
    c = eng.exposure_block.cpu().numpy()
    assert np.array_equal(_bits(c[:8]), _bits(alone[:8])) and np.array_equal(_bits(c[32:32 + 8 * L]), _bits(alone[32:32 + 8 * L]))
    assert not np.array_equal(_bits(c[32 + 8 * L:]), _bits(b[32 + 8 * L:])) and torch.equal(other[0], coords0)


# ------------------------------------------------------------------------------------------------ 6. repeatability
def test_two_runs_give_the_same_bits(eng):
    aln, trace, block, _ = _native_run(eng, "3fgx")
    for _ in range(2):
        eng.predict(aln, None, 0, 0, native=trace, exposure=True)
        eng.sync_check()
        assert np.array_equal(_bits(eng.exposure_block), _bits(block))


# ------------------------------------------------------------------------------------------------ 7. every extra at once
def test_beside_every_other_extra(eng, points):
    from test_align_cpu import indel_copy, moved, random_walk
    L = 65
    aln, coords0, confs0 = _trace(eng, L)
    model = coords0[:, 1].cpu().numpy()
    lib = S.Library.from_traces([indel_copy(model, 51, m=61)[0], random_walk(30, 5), moved(model, 3)[2]])
    native = moved(model, 4)[2]
    structure = indel_copy(model, 52, m=70)[0]
    kw = dict(distmap=True, native=native, structure=structure, library=lib, score_map=True, score_passes=True, ss=True)
    names = ("score_block", "map_score_block", "pass_block", "ss_block", "align_block", "search_block")
    off = eng.predict(aln, None, 2, 0, **kw)
    eng.sync_check()
    off = [x.clone() for x in off]
    blocks0 = [getattr(eng, n).clone() for n in names]
    assert eng.exposure_block is None
    on = eng.predict(aln, None, 2, 0, exposure=True, **kw)
    eng.sync_check()
    assert len(on) == len(off) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(on, off))
    for n, b0 in zip(names, blocks0):
        assert np.array_equal(_bits(getattr(eng, n)), _bits(b0)), n
    full = eng.exposure_block.clone()
    assert full[8].item() == 1.0
    eng.predict(aln, None, 2, 0, native=native, exposure=True)
    eng.sync_check()
    assert np.array_equal(_bits(eng.exposure_block), _bits(full))
    coords, _ = eng.predict(aln, None, 2, 0, exposure=True)
    eng.sync_check()
    alone, f = eng.exposure_block.cpu().numpy(), full.cpu().numpy()
    assert np.array_equal(_bits(alone[:8]), _bits(f[:8])) and np.array_equal(_bits(alone[32:32 + 8 * L]), _bits(f[32:32 + 8 * L]))
    _model_leg(eng.exposure_block, coords, aln[0], points, "every extra L=65")


# ------------------------------------------------------------------------------------------------ 8. precisions
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_three_precisions(synth_sd, points, precision):
    from dmpfold2_amd.predict import Engine
    L = 33
    aln = _one_row(L)
    e = Engine("cuda:0", L, 4)
    try:
        e.set_weights(_tensors(synth_sd))
        e.set_option("precision", precision)
        plain = [x.clone() for x in e.predict(aln, None, 1, 10)]
        e.sync_check()
        coords, confs = e.predict(aln, None, 1, 10, exposure=True)
        e.sync_check()
        assert torch.equal(coords, plain[0]) and torch.equal(confs, plain[1])
        _model_leg(e.exposure_block, coords, aln[0], points, f"precision {precision}")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 9. pipeline
def test_pipeline(synth_sd):
    from dmpfold2_amd.predict import Engine, Pipeline
    lengths = [40, 24, 64]
    alns = [_one_row(L) for L in lengths]
    dev, sdt = torch.device("cuda:0"), _tensors(synth_sd)
    single = Engine(dev, 64, 1)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 64, 1, sdt, streams=2, precision=2, exposure=True)
    try:
        assert all(e.get_option("exposure") == 1 for e in pipe.engines)
        refs = []
        for aln in alns:
            c, f = single.predict(aln, None, 1, 0, exposure=True)
            single.sync_check()
            refs.append((c.clone(), f.clone(), single.exposure_block.clone()))
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), 1, 0) for a in alns]
        res = pipe.collect(tickets)
        for t, ref, L in zip(tickets, refs, lengths):
            assert not isinstance(res[t], Exception), res[t]
            coords, confs, block = res[t]
            assert tuple(confs.shape) == (L,) and tuple(block.shape) == (32 + 16 * L,)
            assert torch.equal(coords, ref[0]) and torch.equal(confs, ref[1]) and np.array_equal(_bits(block), _bits(ref[2])), L
        pipe.engines[1].set_option("exposure", 0)
        with pytest.raises(RuntimeError, match="exposure"):
            pipe.submit(torch.from_numpy(alns[0]).to(dev), 1, 0)
        pipe.set_exposure(False)
        out = pipe.run([torch.from_numpy(alns[0]).to(dev)], 1, 0)
        pipe.sync_check()
        assert len(out[0]) == 2 and torch.equal(out[0][0], refs[0][0])
    finally:
        pipe.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 10. fault
def test_latched_fault_gives_nan_in_the_whole_block(synth_sd):
    """The persistent vertical GRU launched one workgroup short (the test option other tests use): its row barrier times out
    once, DMP_FAULT_VGRU_HANDOFF is latched, and the exposure block is NaN like every other output."""
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, encode_aln, FAULT_VGRU_HANDOFF
    L = 33
    msa = encode_aln(synth.synth_msa(L, 16, 78))
    e = Engine("cuda:0", L, 16)
    try:
        e.set_weights(_tensors(synth_sd))
        e.set_option("vgru_persistent", 1)
        e.set_option("vgru_debug_drop_wg", 1)
        c, f = e.predict_device(torch.from_numpy(msa).to(e.device), None, 0, 0, exposure=True)
        bits = e.sync_faults()
        assert bits & FAULT_VGRU_HANDOFF and bool(torch.isnan(f).all())
        assert tuple(e.exposure_block.shape) == (32 + 16 * L,) and bool(torch.isnan(e.exposure_block).all())
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 11. the option
def test_option_values_and_scratch():
    from dmpfold2_amd import _lib
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 256, 4)
    try:
        assert e.get_option("exposure") == 0 and e.get_option("exposure_chunk") == 0
        before = e.get_option("device_mib")
        for bad in (2, -1, 4096):
            with pytest.raises(_lib.DmpError, match="exposure must be 0 or 1, got %d" % bad):
                e.set_option("exposure", bad)
        e.set_option("exposure", 0)
        assert e.get_option("exposure") == 0 and e.get_option("device_mib") == before
        e.set_option("exposure", 1)
        assert e.get_option("exposure") == 1 and before <= e.get_option("device_mib") <= before + 1
        grown = e.get_option("device_mib")
        e.set_option("exposure", 0)
        e.set_option("exposure", 1)
        assert e.get_option("device_mib") == grown
        e.set_option("exposure", 0)
        assert e.get_option("exposure") == 0
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 12. front ends
def test_front_ends(tmp_path, weights_file, monkeypatch, points):
    """`dmpfold --exposure [--exposure-file FILE]` and `dmpfold-batch --exposure`: stdout byte for byte the run's without the
    option, the JSON line the dict of aln_to_coords(..., return_exposure=True), the batch's files and summary carry the same."""
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
        L = plain[0].shape[0]
        c, f, alnmat, ex = aln_to_coords(str(p), return_alnmat=True, return_exposure=True, **kw)
        assert L == 48 and torch.equal(c, plain[0]) and torch.equal(f, plain[1]) and P._ENGINES[0].get_option("exposure") == 0
        want_counts = X.exposure(c.cpu().numpy(), alnmat[0], points)
        assert np.array_equal(ex["n"], want_counts["n"]) and np.array_equal(ex["cn10"], want_counts["cn10"]) and not ex["has_native"]
        assert ex["area"] == pytest.approx(X.area(want_counts["n"]), rel=1e-12) and "burial_ratio" in ex
        want = json.loads(json.dumps({"exposure": S.exposure_json(ex)}))
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file]
        texts, errs = [], []
        for extra in ([], ["--exposure"], ["--exposure", "--exposure-file", str(tmp_path / "exposure.json")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        assert json.loads(errs[1].strip().split("\n")[-1]) == want and "exposure" not in errs[0] and "exposure" not in errs[2]
        assert json.loads((tmp_path / "exposure.json").read_text()) == want
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--exposure"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 1 and summary["exposure_targets"] == 1
            assert summary["exposure"]["t48"]["area"] == want["exposure"]["area"]
            assert summary["mean_exposure_area"] == want["exposure"]["area"] == summary["median_exposure_area"]
            assert summary["mean_exposure_burial_ratio"] == want["exposure"]["burial_ratio"] and "mean_exposure_r_area" not in summary
            if fmt == "pdb":
                assert (out_dir / "t48.pdb").read_text() == texts[0]
                assert json.loads((out_dir / "t48.exposure.json").read_text()) == want
            else:
                z = np.load(str(out_dir / "t48.npz"))
                assert np.array_equal(z["coords"], c.cpu().numpy()) and np.array_equal(z["exp_n"], ex["n"]) and z["exp_n"].shape == (L, 5)
                assert np.array_equal(z["exp_hse_up"], ex["hse_up"]) and np.array_equal(z["exp_hse_down"], ex["hse_down"])
                assert np.array_equal(z["exp_cn10"], ex["cn10"]) and np.array_equal(z["exp_area"], ex["area_res"])
    finally:
        P._ENGINES.clear()
