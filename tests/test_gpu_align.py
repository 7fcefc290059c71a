"""A prediction aligned with a structure of any length on the GPU (option "align_structure"; include/dmpfold_hip.h).

Every number is compared with the float64 yardstick of tests/test_align_cpu.py, fed the float32 model trace the GPU returned
and the same structure: ali, n_ali, seed_offset and seeds exactly, the floats within one float32 ulp (compare_alignment).
A case whose yardstick margin is below 1e-9 fails with "choose another seed"; the seeds below were fixed with the yardstick
so that none does.  The largest differences seen are printed.
"""
import contextlib
import io
import json
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_rows
from test_align_cpu import compare_alignment, indel_copy, moved, random_walk, yardstick

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

GUARD = 4096
MAX_L = 257
LENGTHS = [8, 31, 32, 33, 63, 64, 65, 255, 256, 257]
KINDS = ["same", "shorter", "longer"]
# seed of the indel-and-noise copy per (L, kind), where the default 100 + L + 1000 * KINDS.index(kind) gave a near tie
SEEDS = {}


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


@pytest.fixture(scope="module")
def eng(synth_sd):
    """One engine (seed-0 weights, precision 2, max_L = 257) for the single-engine tests."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", MAX_L, 64)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


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


def _aligned(eng, aln, structure, iterations=0, minsteps=0, **kw):
    """(outputs, alignment dict) of a prediction with `structure`; the option is off again afterwards."""
    out = eng.predict(aln, None, iterations, minsteps, structure=structure, **kw)
    eng.sync_check()
    assert eng.get_option("align_structure") == 0
    return out, eng.alignment


def _check(al, coords, structure, tag):
    want, margin = yardstick(coords[:, 1].cpu().numpy(), structure)
    print(tag, "n_ali %d tm_model %.4f margin %.2e" % (want["n_ali"], want["tm_model"], margin), file=sys.stderr)
    seen = compare_alignment(al, want, margin, tag)
    print(tag, "largest differences in float32 ulps:", seen, file=sys.stderr)
    return want


def _m_of(L, kind):
    return {"same": L, "shorter": max(L - 3, 3), "longer": min(L + 5, MAX_L)}[kind]


def _bits(x):
    return (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)).reshape(-1).view(np.uint32)


def _outs(block, L):
    return block[1:25 + 2 * L]


# ------------------------------------------------------------------------------------------------ 1. length sweep
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_length_sweep(eng, L, kind):
    """The structure: an indel-and-noise copy of the model's own trace with m rows.  (On the parent commit the option is
    unknown: the call raises.)"""
    aln, coords0, confs0 = _trace(eng, L)
    m = _m_of(L, kind)
    structure, _ = indel_copy(coords0[:, 1].cpu().numpy(), SEEDS.get((L, kind), 100 + L + 1000 * KINDS.index(kind)), m=m)
    assert structure.shape == (m, 3)
    (coords, confs), al = _aligned(eng, aln, structure)
    assert torch.equal(coords, coords0) and torch.equal(confs, confs0)
    assert al["m"] == float(m) and np.array_equal(al["structure"], structure)
    want = _check(al, coords, structure, f"sweep L={L} m={m}")
    assert al["seeds"] == L + m - 2 * max(min(L, m) // 2, min(5, L, m)) + 1
    assert np.array_equal(np.isnan(al["deviation"]), want["ali"] < 0) and al["n_ali"] == int((al["ali"] >= 0).sum())
    assert eng.align_block[21:25].cpu().tolist() == [0.0] * 4


# ------------------------------------------------------------------------------------------------ 2. smallest m, bad input
def test_smallest_m(eng):
    """m = 3 against L = 8: 6 seeds, a 3 x 8 DP, at most 3 pairs."""
    aln, coords0, _ = _trace(eng, 8)
    model = coords0[:, 1].cpu().numpy()
    _, _, structure = moved(model[2:5].astype(np.float64) + np.random.default_rng(4).normal(scale=0.3, size=(3, 3)), 4)
    (coords, _), al = _aligned(eng, aln, structure)
    assert torch.equal(coords, coords0)
    assert al["seeds"] == 6 and al["n_ali"] <= 3
    _check(al, coords, structure, "smallest m")


def _raw(eng, aln, iterations=0, emit=False, score_block=None, align_block=None, fill=float("nan")):
    """dmp_predict into a poisoned buffer with the blocks' inputs in place -> (coords, buffer with its guard, n_out)."""
    L = aln.shape[1]
    m = None if align_block is None else (len(align_block) - S.align_floats(L, 0)) // 3
    n_out = S.conf_floats(L, emit, score_block is not None, m)
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.full((15 * L + GUARD,), fill, dtype=torch.float32, device=eng.device)
    buf = torch.full((n_out + GUARD,), fill, dtype=torch.float32, device=eng.device)
    if score_block is not None:
        s0 = S.score_offset(L, emit)
        buf[s0:s0 + len(score_block)] = torch.from_numpy(score_block).to(eng.device)
    if align_block is not None:
        a0 = S.align_offset(L, emit, score_block is not None)
        buf[a0:n_out] = torch.from_numpy(align_block).to(eng.device)
    opts = (("emit_distmap", int(emit)), ("score_native", int(score_block is not None)), ("align_structure", int(align_block is not None)))
    for k, v in opts:
        eng.set_option(k, v)
    try:
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), aln.shape[0], L, None, 0, iterations, 0, coords.data_ptr(),
                                 buf.data_ptr(), eng.stream())
        assert rc == 0, eng.lib.dmp_last_error()
        bits = eng.sync_faults()
    finally:
        for k, _ in opts:
            eng.set_option(k, 0)
    return coords, buf, n_out, bits


@pytest.mark.parametrize("case", ["m=2", "m=2.5", "m=max_L+1", "NaN coordinate"])
def test_bad_input(eng, case):
    """Every out slot NaN, the inputs untouched, no fault, the structure the plain run's bits."""
    L = 33
    aln, coords0, confs0 = _trace(eng, L)
    walk = random_walk(MAX_L + 1, 12)
    if case == "m=2":
        block = S.pack_structure(walk[:2], L)
    elif case == "m=2.5":
        block = S.pack_structure(walk[:20], L, m_value=2.5)
    elif case == "m=max_L+1":
        block = S.pack_structure(walk, L)
    else:
        bad = walk[:20].copy()
        bad[7, 1] = np.nan
        block = S.pack_structure(bad, L)
    coords, buf, n_out, bits = _raw(eng, aln, align_block=block)
    h = buf.cpu().numpy()
    assert bits == 0
    assert np.array_equal(_bits(coords[:15 * L]), _bits(coords0)) and np.array_equal(_bits(h[:L]), _bits(confs0))
    got = h[L:n_out]
    assert np.isnan(_outs(got, L)).all(), np.nonzero(~np.isnan(_outs(got, L)))[0]
    assert np.array_equal(_bits(got[:1]), _bits(block[:1])) and np.array_equal(_bits(got[25 + 2 * L:]), _bits(block[25 + 2 * L:]))
    assert np.isnan(h[n_out:]).all()
    al = S.unpack_alignment(got, L)
    assert al["n_ali"] == 0 and (al["ali"] == -1).all() and S.alignment_json(al)["tm_struct"] is None


def test_option_values(eng):
    from dmpfold2_amd import _lib
    for bad in (2, -1):
        with pytest.raises(_lib.DmpError):
            eng.set_option("align_structure", bad)
    assert eng.get_option("align_structure") == 0
    eng.set_option("align_structure", 1)
    assert eng.get_option("align_structure") == 1
    eng.set_option("align_structure", 0)
    with pytest.raises(ValueError):
        eng.predict(_one_row(8), None, 0, 0, structure=np.zeros((5, 2)))
    assert eng.get_option("align_structure") == 0


# ------------------------------------------------------------------------------------------------ 3. rigid copy at capacity
def test_rigid_copy_L2048(synth_sd):
    """The only place the LDS diagonals, the direction scratch and the 2 x 2048 - 2 x 1024 + 1 seed records are reached.
    No yardstick here (it would take minutes), the properties of a rigid copy instead."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 2048, 1)
    try:
        e.set_weights(_tensors(synth_sd))
        e.set_option("precision", 2)
        aln = _one_row(2048)
        coords0, _ = e.predict(aln, None, 0, 0)
        e.sync_check()
        model = coords0[:, 1].cpu().numpy()
        R, t, structure = moved(model, 9)
        (coords, _), al = _aligned(e, aln, structure)
        assert torch.equal(coords, coords0)
        print("rigid L=2048: tm", al["tm_model"], al["tm_struct"], "rmsd", al["rmsd_ali"], "seed_offset", al["seed_offset"],
              "max|R - R0|", float(np.abs(al["R"] - R).max()), "max|t - t0|", float(np.abs(al["t"] - t).max()), file=sys.stderr)
        assert al["seeds"] == 2 * 2048 - 2 * 1024 + 1 and al["n_ali"] == 2048
        assert np.array_equal(al["ali"], np.arange(2048))
        assert al["tm_model"] >= 1.0 - 1e-6 and al["tm_struct"] >= 1.0 - 1e-6 and al["rmsd_ali"] <= 1e-4
        assert np.abs(al["R"] - R).max() <= 1e-5 and np.abs(al["t"] - t).max() <= 1e-5
        assert float(al["deviation"].max()) <= 1e-3
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. with the other options
def test_option_off_and_on(eng):
    """"align_structure" 0 and 1 crossed with "emit_distmap" and "score_native": coords, confs, map, info and score block
    bit for bit the same throughout; the raw buffer exactly conf_floats(...) long with the block at its documented offset;
    a convergence stop leaves the block of the equivalent -n p run."""
    L = 65
    aln = _one_row(L)
    plain, _ = eng.predict(aln, None, 2, 0)
    eng.sync_check()
    model = plain[:, 1].cpu().numpy()
    structure, _ = indel_copy(model, 51, m=61)
    native = random_walk(L, 21)
    native[::9] = np.nan
    ablock, sblock = S.pack_structure(structure, L), S.pack_native(native, 0.0, L)
    ref_align = None
    for emit in (False, True):
        for score in (False, True):
            c0, b0, n0, bits0 = _raw(eng, aln, 2, emit, sblock if score else None, None)
            c1, b1, n1, bits1 = _raw(eng, aln, 2, emit, sblock if score else None, ablock)
            assert bits0 == 0 and bits1 == 0
            assert n0 == S.conf_floats(L, emit, score) and n1 == n0 + S.align_floats(L, 61) == S.conf_floats(L, emit, score, 61)
            assert np.array_equal(_bits(c0), _bits(c1)), (emit, score)
            assert np.array_equal(_bits(b0[:n0]), _bits(b1[:n0])), (emit, score)
            assert bool(torch.isnan(b0[n0:]).all()) and bool(torch.isnan(b1[n1:]).all()), "a guard float was written"
            assert np.array_equal(_bits(c0[:15 * L]), _bits(plain))
            blk = b1[S.align_offset(L, emit, score):n1].cpu().numpy()
            assert not np.isnan(_outs(blk, L)[:24]).any()
            assert np.array_equal(_bits(blk[:1]), _bits(ablock[:1])) and np.array_equal(_bits(blk[25 + 2 * L:]), _bits(ablock[25 + 2 * L:]))
            if ref_align is None:
                ref_align = blk
                _check(S.unpack_alignment(blk, L), plain, structure, "off and on L=65")
            assert np.array_equal(_bits(blk), _bits(ref_align)), (emit, score)
    # the Python route: the same block, views of one allocation, the options off again
    (c, f, dm, info), al = _aligned(eng, aln, structure, 2, 0, distmap=True, native=native)
    assert [eng.get_option(k) for k in ("emit_distmap", "score_native", "align_structure")] == [0, 0, 0]
    assert np.array_equal(_bits(eng.align_block), _bits(ref_align)) and torch.equal(c, plain)
    assert eng.align_block.data_ptr() == f.data_ptr() + 4 * S.align_offset(L, True, True)
    assert eng.score_block.data_ptr() == f.data_ptr() + 4 * S.score_offset(L, True)
    # a tolerance so wide that the first comparison stops the recycling: passes 0 and 1 run
    (c3, f3), _ = _aligned(eng, aln, structure, 6, 0, converge=1e3)
    blk3 = eng.align_block.cpu().numpy().copy()
    assert eng.passes_run == 2 and eng.get_option("recycle_tol_mA") == 0
    (c4, f4), _ = _aligned(eng, aln, structure, 1, 0)
    assert torch.equal(c3, c4) and torch.equal(f3, f4)
    assert np.array_equal(_bits(blk3), _bits(eng.align_block))
    # the option set by hand, no structure given: m = 0, NaN in every out slot
    eng.set_option("align_structure", 1)
    try:
        out = eng.predict(aln, None, 2, 0)
        eng.sync_check()
        assert len(out) == 2 and torch.equal(out[0], plain)
        blk = eng.align_block.cpu().numpy()
        assert blk.shape == (25 + 2 * L,) and blk[0] == 0.0 and np.isnan(blk[1:]).all() and eng.alignment["n_ali"] == 0
    finally:
        eng.set_option("align_structure", 0)
    out = eng.predict(aln, None, 2, 0)
    eng.sync_check()
    assert eng.alignment is None and eng.align_block is None


# ------------------------------------------------------------------------------------------------ 5. software-latched fault
def test_latched_fault_gives_nan_in_every_out_slot(eng):
    """A residue code of 22 raises the device-side flag DMP_FAULT_BAD_CODE (a software flag, not a GPU fault): every out
    slot of the align block (and of the score block in front of it) is NaN, m and the structure are as the caller wrote
    them, the guard stays."""
    from dmpfold2_amd.predict import FAULT_BAD_CODE
    L = 33
    aln = _one_row(L).copy()
    aln[0, 5] = 22
    structure = random_walk(29, 8)
    native = random_walk(L, 9)
    ablock, sblock = S.pack_structure(structure, L), S.pack_native(native, 40.0, L)
    coords, buf, n_out, bits = _raw(eng, aln, 1, False, sblock, ablock, fill=7.0)
    assert bits == FAULT_BAD_CODE
    h = buf.cpu().numpy()
    a0 = S.align_offset(L, False, True)
    assert bool(torch.isnan(coords[:15 * L]).all()) and np.isnan(h[:L]).all()
    assert np.array_equal(h[L:L + 3 * L + 1], sblock[:3 * L + 1]) and np.isnan(h[L + 3 * L + 1:a0]).all()
    assert h[a0] == 29.0 and np.isnan(h[a0 + 1:a0 + 25 + 2 * L]).all()
    assert np.array_equal(h[a0 + 25 + 2 * L:n_out], structure.reshape(-1)), "the structure was touched"
    assert (h[n_out:] == 7.0).all(), "the NaN fill went past the align block"
    aln_ok, coords0, _ = _trace(eng, L)
    structure, _ = indel_copy(coords0[:, 1].cpu().numpy(), 133, m=30)
    (c, _), al = _aligned(eng, aln_ok, structure)                   # the next prediction on the engine is whole again
    _check(al, c, structure, "after a fault L=33")


# ------------------------------------------------------------------------------------------------ 6. pipeline
@pytest.mark.parametrize("streams", [2, 4])
def test_pipeline(synth_sd, streams):
    """Six targets of mixed length, structures of mixed length, two targets without one (m = 0, NaN outs): every ticket's
    align block is bit for bit the lone context's; engines that disagree on the option raise; with the option off `result`
    has its old shape."""
    from dmpfold2_amd.predict import Engine, Pipeline
    lengths = [40, 24, 64, 33, 40, 57]
    ms = [37, 31, None, 64, 3, None]
    alns = [_one_row(L) for L in lengths]
    dev = torch.device("cuda:0")
    sdt = _tensors(synth_sd)
    single = Engine(dev, 64, 1)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 64, 1, sdt, streams=streams, precision=2)
    try:
        structures, refs = [], []
        single.set_option("align_structure", 1)
        for k, (aln, m) in enumerate(zip(alns, ms)):
            structures.append(None if m is None else random_walk(m, 400 + k))
            c, f = single.predict(aln, None, 1, 0, structure=structures[-1])
            single.sync_check()
            refs.append((c.clone(), f.clone(), single.align_block.clone()))
        single.set_option("align_structure", 0)
        assert all(e.get_option("align_structure") == 0 for e in pipe.engines)
        t = pipe.submit(torch.from_numpy(alns[0]).to(dev), 1, 0, structure=structures[0])          # ignored: the option is off
        pipe.drain()
        pipe.sync_check()
        old = pipe.result(t)
        assert len(old) == 2 and torch.equal(old[0], refs[0][0]) and torch.equal(old[1], refs[0][1])
        pipe.engines[0].set_option("align_structure", 1)
        with pytest.raises(RuntimeError, match="align_structure"):
            pipe.submit(torch.from_numpy(alns[0]).to(dev), 1, 0, structure=structures[0])
        pipe.set_align(True)
        assert all(e.get_option("align_structure") == 1 for e in pipe.engines)
        with pytest.raises(RuntimeError):
            pipe.submit(torch.from_numpy(alns[0]).to(dev), 1, 0, structure=random_walk(65, 1))      # beyond the capacity
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), 1, 0, structure=s) for a, s in zip(alns, structures)]
        res = pipe.collect(tickets)
        for t, ref, L, m in zip(tickets, refs, lengths, ms):
            assert not isinstance(res[t], Exception), res[t]
            coords, confs, block = res[t]
            assert tuple(confs.shape) == (L,) and tuple(block.shape) == (25 + 2 * L + 3 * (m or 0),)
            assert torch.equal(coords, ref[0]) and torch.equal(confs, ref[1])
            assert np.array_equal(_bits(block), _bits(ref[2])), (L, m)
            al = S.unpack_alignment(block, L)
            if m is None:
                assert al["m"] == 0.0 and np.isnan(block[1:].cpu().numpy()).all()
            else:
                assert 3 <= al["n_ali"] <= min(L, m) and 0.0 < al["tm_model"] <= 1.0
        pipe.set_align(False)
        out = pipe.run([torch.from_numpy(alns[2]).to(dev)], 1, 0)
        pipe.sync_check()
        assert len(out[0]) == 2 and torch.equal(out[0][0], refs[2][0])
    finally:
        pipe.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 7. front ends
def _write_pdb(path, ca, chain="A"):
    with open(path, "w") as fh:
        for k, xyz in enumerate(ca):
            fh.write("ATOM  %5d  CA  %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n"
                     % (k + 1, S.AA3[k % 20], chain, k + 1, xyz[0], xyz[1], xyz[2]))
        fh.write("TER\nEND\n")


def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --compare`: stdout byte for byte the run's without it, the JSON line (stderr or --alignment FILE) the numbers
    of Engine.alignment; aln_to_coords(compare=, return_alignment=True) behind return_scores; `dmpfold-batch --structures`:
    summary, npz arrays and <stem>.alignment.json carry the same numbers, the target without a file has no alignment."""
    import dmpfold2_amd.predict as P
    from dmpfold2_amd import aln_to_coords, run_dmpfold
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        paths = []
        for name, stem in (("pf10963_n3_m0", "pf"), ("synth_L40_N64_n2_m0", "s40")):
            p = tmp_path / f"{stem}.aln"
            p.write_text("\n".join(golden_rows(load_golden(name))) + "\n")
            paths.append(str(p))
        structs = tmp_path / "structures"
        structs.mkdir()
        kw = dict(device="cuda:0", iterations=1, minsteps=0, weights_file=weights_file)
        plain = aln_to_coords(paths[0], **kw)
        L = plain[0].shape[0]
        # a structure in PDB precision (three decimals), longer than the model
        structure, _ = indel_copy(plain[0][:, 1].cpu().numpy(), 77, m=L + 9)
        _write_pdb(str(structs / "pf.pdb"), structure)
        structure = S.read_native_ca(str(structs / "pf.pdb"))[0]
        c, f, al = aln_to_coords(paths[0], compare=str(structs / "pf.pdb"), return_alignment=True, **kw)
        assert torch.equal(c, plain[0]) and torch.equal(f, plain[1])
        assert np.array_equal(al["structure"], structure) and al["m"] == L + 9 and al["n_ali"] >= 3
        assert P._ENGINES[0].get_option("align_structure") == 0
        _check(al, c, structure, "front end pf")
        both = aln_to_coords(paths[0], native=np.full((L, 3), np.nan, dtype=np.float32), return_scores=True,
                             compare=structure, compare_chain=None, return_alignment=True, **kw)
        assert len(both) == 4 and both[2]["n_pairs"] == 0 and np.array_equal(both[3]["ali"], al["ali"])
        assert aln_to_coords(paths[0], return_alignment=True, **kw)[-1] is None
        want = S.alignment_json(al)
        args = ["-i", paths[0], "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file]
        texts, errs = [], []
        for extra in ([], ["--compare", str(structs / "pf.pdb")],
                      ["--compare", str(structs / "pf.pdb"), "--compare-chain", "A", "--alignment", str(tmp_path / "pf.json")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        assert json.loads(errs[1].strip().split("\n")[-1]) == want and "tm_model" not in errs[2]
        assert json.loads((tmp_path / "pf.json").read_text()) == want
        header = {k: want[k] for k in ("m",) + S.ALIGN_NAMES}
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i"] + paths + ["-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--structures", str(structs)])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 2 and summary["aligned_targets"] == 1 and summary["alignments"] == {"pf": header}
            if fmt == "pdb":
                assert (out_dir / "pf.pdb").read_text() == texts[0] and (out_dir / "s40.pdb").exists()
                assert json.loads((out_dir / "pf.alignment.json").read_text()) == want
                assert not (out_dir / "s40.alignment.json").exists()
            else:
                z = np.load(str(out_dir / "pf.npz"))
                assert np.array_equal(z["coords"], c.cpu().numpy()) and np.array_equal(z["confs"], f.cpu().numpy())
                assert float(z["tm_model"]) == al["tm_model"] and int(z["n_ali"]) == al["n_ali"]
                assert np.array_equal(z["ali"], al["ali"]) and np.array_equal(z["ali_R"], al["R"])
                assert np.array_equal(z["ali_deviation"], al["deviation"], equal_nan=True)
                z40 = np.load(str(out_dir / "s40.npz"))
                assert "ali" not in z40.files and "coords" in z40.files
    finally:
        P._ENGINES.clear()
