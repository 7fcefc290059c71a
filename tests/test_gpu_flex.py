"""Slow modes and residue flexibility of the model on the GPU (option "flex"; include/dmpfold_hip.h).

The library's flex block is compared with tests/flex_ref.py, the NumPy restatement of the header's definition: the integers
exactly, eigenvalues, modes and msf within the bounds that module derives from the number formats (MARGIN = 8; no constant
from a kernel's output).  The native's leg is a folded-like globule, where every kept eigenvalue stands alone and the
comparison is in full; the model's leg of a one-row alignment with -n 0 -m 0 is a collapsed trace, a nearly complete graph with
a degenerate spectrum, and is held to the integers and to the invariants that hold for any basis.  Every test prints its
largest error / bound per check.  On the parent commit the option and the names do not exist and every test here fails.

Largest error / bound seen on an MI355X (pytest -s, test_worst_ratios): see profiles/flex.txt."""
import sys

import numpy as np
import pytest
import torch

import domains_ref as D
import flex_ref as F
from test_align_cpu import random_walk

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

# all eight pairs wanted (8, 9), one wave's rows (63, 64, 65), the 64-step chain and the tile edges of flex_kirchhoff_kernel (16
# rows, 256 columns: 16, 257), backtransform_kernel<10, 2> (321), tri_eig_kernel<1> (385)
LENGTHS = [8, 9, 16, 63, 64, 65, 129, 257, 321, 385]
WORST = {}                           # check -> (ratio, where): the largest over every comparison of this module


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float32)).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def eng(synth_sd):
    """One engine (seed-0 weights, precision 2) for the single-engine tests."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 400, 8)
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


def _ca(coords):
    return np.ascontiguousarray(coords.cpu().numpy()[:, 1])


def _held(ref, got, tag):
    """flex_ref.check of one leg: printed, recorded, asserted."""
    res = F.check(ref, got)
    print(tag, {k: (round(r, 4), note) for k, (r, note) in res.items()}, file=sys.stderr)
    for k, (r, note) in res.items():
        if r >= WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (r, f"{tag}: {note}")
    assert not F.failed(res), (tag, res)
    return res


def _run(eng, L, native=None, cutoff=7.3, **kw):
    """One prediction with the option on -> (block as float32 array, header, legs); outputs must be the plain run's bits."""
    aln, coords0, confs0 = _trace(eng, L)
    coords, confs = eng.predict_flex(aln, None, 0, 0, flex_cutoff=cutoff, native=native, **kw)
    eng.sync_check()
    assert eng.get_option("flex") == 0 and eng.get_option("flex_cut_mA") == 7300
    assert torch.equal(coords, coords0) and torch.equal(confs, confs0) and tuple(confs.shape) == (L,)
    assert tuple(eng.flex_block.shape) == (48 + 20 * L,) == (S.flex_floats(L),)
    blk = eng.flex_block.cpu().numpy().copy()
    hdr, legs = F.split(blk, L)
    assert hdr[0] == L and hdr[1] == int(round(cutoff * 1000)) and not hdr[3:].any()
    return blk, hdr, legs, coords


def _no_leg(leg):
    return not leg["header"].any() and all(np.isnan(leg[k]).all() for k in ("degree", "msf", "modes"))


# ------------------------------------------------------------------------------------------------ 1. length sweep
@pytest.mark.parametrize("L", LENGTHS)
def test_length_sweep(eng, L):
    native = D.globule(L, 0)
    blk, hdr, legs, coords = _run(eng, L, native)
    assert hdr[2] == 1.0
    ref = F.leg(native)
    res = _held(ref, legs[1], f"sweep L={L} native")
    assert ref.msf_comparable and res["msf"][1] != "n/a" and res["mode"][1] != "n/a"      # (test_flex_cpu.py holds the generator to it)
    model = F.leg(_ca(coords))
    _held(model, legs[0], f"sweep L={L} model")
    print(f"sweep L={L} model: contacts {model.contacts} of {L * (L - 1) // 2}, sigma {model.sigma}", file=sys.stderr)
    fx = eng.flex
    assert fx["has_native"] and fx["native"]["components"] == 1 and fx["native"]["used"] == 7 and fx["L"] == L and fx["cutoff"] == 7.3
    assert fx["native"]["hinges"] == F.hinges(legs[1]["modes"][1]) and len(fx["native"]["collectivity"]) == 7
    assert np.array_equal(fx["native"]["degree"], ref.degree) and "r_conf" in fx and "rmsip" in fx
    # without a native: the model's leg keeps its bits, the native's part is zero / NaN
    blk2, hdr2, legs2, _ = _run(eng, L)
    assert hdr2[2] == 0.0 and _no_leg(legs2[1])
    assert np.array_equal(_bits(blk2[16:32]), _bits(blk[16:32])) and np.array_equal(_bits(blk2[48:48 + 10 * L]), _bits(blk[48:48 + 10 * L]))
    eng.predict(_trace(eng, L)[0], None, 0, 0)
    eng.sync_check()
    assert eng.flex is None and eng.flex_block is None


# ------------------------------------------------------------------------------------------------ 2. constructed natives
@pytest.mark.parametrize("name", ["80+80", "3x80", "insertion"])
def test_constructed_natives_and_the_parse(eng, name):
    native, built = D.constructed(name)
    L = native.shape[0]
    with eng.with_domains():
        blk, hdr, legs, coords = _run(eng, L, native)
        fx, dom = eng.flex, eng.domains
    ref = F.leg(native)
    _held(ref, legs[1], f"{name} native")
    _held(F.leg(_ca(coords)), legs[0], f"{name} model")
    # the host's hinge / parse agreement against the reference's: the native's parse, its first cut, the reference's own mode
    parse = D.parse(native)
    assert dom["has_native"] and np.array_equal(dom["native"]["labels"], parse["labels"])
    nodes = parse["nodes"]
    side_a = np.array([(int(k) >> (int(k).bit_length() - 2)) == 2 for k in nodes])      # the level-1 ancestor is node 2
    assert side_a.any() and not side_a.all()
    want = F.parse_agreement(ref.modes[1], side_a)
    print(name, "hinges", fx["native"]["hinges"], "parse agreement", fx["native"]["parse_agreement"], "reference", want, file=sys.stderr)
    assert fx["native"]["parse_agreement"] == want and want > 0.85
    assert fx["native"]["hinges"] == F.hinges(ref.modes[1]) and fx["native"]["first_mode"] == 1
    if name == "80+80":
        assert any(abs(h - 79.5) <= 5 for h in fx["native"]["hinges"])
        assert fx["native"]["eigenvalues"][1] < 0.6 * fx["native"]["eigenvalues"][2]


# ------------------------------------------------------------------------------------------------ 3. disconnected, missing row
def test_disconnected_native(eng):
    a, b = D.globule(64, 0), D.globule(65, 1)
    native = np.concatenate([a, b - b.mean(0) + a.mean(0) + np.asarray([200.0, 0.0, 0.0], dtype=np.float32)]).astype(np.float32)
    blk, hdr, legs, _ = _run(eng, 129, native)
    ref = F.leg(native)
    assert ref.components == 2 and ref.used == 6
    _held(ref, legs[1], "disconnected native")
    assert legs[1]["header"][2] == 2.0 and legs[1]["header"][3] == 6.0
    fx = eng.flex["native"]
    assert fx["first_mode"] == 2 and len(fx["collectivity"]) == 6


def test_native_with_a_missing_row_has_no_leg(eng):
    native, _ = D.constructed("80+80")
    whole, _, _, _ = _run(eng, 160, native)
    native = native.copy()
    native[17] = np.nan
    blk, hdr, legs, _ = _run(eng, 160, native)
    assert hdr[2] == 0.0 and _no_leg(legs[1]) and not eng.flex["has_native"]
    assert np.array_equal(_bits(blk[16:32]), _bits(whole[16:32])) and np.array_equal(_bits(blk[48:48 + 1600]), _bits(whole[48:48 + 1600]))


# ------------------------------------------------------------------------------------------------ 4. cutoffs, option errors
@pytest.mark.parametrize("cutoff", [4.0, 20.0])
def test_cutoffs(eng, cutoff):
    native = D.globule(96, 0)
    blk, hdr, legs, coords = _run(eng, 96, native, cutoff)
    ref = F.leg(native, int(cutoff * 1000))
    print("cutoff", cutoff, "contacts", ref.contacts, "sigma", ref.sigma, "lambda_1", ref.eigenvalues[1], file=sys.stderr)
    assert ref.connected() and (ref.contacts == 95 if cutoff == 4.0 else ref.contacts > 96 * 95 // 4)
    _held(ref, legs[1], f"cutoff {cutoff} native")
    _held(F.leg(_ca(coords), int(cutoff * 1000)), legs[0], f"cutoff {cutoff} model")


def test_option_errors(eng):
    for name, bad in (("flex", 2), ("flex", -1), ("flex_cut_mA", 3999), ("flex_cut_mA", 20001)):
        before = eng.get_option(name)
        with pytest.raises(Exception, match=name):
            eng.set_option(name, bad)
        assert eng.get_option(name) == before
    for bad in (3.9, 20.5, float("nan")):
        with pytest.raises(ValueError):
            eng.set_flex(True, bad)
        with pytest.raises(ValueError):
            eng.predict_flex(_trace(eng, 16)[0], None, 0, 0, flex_cutoff=bad)
    assert eng.get_option("flex") == 0 and eng.get_option("flex_cut_mA") == 7300
    eng.set_flex(True, 9.0)
    assert eng.get_option("flex") == 1 and eng.get_option("flex_cut_mA") == 9000
    eng.set_flex(False)
    eng.set_option("flex_cut_mA", 7300)
    assert eng.get_option("flex") == 0


# ------------------------------------------------------------------------------------------------ 5. the same bits
def test_two_runs_give_the_same_bits_and_the_solver_scratch_is_its_own(eng):
    native = D.globule(129, 0)
    aln, coords0, _ = _trace(eng, 129)
    eng.predict(aln, None, 0, 0)                                       # (the fetch hands out the last prediction's)
    mds0, gram0 = eng.fetch("mds", 129 * 8).clone(), eng.fetch("gram", 129 * 129).clone()
    eng.sync_check()
    first, _, _, _ = _run(eng, 129, native)
    mds1, gram1 = eng.fetch("mds", 129 * 8).clone(), eng.fetch("gram", 129 * 129).clone()
    second, _, _, _ = _run(eng, 129, native)
    assert np.array_equal(_bits(first), _bits(second))
    assert mds0.numel() == 129 * 8 and np.array_equal(_bits(mds0), _bits(mds1)) and np.array_equal(_bits(gram0), _bits(gram1))


def test_alone_and_beside_every_other_block_engine_and_pipeline(synth_sd):
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, Pipeline
    L, N, ITERATIONS, MINSTEPS = 24, 4, 1, 5
    OTHERS = ("score_block", "align_block", "search_block", "map_score_block", "pass_block", "ss_block", "exposure_block")
    MORE = ("domains_block", "domain_score_block")
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
    # (the engines of a pipeline of several take the Householder steps as one launch each: the form whose bits theirs are - inside
    # a cluster of equal eigenvalues, and a collapsed model has little else, the two forms may return different bases)
    eng.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, L, N, sdt, streams=2, precision=2, distmap=True, score=True, align=True, search=library, score_map=True,
                    score_passes=True, ss=True, exposure=True)
    try:
        with eng.with_domains(**FORCED), eng.with_score_domains():
            without = [x.clone() for x in eng.predict(aln, None, ITERATIONS, MINSTEPS, **everything)]
            eng.sync_check()
            blocks = {name: getattr(eng, name).clone() for name in OTHERS + MORE}
            assert eng.flex_block is None
        # alone
        coords, confs = eng.predict_flex(aln, None, ITERATIONS, MINSTEPS)
        eng.sync_check()
        alone = eng.flex_block.clone()
        assert np.array_equal(_bits(coords), _bits(without[0])) and np.array_equal(_bits(confs), _bits(without[1]))
        assert all(getattr(eng, name) is None for name in OTHERS + MORE)
        _, legs = F.split(alone.cpu().numpy(), L)
        _held(F.leg(_ca(coords)), legs[0], "alone")
        # beside all nine
        with eng.with_domains(**FORCED), eng.with_score_domains():
            full = [x.clone() for x in eng.predict_flex(aln, None, ITERATIONS, MINSTEPS, **everything)]
            eng.sync_check()
            beside = eng.flex_block.clone()
            for name in OTHERS + MORE:
                assert np.array_equal(_bits(getattr(eng, name)), _bits(blocks[name])), name
        assert len(full) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(full, without))
        assert beside[2].item() == 1.0 and np.array_equal(_bits(beside[16:32]), _bits(alone[16:32]))
        assert np.array_equal(_bits(beside[48:48 + 10 * L]), _bits(alone[48:48 + 10 * L]))
        _, legs = F.split(beside.cpu().numpy(), L)
        _held(F.leg(native), legs[1], "beside, native")
        # the pipeline without the option: what it has always handed out
        ticket = pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure)
        res = pipe.collect([ticket])[ticket]
        assert not isinstance(res, Exception), res
        assert len(res) == 4 + len(OTHERS)
        # ... and with it: the same tuple, the same bits, the flex block on the target's Outputs
        pipe.use_flex(True)
        tickets = [pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure) for _ in range(2)]
        got = pipe.collect(tickets)
        for t in tickets:
            assert not isinstance(got[t], Exception), got[t]
            assert len(got[t]) == 4 + len(OTHERS)
            for name, a, b in zip(("coords", "confs", "distmap", "info") + OTHERS, got[t], without + [blocks[n] for n in OTHERS]):
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), name
            assert np.array_equal(_bits(pipe.collected[t].flex_block), _bits(beside))
        # engines that disagree
        pipe.engines[1].set_option("flex", 0)
        with pytest.raises(RuntimeError, match="flex"):
            pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS)
        pipe.engines[1].set_option("flex", 1)
        pipe.engines[1].set_option("flex_cut_mA", 8000)
        with pytest.raises(RuntimeError, match="flex_cut_mA"):
            pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS)
        pipe.use_flex(False)
    finally:
        pipe.close()
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. front ends
def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --flex [...]` and `dmpfold-batch --flex [...]`: stdout byte for byte the run's without the option, the JSON line
    the dict of aln_to_flex, the batch's files and summary carry the same figures."""
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
        flags = ["--flex", "--flex-cutoff", "9.5"]
        plain = aln_to_coords(str(p), **kw)
        c, f, alnmat, fx = P.aln_to_flex(str(p), return_alnmat=True, **kw, flex_cutoff=9.5)
        assert c.shape[0] == 48 and torch.equal(c, plain[0]) and torch.equal(f, plain[1])
        assert P._ENGINES[0].get_option("flex") == 0 and P._ENGINES[0].get_option("flex_cut_mA") == 7300
        ref = F.leg(_ca(c), 9500)
        assert fx["cutoff"] == 9.5 and not fx["has_native"] and fx["contacts"] == ref.contacts and fx["sigma"] == ref.sigma
        assert np.array_equal(fx["degree"], ref.degree) and "r_conf" in fx and "rho_conf" in fx
        _held(ref, {"header": np.r_[[fx[k] for k in S.FLEX_FIELDS], np.zeros(4), fx["eigenvalues"]].astype(np.float32),
                    "degree": fx["degree"].astype(np.float32), "msf": fx["msf"], "modes": fx["modes"]}, "aln_to_flex")
        want = json.loads(json.dumps({"flex": S.flex_json(fx)}))
        with pytest.raises(ValueError):
            P.aln_to_flex(str(p), **kw, flex_cutoff=3.0)
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file]
        texts, errs = [], []
        for extra in ([], flags, flags + ["--flex-file", str(tmp_path / "flex.json")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        assert json.loads(errs[1].strip().split("\n")[-1]) == want and "flex" not in errs[0] and "flex" not in errs[2]
        assert json.loads((tmp_path / "flex.json").read_text()) == want
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                # (one stream: the pipeline's one engine then tridiagonalises in the form aln_to_flex's does, and the collapsed
                # model's degenerate modes come in the same basis - see the test above)
                rc = batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "1"] + flags)
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 1 and summary["flex_targets"] == 1 and batch._FLEX is None
            brief = summary["flex"]["t48"]
            assert brief["components"] == fx["components"] == summary["mean_flex_components"] and brief["hinges"] == len(fx["hinges"])
            assert brief["lambda_1"] == want["flex"]["eigenvalues"][fx["first_mode"]] == summary["median_flex_lambda_1"]
            assert brief["r_conf"] == want["flex"]["r_conf"]
            if fmt == "pdb":
                assert (out_dir / "t48.pdb").read_text() == texts[0]
                assert json.loads((out_dir / "t48.flex.json").read_text()) == want
            else:
                z = np.load(str(out_dir / "t48.npz"))
                assert np.array_equal(z["coords"], c.cpu().numpy())
                assert np.array_equal(_bits(z["flex_eig"]), _bits(fx["eigenvalues"].astype(np.float32)))
                assert np.array_equal(_bits(z["flex_modes"]), _bits(fx["modes"])) and z["flex_modes"].shape == (8, 48)
                assert np.array_equal(_bits(z["flex_msf"]), _bits(fx["msf"])) and np.array_equal(z["flex_degree"], fx["degree"])
    finally:
        P._ENGINES.clear()


def test_worst_ratios():
    """The largest error / bound per check over every comparison above (pytest -s prints it; profiles/flex.txt records it)."""
    print("flex: largest error / bound per check:", {k: (round(r, 4), where) for k, (r, where) in sorted(WORST.items())}, file=sys.stderr)
    assert WORST and all(r <= 1.0 for r, _ in WORST.values())
