"""Structural domains of the predicted model on the GPU (option "domains"; include/dmpfold_hip.h).

The library's domain block is compared with tests/domains_ref.py, the NumPy restatement of the header's definition, evaluated
on the float32 coordinates the same call returned.  Every output is an integer: every comparison is exact, bit for bit; there
is no tolerance anywhere.  On the parent commit the option is unknown and every test here fails."""
import sys

import numpy as np
import pytest
import torch

import domains_ref as R
from test_align_cpu import random_walk

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

LENGTHS = [8, 15, 16, 17, 63, 64, 65, 79, 80, 81, 255, 256, 257]
DEFAULTS = dict(domains_tau=0.25, domains_min_size=40, domains_min_segment=10)
FORCED = dict(domains_tau=1.0, domains_min_size=8, domains_min_segment=2)        # every admissible cut is accepted


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float32)).reshape(-1).view(np.uint32)


def _ref(params):
    return dict(tau_milli=int(round(params["domains_tau"] * 1000)), min_size=params["domains_min_size"],
                min_segment=params["domains_min_segment"])


@pytest.fixture(scope="module")
def eng(synth_sd):
    """One engine (seed-0 weights, precision 2) for the single-engine tests."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 300, 64)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


def _one_row(L):
    from dmpfold2_amd import synth
    return np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L)))


_TRACES = {}
_SEEN = {}                           # what the forced sweep met, by length: the restatement's header


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


def _same_block(block, want, tag):
    got = block.cpu().numpy()
    assert got.shape == want.shape, tag
    differ = np.flatnonzero(_bits(got) != _bits(want))
    print(tag, "header", got[:8].tolist(), "native", got[16:24].tolist(), "floats that differ:", differ[:8].tolist(), file=sys.stderr)
    assert differ.size == 0, tag


# ------------------------------------------------------------------------------------------------ 1. length sweep
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("params", [DEFAULTS, FORCED], ids=["defaults", "forced"])
def test_length_sweep(eng, L, params):
    """Synthetic weights, one-row alignments, -n 0 -m 0: collapsed models, which mostly stay whole at the defaults."""
    aln, coords0, confs0 = _trace(eng, L)
    coords, confs = eng.predict_domains(aln, None, 0, 0, **params)
    eng.sync_check()
    assert all(eng.get_option(name) == v for name, v in (("domains", 0), ("domains_tau_milli", 250), ("domains_min_size", 40),
                                                         ("domains_min_segment", 10)))
    assert torch.equal(coords, coords0) and torch.equal(confs, confs0) and tuple(confs.shape) == (L,)
    assert tuple(eng.domains_block.shape) == (32 + 2 * L + 256,) and eng.exposure_block is None
    want = R.parse(_ca(coords), **_ref(params))
    _same_block(eng.domains_block, R.block(want), f"sweep L={L} {params['domains_min_size']}")
    dom = eng.domains
    assert np.array_equal(dom["labels"], want["labels"]) and dom["domains"] == want["header"][0] and not dom["has_native"]
    assert [row["size"] for row in dom["table"]] == want["table"][:, 0].tolist() and all("rg" in row and "mean_conf" in row for row in dom["table"])
    if params is FORCED:
        _SEEN[L] = want
    eng.predict(aln, None, 0, 0)
    eng.sync_check()
    assert eng.domains is None and eng.domains_block is None


def test_forced_sweep_met_every_path():
    """The forced sweep accepts every admissible cut: among its lengths are sixteen domains, a domain of several segments, a
    final domain of level 4 that was large enough to examine - and a chain too short to examine at all."""
    assert set(_SEEN) == set(LENGTHS)
    headers = {L: p["header"] for L, p in _SEEN.items()}
    print("forced sweep:", headers, file=sys.stderr)
    assert max(h[0] for h in headers.values()) == 16 and any(h[5] > 0 for h in headers.values())
    assert any(h[7] == 1 for h in headers.values()) and headers[257][6] == 4
    assert headers[8][0] == 1 and headers[15][0] == 1 and headers[16][0] >= 1


# ------------------------------------------------------------------------------------------------ 2. the native's leg
@pytest.mark.parametrize("name", ["80+80", "100+150", "3x80", "insertion"])
def test_native_leg_on_constructed_traces(eng, name):
    native, built = R.constructed(name)
    L = native.shape[0]
    aln, coords0, confs0 = _trace(eng, L)
    coords, confs = eng.predict_domains(aln, None, 0, 0, native=native)
    eng.sync_check()
    assert torch.equal(coords, coords0) and torch.equal(confs, confs0)
    model, nat = R.parse(_ca(coords)), R.parse(native)
    _same_block(eng.domains_block, R.block(model, nat), name)
    dom = eng.domains
    assert dom["has_native"] and np.array_equal(dom["native"]["labels"], nat["labels"])
    assert 0.0 < dom["overlap"] <= 1.0
    if name != "insertion":
        assert np.array_equal(nat["labels"], built), name             # the constructed boundaries themselves
    else:
        assert nat["header"][0] == 2 and nat["table"][0, 1] == 2 and nat["table"][1, 1] == 1


def test_native_with_a_missing_row_has_no_leg(eng):
    native, _ = R.constructed("80+80")
    native = native.copy()
    native[17] = np.nan
    aln, coords0, _ = _trace(eng, 160)
    coords, _ = eng.predict_domains(aln, None, 0, 0, native=native)
    eng.sync_check()
    _same_block(eng.domains_block, R.block(R.parse(_ca(coords))), "native with a NaN row")
    b = eng.domains_block.cpu().numpy()
    assert not b[16:32].any() and np.isnan(b[32 + 160:32 + 320]).all() and not b[32 + 320 + 128:].any() and not eng.domains["has_native"]


# ------------------------------------------------------------------------------------------------ 3. beside the other blocks
def test_alone_and_beside_the_seven_other_blocks_engine_and_pipeline(synth_sd):
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, Pipeline
    L, N, ITERATIONS, MINSTEPS = 24, 4, 1, 5
    OTHERS = ("score_block", "align_block", "search_block", "map_score_block", "pass_block", "ss_block", "exposure_block")
    aln = np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, N, 1024)))
    native = random_walk(L, 1).astype(np.float32)
    native[5] = np.nan
    structure = random_walk(12, 2).astype(np.float32)
    library = S.Library.from_traces([random_walk(8, 3), random_walk(12, 4)])
    everything = dict(distmap=True, native=native, structure=structure, library=library, score_map=True, score_passes=True, ss=True,
                      exposure=True)
    dev, sdt = torch.device("cuda:0"), _tensors(synth_sd)
    eng = Engine(dev, L, N)
    eng.set_weights(sdt)
    eng.set_option("precision", 2)
    eng.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, L, N, sdt, streams=2, precision=2, distmap=True, score=True, align=True, search=library, score_map=True,
                    score_passes=True, ss=True, exposure=True)
    try:
        without = [x.clone() for x in eng.predict(aln, None, ITERATIONS, MINSTEPS, **everything)]
        eng.sync_check()
        blocks = {name: getattr(eng, name).clone() for name in OTHERS}
        assert eng.domains_block is None
        # alone
        coords, confs = eng.predict_domains(aln, None, ITERATIONS, MINSTEPS, **FORCED)
        eng.sync_check()
        alone = eng.domains_block.clone()
        assert np.array_equal(_bits(coords), _bits(without[0])) and np.array_equal(_bits(confs), _bits(without[1]))
        assert all(getattr(eng, name) is None for name in OTHERS)
        _same_block(alone, R.block(R.parse(_ca(coords), **_ref(FORCED))), "alone")
        assert alone[0].item() >= 2.0                                  # (24 residues, min_size 8: a cut is admissible)
        # beside all seven
        full = [x.clone() for x in eng.predict_domains(aln, None, ITERATIONS, MINSTEPS, **FORCED, **everything)]
        eng.sync_check()
        assert len(full) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(full, without))
        assert np.array_equal(_bits(eng.domains_block), _bits(alone))
        for name in OTHERS:
            assert np.array_equal(_bits(getattr(eng, name)), _bits(blocks[name])), name
        # the pipeline without the option: what it has always handed out
        ticket = pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure)
        res = pipe.collect([ticket])[ticket]
        assert not isinstance(res, Exception), res
        assert len(res) == 4 + len(OTHERS)
        # ... and with it: the domain block last of all, everything else the same bits
        pipe.use_domains(True, FORCED["domains_tau"], FORCED["domains_min_size"], FORCED["domains_min_segment"])
        tickets = [pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure) for _ in range(2)]
        got = pipe.collect(tickets)
        for t in tickets:
            assert not isinstance(got[t], Exception), got[t]
            assert len(got[t]) == 5 + len(OTHERS)
            for name, a, b in zip(("coords", "confs", "distmap", "info") + OTHERS, got[t], without + [blocks[n] for n in OTHERS]):
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), name
            assert np.array_equal(_bits(got[t][-1]), _bits(alone))
        # engines that disagree
        pipe.engines[1].set_option("domains", 0)
        with pytest.raises(RuntimeError, match="domains"):
            pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS)
        pipe.engines[1].set_option("domains", 1)
        pipe.engines[1].set_option("domains_min_size", 9)
        with pytest.raises(RuntimeError, match="domains_min_size"):
            pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS)
        pipe.use_domains(False)
    finally:
        pipe.close()
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. option errors
def test_option_errors(eng):
    for name, bad in (("domains", 2), ("domains", -1), ("domains_tau_milli", 0), ("domains_tau_milli", 1001), ("domains_min_size", 7),
                      ("domains_min_size", 1025), ("domains_min_segment", 0), ("domains_min_segment", 65)):
        before = eng.get_option(name)
        with pytest.raises(Exception, match=name):
            eng.set_option(name, bad)
        assert eng.get_option(name) == before
    aln, coords0, confs0 = _trace(eng, 17)
    # min_segment above min_size: each value is in range, the prediction does not begin
    eng.set_option("domains_min_size", 8)
    eng.set_option("domains_min_segment", 9)
    eng.set_option("domains", 1)
    try:
        with pytest.raises(Exception, match="domains_min_segment"):
            eng.predict(aln, None, 0, 0)
        eng.set_option("domains", 0)
        coords, confs = eng.predict(aln, None, 0, 0)                   # with the option off the pair is not looked at
        eng.sync_check()
        assert torch.equal(coords, coords0) and torch.equal(confs, confs0)
    finally:
        eng.set_domains(False)
        eng.set_option("domains_min_size", 40)
        eng.set_option("domains_min_segment", 10)
    with pytest.raises(ValueError):
        eng.predict_domains(aln, None, 0, 0, domains_min_size=8, domains_min_segment=9)
    with pytest.raises(ValueError):
        eng.predict_domains(aln, None, 0, 0, domains_tau=0.0)
    assert eng.get_option("domains") == 0


# ------------------------------------------------------------------------------------------------ 5. front ends
def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --domains [...]` and `dmpfold-batch --domains [...]`: stdout byte for byte the run's without the option, the JSON
    line the dict of aln_to_domains, the batch's files and summary carry the same parse."""
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
        forced = dict(domains_tau=1.0, domains_min_size=8, domains_min_segment=2)
        flags = ["--domains", "--domains-tau", "1.0", "--domains-min-size", "8", "--domains-min-segment", "2"]
        plain = aln_to_coords(str(p), **kw)
        c, f, alnmat, dom = P.aln_to_domains(str(p), return_alnmat=True, **kw, **forced)
        assert c.shape[0] == 48 and torch.equal(c, plain[0]) and torch.equal(f, plain[1])
        assert P._ENGINES[0].get_option("domains") == 0 and P._ENGINES[0].get_option("domains_min_size") == 40
        ref = R.parse(_ca(c), **_ref(forced))
        assert np.array_equal(dom["labels"], ref["labels"]) and dom["domains"] == ref["header"][0] >= 2 and not dom["has_native"]
        assert all("rg" in row and "mean_conf" in row for row in dom["table"])
        want = json.loads(json.dumps({"domains": S.domains_json(dom)}))
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file]
        texts, errs = [], []
        for extra in ([], flags, flags + ["--domains-file", str(tmp_path / "domains.json")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        assert json.loads(errs[1].strip().split("\n")[-1]) == want and "domains" not in errs[0] and "domains" not in errs[2]
        assert json.loads((tmp_path / "domains.json").read_text()) == want
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2"] + flags)
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 1 and summary["domain_targets"] == 1 and batch._DOMAINS is None
            assert summary["domains"]["t48"]["domains"] == dom["domains"] == summary["mean_domains"] == summary["median_domains"]
            assert summary["multi_domain_share"] == 1.0 and summary["domains"]["t48"]["sizes"] == [row["size"] for row in dom["table"]]
            if fmt == "pdb":
                assert (out_dir / "t48.pdb").read_text() == texts[0]
                assert json.loads((out_dir / "t48.domains.json").read_text()) == want
            else:
                z = np.load(str(out_dir / "t48.npz"))
                assert np.array_equal(z["coords"], c.cpu().numpy()) and np.array_equal(z["dom_label"], dom["labels"])
                assert np.array_equal(z["dom_table"], ref["table"])
    finally:
        P._ENGINES.clear()
