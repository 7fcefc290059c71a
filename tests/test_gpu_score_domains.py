"""Every domain of the model scored against the native on the GPU (option "score_domains"; include/dmpfold_hip.h).

Row (leg, d) is defined as what "score_native" returns for the same model trace and a native masked to the domain, with lnorm 0.
Two yardsticks: that masked call on the same engine, bit for bit (1); the float64 restatement of tests/score_domains_ref.py, by
the rule of test_score_cpu.compare_with_yardstick - integer-derived values exact, tm, rmsd, R, t and the deviations within 1
float32 ulp - with the four pair counts exact (2).  One engine (max_L = 257, synthetic weights, precision 2), one-row
alignments, 0 recycling passes and 0 minimiser steps throughout.  The native of a length is the model's own trace with each of
the model's domains moved by its own rigid transform, plus small noise: it is whole, so both legs exist.  On the parent commit
the option is unknown and every test here fails."""
import contextlib
import sys

import numpy as np
import pytest
import torch

import domains_ref as R
import score_domains_ref as DR
from test_score_cpu import NEAR_TIE, compare_with_yardstick

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

MAX_L = 257
GUARD = 4096
DEFAULTS = dict(tau=0.25, min_size=40, min_segment=10)
FORCED = dict(tau=1.0, min_size=8, min_segment=2)            # every admissible cut is accepted
FORCED_REF = dict(tau_milli=1000, min_size=8, min_segment=2)
MULTI = (17, 65, 257)
NOISE = 0.3                                                   # Angstrom, of the native's residues


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


@pytest.fixture(scope="module")
def eng(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", MAX_L, 64)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


def _one_row(L):
    from dmpfold2_amd import synth
    return np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L)))


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float32)).reshape(-1).view(np.uint32)


_PLAIN = {}


def _plain(eng, L):
    """The plain prediction of the one-row alignment of length L, made once: (aln, coords, confs, C-alpha trace)."""
    if L not in _PLAIN:
        aln = _one_row(L)
        coords, confs = eng.predict(aln, None, 0, 0)
        eng.sync_check()
        _PLAIN[L] = (aln, coords.clone(), confs.clone(), np.ascontiguousarray(coords.cpu().numpy()[:, 1]))
    return _PLAIN[L]


def _scored(eng, aln, native, lnorm=0.0, params=DEFAULTS, **asked):
    """One prediction with every domain scored -> dict of host copies.  Every option is as it was afterwards."""
    with eng.with_domains(**params), eng.with_score_domains():
        coords, confs = eng.predict(aln, None, 0, 0, native=(native, lnorm), **asked)[:2]
        eng.sync_check()
    assert [eng.get_option(k) for k in ("score_domains", "domains", "score_native")] == [0, 0, 0]
    return dict(coords=coords.clone(), confs=confs.clone(), dom=eng.domains_block.cpu().numpy().copy(),
                score=eng.score_block.cpu().numpy().copy(), ds=eng.domain_score_block.cpu().numpy().copy(), un=eng.domain_scores)


def _masked_call(eng, aln, native, labels, d):
    """"score_native" alone with the native masked to domain d, lnorm 0 -> the score block."""
    eng.predict(aln, None, 0, 0, native=(DR.masked(native, labels, d), 0.0))
    eng.sync_check()
    assert eng.domain_score_block is None
    return eng.score_block.cpu().numpy().copy()


def _labels(dom, L):
    """(labels, D) of both legs of a domain block."""
    return [(dom[32 + e * L:32 + (e + 1) * L].astype(np.int64), int(dom[16 * e])) for e in range(2)]


def _row_equals_masked_call(ds, sb, L, leg, d, labels, tag):
    """Check 1 for one row: floats 1 .. 23 and the two arrays on the domain's residues, in bits."""
    un = S.unpack_domain_scores(ds, L)
    row, hdr = un["table"][leg, d], sb[3 * L:3 * L + 24]
    assert np.array_equal(_bits(row[1:24]), _bits(hdr[1:24])), (tag, np.flatnonzero(_bits(row[1:24]) != _bits(hdr[1:24])) + 1)
    mine = labels == d
    for k, name in enumerate(("lddt_res", "deviation")):
        got, want = un["res"][2 * leg + k][mine], sb[3 * L + 24 + k * L:3 * L + 24 + (k + 1) * L][mine]
        assert np.array_equal(_bits(got), _bits(want)), (tag, name)
    assert row[0] == hdr[1], (tag, "n")
    return un


_MULTI = {}


def _multi(eng, L):
    """Made once per length and left unchanged: the forced parse of the plain prediction, the native made from it, the scored
    prediction."""
    if L not in _MULTI:
        aln, coords0, confs0, model = _plain(eng, L)
        parse = R.parse(model, **FORCED_REF)
        native = DR.moved_by_domain(model, parse["labels"], noise=NOISE, seed=L)
        got = _scored(eng, aln, native, params=FORCED)
        legs = _labels(got["dom"], L)
        assert np.array_equal(legs[0][0], parse["labels"]) and legs[0][1] == parse["header"][0], "the library's parse is the restatement's"
        assert legs[1][1] >= 1, "the native is whole: its leg exists"
        _MULTI[L] = dict(aln=aln, model=model, native=native, got=got, legs=legs)
    return _MULTI[L]


# ------------------------------------------------------------------------------------------------ 1. the definition, in bits
def _chosen(dom, L, leg, D):
    """At L = 257: the first, the last, the smallest and a domain of several segments (every domain at the shorter lengths)."""
    if L < 257:
        return list(range(D))
    table = dom[32 + 2 * L + 128 * leg:32 + 2 * L + 128 * (leg + 1)].reshape(16, 8)[:D]
    split = [d for d in range(D) if table[d, 1] > 1]
    return sorted({0, D - 1, int(np.argmin(table[:, 0]))} | set(split[:1]))


@pytest.mark.parametrize("L", MULTI)
def test_every_row_is_the_masked_call_in_bits(eng, L):
    c = _multi(eng, L)
    ds, dom = c["got"]["ds"], c["got"]["dom"]
    assert ds.shape == (S.domain_score_floats(L),) and ds[0] == c["legs"][0][1] and ds[1] == c["legs"][1][1] and ds[2] == L
    assert (ds[3:16] == 0).all()
    for leg, (labels, D) in enumerate(c["legs"]):
        table = dom[32 + 2 * L + 128 * leg:32 + 2 * L + 128 * (leg + 1)].reshape(16, 8)
        for d in _chosen(dom, L, leg, D):
            sb = _masked_call(eng, c["aln"], c["native"], labels, d)
            un = _row_equals_masked_call(ds, sb, L, leg, d, labels, f"L={L} leg {leg} domain {d}")
            row = un["table"][leg, d]
            assert row[0] == (labels == d).sum() and row[28] == table[d, 0] and (row[29:] == 0).all()
        un = S.unpack_domain_scores(ds, L)
        assert np.isnan(un["table"][leg, D:]).all() and not np.isnan(un["table"][leg, :D]).any()
        assert not np.isnan(un["res"][2 * leg:2 * leg + 2]).any(), "every residue lies in a domain of three rows or more"
    assert any(D > 1 for _, D in c["legs"]) or L == 17


# ------------------------------------------------------------------------------------------------ 2. the float64 yardstick
@pytest.mark.parametrize("L", MULTI)
def test_every_row_against_the_yardstick(eng, L):
    c = _multi(eng, L)
    un = c["got"]["un"]
    assert un["domains"] == c["legs"][0][1] and un["domains_native"] == c["legs"][1][1] and un["present"] == L and len(un["legs"]) == 2
    near = DR.near_pairs(c["native"])
    for leg, (labels, D) in enumerate(c["legs"]):
        want = DR.leg(c["model"], c["native"], labels, D)
        got = un["legs"][leg]
        for d in range(D):
            w, g = want["rows"][d], dict(got["rows"][d])
            mine = labels == d
            # compare_with_yardstick reads whole arrays: the domain's residues of both sides, NaN elsewhere on both
            for name in ("lddt_res", "deviation"):
                g[name] = np.where(mine, got[name], np.nan)
                w = dict(w, **{name: np.where(mine, want[name], np.nan)})
            seen = compare_with_yardstick(g, w, w["margin"], f"L={L} leg {leg} domain {d}")
            print(f"L={L} leg {leg} domain {d} (n={w['n']}): tm {w['tm']:.4f} margin {w['margin']:.2e} ulps", seen, file=sys.stderr)
            for name in ("n", "size", "preserved", "pairs", "outer_preserved", "outer_pairs"):
                assert g[name] == w[name], (L, leg, d, name, g[name], w[name])
        total = sum(r["pairs"] + r["outer_pairs"] for r in got["rows"])
        assert total == near, (L, leg, total, near)
        assert got["lddt_intra"] == sum(r["preserved"] for r in want["rows"]) / (4.0 * sum(r["pairs"] for r in want["rows"]))


def test_the_sweep_met_every_path(eng):
    """So that a change of weights cannot hollow the cases out: many domains, a domain of several segments, more than 256 rows
    in a leg, grids sized for more domains than there are, and pairs that leave a domain."""
    seen_split, most = False, 0
    for L in MULTI:
        c = _multi(eng, L)
        for leg, (labels, D) in enumerate(c["legs"]):
            table = c["got"]["dom"][32 + 2 * L + 128 * leg:32 + 2 * L + 128 * (leg + 1)].reshape(16, 8)[:D]
            seen_split |= bool((table[:, 1] > 1).any())
            most = max(most, D)
            assert D <= max(1, min(16, L // 8))
        for leg, (labels, D) in enumerate(c["legs"]):
            assert D == 1 or sum(r["outer_pairs"] for r in c["got"]["un"]["legs"][leg]["rows"]) > 0, (L, leg)
    assert most >= 8 and seen_split


# ------------------------------------------------------------------------------------------------ 3. one domain
@pytest.mark.parametrize("lnorm", [0.0, 40.0])
def test_one_domain_is_the_whole_chain(eng, lnorm):
    L = 16
    aln, coords0, confs0, model = _plain(eng, L)
    native = DR.moved_by_domain(model, np.zeros(L, dtype=np.int64), noise=NOISE, seed=3)
    got = _scored(eng, aln, native, lnorm=lnorm)
    assert got["dom"][0] == 1 and got["dom"][16] == 1, "the default parse keeps both whole"
    ds, sb = got["ds"], got["score"]
    if lnorm:
        assert sb[3 * L] == lnorm
        sb = _masked_call(eng, aln, native, np.zeros(L, dtype=np.int64), 0)       # the whole call with lnorm 0, not the score block
        assert sb[3 * L] == 0.0 and not np.array_equal(_bits(sb[3 * L + 3:3 * L + 6]), _bits(got["score"][3 * L + 3:3 * L + 6]))
    for leg in range(2):
        un = _row_equals_masked_call(ds, sb, L, leg, 0, np.zeros(L, dtype=np.int64), f"lnorm {lnorm} leg {leg}")
        assert np.array_equal(_bits(un["res"][2 * leg]), _bits(sb[3 * L + 24:4 * L + 24]))
        assert np.array_equal(_bits(un["res"][2 * leg + 1]), _bits(sb[4 * L + 24:]))
        row = un["table"][leg, 0]
        assert row[0] == L and row[28] == L and row[26] == 0 and row[27] == 0 and row[25] == DR.near_pairs(native)
        assert np.isnan(un["table"][leg, 1:]).all()
    assert torch.equal(got["coords"], coords0) and torch.equal(got["confs"], confs0)


# ------------------------------------------------------------------------------------------------ 4. a partial native
def test_partial_native_starves_a_domain(eng):
    """Native rows absent, among them all but two of the smallest model domain and two rows elsewhere.  (Five absent rows cannot
    starve a domain here: "domains_min_size" is at least 8, so a domain keeps three rows unless six or more of its rows go.)"""
    L = 65
    c = _multi(eng, L)
    labels, D = c["legs"][0]
    starved = int(np.argmin([(labels == d).sum() for d in range(D)]))
    idx = np.flatnonzero(labels == starved)
    native = c["native"].copy()
    others = [i for i in range(L) if labels[i] != starved]
    gone = list(idx[:len(idx) - 2]) + [others[3], others[-4]]      # two rows of the domain stay
    native[gone] = np.nan
    got = _scored(eng, c["aln"], native, params=FORCED)
    ds, un = got["ds"], got["un"]
    assert got["dom"][16] == 0 and ds[1] == 0 and ds[0] == D and ds[2] == L - len(gone) and len(un["legs"]) == 1
    assert np.isnan(un["table"][1]).all() and np.isnan(un["res"][2:]).all(), "no leg of the native"
    row = un["table"][0, starved]
    pres, pairs, opres, opairs, margin = DR.pair_counts(c["model"], native, labels, starved)
    assert margin >= NEAR_TIE
    assert row[0] == 2 and row[1] == 2 and np.isnan(row[2:24]).all() and row[28] == len(idx) and (row[29:] == 0).all()
    assert row[24:28].tolist() == [pres, pairs, opres, opairs] and opairs > 0
    assert np.isnan(un["res"][0][gone]).all() and np.isnan(un["res"][1][gone]).all()
    assert np.isnan(un["res"][0][idx]).all() and np.isnan(un["res"][1][idx]).all(), "a domain of two rows has no per-residue values"
    for d in range(D):
        if d != starved:
            sb = _masked_call(eng, c["aln"], native, labels, d)
            _row_equals_masked_call(ds, sb, L, 0, d, labels, f"partial native, domain {d}")
    kept = np.setdiff1d(np.arange(L), np.concatenate([gone, idx]))
    assert not np.isnan(un["res"][:2, kept]).any()
    total = sum(r["pairs"] + r["outer_pairs"] for r in un["legs"][0]["rows"])
    assert total == DR.near_pairs(native)


# ------------------------------------------------------------------------------------------------ 5. nothing else changes
def test_every_other_block_keeps_its_bits(eng):
    from test_gpu_search import _library_for
    L = 65
    c = _multi(eng, L)
    lib = _library_for(c["model"])
    lib.domains = True
    watched = ("emit_distmap", "score_map", "score_passes", "assign_ss", "exposure", "domains", "search_structures", "search_domains",
               "score_native", "score_domains")
    before = [eng.get_option(k) for k in watched]
    asked = dict(distmap=True, score_map=True, score_passes=True, ss=True, exposure=True, library=lib)
    outs = {}
    for on in (0, 1):
        with contextlib.ExitStack() as stack:
            stack.enter_context(eng.with_domains(**FORCED))
            if on:
                stack.enter_context(eng.with_score_domains())
            res = eng.predict(c["aln"], None, 0, 0, native=(c["native"], 0.0), **asked)
            eng.sync_check()
            last = eng._last.out
            outs[on] = dict(coords=res[0].clone(), confs=res[1].clone(), distmap=res[2].clone(), info=res[3].clone(),
                            **{name: getattr(last, name).clone() for name in ("score_block", "map_block", "pass_block", "ss_block",
                                                                               "exposure_block", "domains_block", "domain_search_block",
                                                                               "search_block")},
                            ds=None if last.domain_score_block is None else last.domain_score_block.clone())
        assert [eng.get_option(k) for k in watched] == before, "the options read as before"
    assert outs[0]["ds"] is None and outs[1]["ds"].shape == (S.domain_score_floats(L),)
    for name in outs[0]:
        if name != "ds":
            assert np.array_equal(_bits(outs[0][name]), _bits(outs[1][name])), name
    assert np.array_equal(_bits(outs[1]["ds"]), _bits(c["got"]["ds"])), "the block does not depend on the other options"
    lib.domains = False


def test_raw_buffer_and_guard(eng):
    """dmp_predict into a poisoned buffer with "score_native", "domains" and "score_domains" alone: the block lies at the end of
    the domain block, the guard behind it stays, the result is the engine's."""
    L = 65
    c = _multi(eng, L)
    lay = S.Layout(L, score=True, domains=True, score_domains=True)
    assert lay.total == L + S.score_floats(L) + S.domains_floats(L) + S.domain_score_floats(L) and lay.domain_score_off + S.domain_score_floats(L) == lay.total
    d_msa = torch.from_numpy(c["aln"]).to(eng.device)
    coords = torch.full((15 * L + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    buf = torch.full((lay.total + GUARD,), 7.0, dtype=torch.float32, device=eng.device)
    buf[lay.score_off:lay.score_off + S.score_floats(L)] = torch.from_numpy(S.pack_native(c["native"], 0.0, L)).to(eng.device)
    with eng.with_domains(**FORCED):
        eng.set_option("score_native", 1)
        eng.set_option("score_domains", 1)
        try:
            rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 0, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
            assert rc == 0, eng.lib.dmp_last_error()
            eng.sync_check()
        finally:
            eng.set_option("score_domains", 0)
            eng.set_option("score_native", 0)
    h = buf.cpu().numpy()
    assert (h[lay.total:] == 7.0).all() and bool(torch.isnan(coords[15 * L:]).all()), "a guard float was written"
    assert np.array_equal(_bits(lay.domain_score_block(h)), _bits(c["got"]["ds"]))
    assert np.array_equal(_bits(lay.domains_block(h)), _bits(c["got"]["dom"]))


# ------------------------------------------------------------------------------------------------ 6. software-latched flag
def test_latched_flag_gives_nan_in_the_whole_block(eng):
    """A residue code of 22 raises the device-side flag DMP_FAULT_BAD_CODE (a software flag, not a GPU fault): the whole block
    is NaN, the inputs are untouched, the guard stays, and the next prediction on the engine is whole again."""
    from dmpfold2_amd.predict import FAULT_BAD_CODE
    L = 65
    c = _multi(eng, L)
    aln = c["aln"].copy()
    aln[0, 5] = 22
    lay = S.Layout(L, score=True, domains=True, score_domains=True)
    inputs = S.pack_native(c["native"], 40.0, L)[:3 * L + 1]
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.zeros((L, 5, 3), dtype=torch.float32, device=eng.device)
    buf = torch.zeros((lay.total + GUARD,), dtype=torch.float32, device=eng.device)
    buf[lay.total:] = 7.0
    buf[lay.score_off:lay.score_off + 3 * L + 1] = torch.from_numpy(inputs).to(eng.device)
    with eng.with_domains(**FORCED):
        eng.set_option("score_native", 1)
        eng.set_option("score_domains", 1)
        try:
            rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 1, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
            assert rc == 0
            assert eng.sync_faults() == FAULT_BAD_CODE
        finally:
            eng.set_option("score_domains", 0)
            eng.set_option("score_native", 0)
    h = buf.cpu().numpy()
    assert np.isnan(lay.domain_score_block(h)).all() and np.isnan(lay.domains_block(h)).all()
    assert np.array_equal(h[lay.score_off:lay.score_off + 3 * L + 1], inputs, equal_nan=True), "the inputs were touched"
    assert (h[lay.total:] == 7.0).all(), "the NaN fill went past the block"
    un = S.unpack_domain_scores(lay.domain_score_block(h), L)
    assert un["domains"] == 0 and un["legs"] == []
    again = _scored(eng, c["aln"], c["native"], params=FORCED)
    assert np.array_equal(_bits(again["ds"]), _bits(c["got"]["ds"]))


# ------------------------------------------------------------------------------------------------ 7. option values
def test_option_values(eng):
    """0 and 1 alone; a prediction begun with the option on and "domains" or "score_native" off fails with DMP_ERR_ARG and names
    the missing option (the raw call: Engine.predict turns "domains" on itself and asks for a native first)."""
    from dmpfold2_amd import _lib
    for bad in (-1, 2, 3):
        with pytest.raises(_lib.DmpError, match="score_domains must be 0 or 1"):
            eng.set_option("score_domains", bad)
    assert eng.get_option("score_domains") == 0
    L = 16
    aln = _one_row(L)
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.zeros((L, 5, 3), dtype=torch.float32, device=eng.device)
    buf = torch.zeros((S.Layout(L, score=True, domains=True, score_domains=True).total,), dtype=torch.float32, device=eng.device)
    mib = eng.get_option("device_mib")
    eng.set_option("score_domains", 1)
    try:
        assert eng.get_option("score_domains") == 1 and eng.get_option("device_mib") >= mib
        for on, missing in ((("score_native",), "domains"), (("domains",), "score_native"), ((), "domains")):
            for name in on:
                eng.set_option(name, 1)
            try:
                rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 0, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
                message = eng.lib.dmp_last_error().decode()
                assert rc == -1 and message.startswith("score_domains") and f"option {missing}, which is 0" in message, (on, rc, message)
            finally:
                for name in on:
                    eng.set_option(name, 0)
    finally:
        eng.set_option("score_domains", 0)
    with eng.with_score_domains():
        with pytest.raises(ValueError, match="score_domains scores every domain against a native structure"):
            eng.predict(aln, None, 0, 0)
    assert [eng.get_option(k) for k in ("score_domains", "domains", "score_native")] == [0, 0, 0]
    out = eng.predict(aln, None, 0, 0)                                 # the engine is whole afterwards
    eng.sync_check()
    assert len(out) == 2 and eng.domain_scores is None and eng.domain_score_block is None


def test_one_domain_of_more_than_256_rows(eng):
    """The default parse keeps the 257 residues whole: one domain whose rows outnumber a workgroup's threads, 1 + 5 x 257 seeds
    on the flat grid."""
    L = 257
    aln, coords0, confs0, model = _plain(eng, L)
    native = DR.moved_by_domain(model, np.zeros(L, dtype=np.int64), noise=NOISE, seed=5)
    got = _scored(eng, aln, native)
    assert got["dom"][0] == 1 and got["dom"][16] == 1, "the default parse keeps both whole"
    for leg in range(2):
        _row_equals_masked_call(got["ds"], got["score"], L, leg, 0, np.zeros(L, dtype=np.int64), f"L=257 whole, leg {leg}")
    assert got["ds"][16 + 25] == DR.near_pairs(native) and got["ds"][16 + 27] == 0


# ------------------------------------------------------------------------------------------------ 8. pipeline and front ends
def test_pipeline_gives_the_engines_blocks(eng, synth_sd):
    from dmpfold2_amd.predict import Pipeline
    dev = torch.device("cuda:0")
    pipe = Pipeline(dev, MAX_L, 4, _tensors(synth_sd), streams=2, precision=2)
    try:
        with pytest.raises(RuntimeError, match="set_score"):
            pipe.use_score_domains(True)
        pipe.set_score(True)
        pipe.use_domains(True, **FORCED)
        pipe.use_score_domains(True)
        assert all(e.get_option("score_domains") == 1 and e.get_option("domains") == 1 for e in pipe.engines)
        cases = [_multi(eng, L) for L in (17, 65)]
        tickets = [pipe.submit(torch.from_numpy(c["aln"]).to(dev), 0, 0, native=(c["native"], 0.0)) for c in cases]
        kept = {t: pipe.outputs_of(t) for t in tickets}
        got = pipe.collect(tickets)
        for t, c in zip(tickets, cases):
            assert not isinstance(got[t], Exception), got[t]
            assert len(got[t]) == 4, "coords, confs, the score block, the domain block: the new block is never handed out"
            assert np.array_equal(_bits(kept[t].domain_score_block), _bits(c["got"]["ds"]))
            assert np.array_equal(_bits(pipe.collected[t].domain_score_block), _bits(c["got"]["ds"]))
            assert np.array_equal(_bits(got[t][3]), _bits(c["got"]["dom"])) and np.array_equal(_bits(got[t][2]), _bits(c["got"]["score"]))
        pipe.use_score_domains(False)
        assert all(e.get_option("score_domains") == 0 and e.get_option("domains") == 1 for e in pipe.engines)
    finally:
        pipe.close()


def _write_pdb(path, seq, ca, chain="A"):
    three = dict(zip(S.AA1, S.AA3))
    with open(path, "w") as fh:
        for k, (aa, xyz) in enumerate(zip(seq, ca)):
            fh.write("ATOM  %5d  CA  %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n"
                     % (k + 1, three[aa], chain, k + 1, xyz[0], xyz[1], xyz[2]))
        fh.write("TER\nEND\n")


def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --native --score-domains`: stdout byte for byte the plain run's, the JSON line of --native gains "domain_scores";
    `dmpfold-batch --natives --score-domains`: <stem>.scores.json carries the same key, npz the two arrays, the summary the
    per-target figures."""
    import contextlib
    import io
    import json
    import dmpfold2_amd.predict as P
    from conftest import load_golden, golden_rows
    from dmpfold2_amd import aln_to_coords, run_dmpfold
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        rows = golden_rows(load_golden("pf10963_n3_m0"))
        p = tmp_path / "pf.aln"
        p.write_text("\n".join(rows) + "\n")
        plain = aln_to_coords(str(p), device="cuda:0", iterations=1, minsteps=0, weights_file=weights_file)
        L = plain[0].shape[0]
        model = plain[0][:, 1].cpu().numpy()
        parse = R.parse(model, **FORCED_REF)
        D = parse["header"][0]
        natives = tmp_path / "natives"
        natives.mkdir()
        _write_pdb(str(natives / "pf.pdb"), rows[0], DR.moved_by_domain(model, parse["labels"], noise=NOISE, seed=9))
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file, "--native", str(natives / "pf.pdb"),
                "--domains", "--domains-tau", "1.0", "--domains-min-size", "8", "--domains-min-segment", "2"]
        texts, errs = [], []
        for extra in ([], ["--score-domains"], ["--score-domains", "--scores", str(tmp_path / "scores.json")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        first = [json.loads(line) for line in errs[0].strip().split("\n")]
        second = [json.loads(line) for line in errs[1].strip().split("\n")]
        assert "domain_scores" not in first[0] and first[1] == second[1], "the domains line"
        js = second[0].pop("domain_scores")
        assert second[0] == first[0], "the scores line but for its new key"
        assert json.loads((tmp_path / "scores.json").read_text())["domain_scores"] == js
        e = P._ENGINES[0]
        assert js == json.loads(json.dumps(S.domain_scores_json(e.domain_scores, e.domains)))
        assert js["domains"] == D >= 2 and js["present"] == L and [r["size"] for r in js["model"]["rows"]] == parse["table"][:, 0].tolist()
        assert js["model"]["rows"][D - 1]["segments"] == S._segments(parse["labels"], D - 1)
        assert js["model"]["tm_domains"] > first[0]["tm"]
        assert js["model"]["lddt_inter"] is None or js["model"]["lddt_intra"] > js["model"]["lddt_inter"]
        assert [e.get_option(k) for k in ("score_domains", "domains", "score_native")] == [0, 0, 0]
        with pytest.raises(SystemExit):
            with contextlib.redirect_stderr(io.StringIO()):
                run_dmpfold(["-i", str(p), "--score-domains"])
        common = ["-i", str(p), "-n", "1", "-m", "0", "-w", weights_file, "--streams", "2", "--natives", str(natives),
                  "--domains", "--domains-tau", "1.0", "--domains-min-size", "8", "--domains-min-segment", "2"]
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(common + ["-o", str(out_dir), "--format", fmt, "--score-domains"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            leg = "native" if "native" in js else "model"
            assert summary["targets"] == 1 and summary["domain_scored_targets"] == 1
            assert summary["domain_scores"]["pf"] == {"leg": leg, "domains": len(js[leg]["rows"]), "tm_domains": js[leg]["tm_domains"],
                                                      "lddt_inter": js[leg]["lddt_inter"]}
            assert summary["mean_domain_tm_domains"] == js[leg]["tm_domains"] == summary["median_domain_tm_domains"]
            if fmt == "pdb":
                assert (out_dir / "pf.pdb").read_text() == texts[0]
                assert json.loads((out_dir / "pf.scores.json").read_text())["domain_scores"] == js
            else:
                z = np.load(str(out_dir / "pf.npz"))
                assert z["dom_score_table"].shape == (2, 16, 32) and z["dom_score_res"].shape == (4, L) and z["dom_score_table"].dtype == np.float32
                assert np.array_equal(_bits(z["dom_score_table"]), _bits(e.domain_scores["table"]))
                assert np.array_equal(_bits(z["dom_score_res"]), _bits(e.domain_scores["res"]))
    finally:
        P._ENGINES.clear()
