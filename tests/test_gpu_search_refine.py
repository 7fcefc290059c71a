"""The library search in two stages on the GPU (option "search_refine"; include/dmpfold_hip.h): every entry screened by its best
gapless threading, the best R by that refined.

A refined entry must be, bit for bit, the entry of a run without the option (which tests/test_gpu_search.py holds to
"align_structure" and that to the float64 definition); a screened entry is compared with the screen's float64 yardstick
(tests/search_refine_ref.py) by the rule of test_align_cpu.compare_alignment: integers equal, floats within 1 float32 ulp.
One engine (max_L = 257, synthetic weights, precision 2), one-row alignments, 0 recycling passes and 0 minimiser steps, raw
blocks through the C ABI.  The library of 16 is made from the MODEL's trace, so which entries are related does not depend on
what the synthetic weights predict; whether the screen separates them from the others does, so that condition on the
inputs is checked from the yardstick wherever the yardstick runs.
"""
import contextlib
import io
import json
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_rows
from search_refine_ref import RELATED, input_condition, library_traces, screen_yardstick
from test_align_cpu import compare_alignment, indel_copy, moved, random_walk

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

GUARD = 4096
MAX_L = 257
K16 = 16
OPTS = ("emit_distmap", "score_native", "align_structure", "search_max_m", "search_chunk", "search_structures")


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
    return (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)).reshape(-1).view(np.uint32)


def _entry(sb, L, K, k):
    """Entry k's 24 + 2L out floats of a search block."""
    return np.concatenate([sb[2 * K + 24 * k:2 * K + 24 * (k + 1)], sb[26 * K + 2 * L * k:26 * K + 2 * L * (k + 1)]])


def _mark(sb, K):
    """Offset 21 of every entry's header."""
    return sb[2 * K + 20:26 * K:24]


def _tm(sb, K):
    return sb[2 * K + 2:26 * K:24]


def _raw(eng, aln, search_block, K, refine=None, emit=False, score_block=None, align_block=None, chunk=0, fill=float("nan")):
    """dmp_predict into a poisoned buffer with every block's inputs in place -> (coords, host buffer, n_other, B0, n_out, bits):
    n_other = what the other options take, the search block lies at [B0, n_out), the guard behind n_out.  `refine` None: the
    option "search_refine" is never touched."""
    L = aln.shape[1]
    m_rows = None if align_block is None else (len(align_block) - S.align_floats(L, 0)) // 3
    n_other = S.conf_floats(L, emit, score_block is not None, m_rows)
    b0, n_out = None, n_other
    if search_block is not None:
        b0 = S.search_offset(L, emit, score_block is not None, None if align_block is None else align_block[0], MAX_L)
        n_out = max(n_other, b0 + len(search_block))
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.full((15 * L + GUARD,), fill, dtype=torch.float32, device=eng.device)
    buf = torch.full((n_out + GUARD,), fill, dtype=torch.float32, device=eng.device)
    if score_block is not None:
        s0 = S.score_offset(L, emit)
        buf[s0:s0 + len(score_block)] = torch.from_numpy(score_block).to(eng.device)
    if align_block is not None:
        a0 = S.align_offset(L, emit, score_block is not None)
        buf[a0:a0 + len(align_block)] = torch.from_numpy(align_block).to(eng.device)
    if search_block is not None:
        buf[b0:b0 + len(search_block)] = torch.from_numpy(search_block).to(eng.device)
    values = (int(emit), int(score_block is not None), int(align_block is not None), 0, chunk, K if search_block is not None else 0)
    try:
        for k, v in zip(OPTS, values):
            eng.set_option(k, v)
        if refine is not None:
            eng.set_option("search_refine", refine)
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), aln.shape[0], L, None, 0, 0, 0, coords.data_ptr(), buf.data_ptr(),
                                 eng.stream())
        assert rc == 0, eng.lib.dmp_last_error()
        bits = eng.sync_faults()
    finally:
        if refine is not None:
            eng.set_option("search_refine", 0)
        for k in reversed(OPTS):
            eng.set_option(k, 0)
    return coords, buf.cpu().numpy(), n_other, b0, n_out, bits


def _search(eng, aln, packed, K, refine=None, chunk=0):
    """The search block of one run, after the checks every run must pass: no fault, the guard untouched, the inputs kept."""
    L = aln.shape[1]
    _, h, n_other, b0, n_out, bits = _raw(eng, aln, packed, K, refine=refine, chunk=chunk)
    assert bits == 0 and b0 == L == n_other
    assert np.isnan(h[n_out:]).all() and len(h) - n_out == GUARD, "a guard float was written"
    sb = h[b0:n_out]
    assert np.array_equal(_bits(sb[:K]), _bits(packed[:K])) and np.array_equal(_bits(sb[26 * K + 2 * L * K:]), _bits(packed[26 * K + 2 * L * K:]))
    return sb


_CASES = {}


def _case(eng, L):
    """Made once per length and left unchanged: the plain prediction, the library of 16 made from its trace, the block of a run
    that never set the option (`base`), the block with R = 4 (`four`), and - at the lengths the yardstick covers - the
    screen's yardstick of every entry."""
    if L not in _CASES:
        aln = _one_row(L)
        coords0, confs0 = eng.predict(aln, None, 0, 0)
        eng.sync_check()
        model = coords0[:, 1].cpu().numpy().copy()
        traces = library_traces(model, cap=MAX_L)
        lib = S.Library.from_traces(traces)
        packed = S.pack_library(lib, L)
        base = _search(eng, aln, packed, K16)                 # (on the parent commit as well: the option is never named)
        four = _search(eng, aln, packed, K16, refine=4)       # (on the parent commit: "unknown option")
        _CASES[L] = dict(aln=aln, coords=coords0.clone(), confs=confs0.clone(), model=model, lib=lib, packed=packed, base=base,
                         four=four, screen=[screen_yardstick(model, t) for t in traces] if L <= 64 else None)
    return _CASES[L]


def _check_mixed(sb, base, L, K, refined, tag):
    """A block whose `refined` entries are the base run's bit for bit, every other one screened; the ranks the host's."""
    marks = _mark(sb, K)
    assert sorted(np.nonzero(marks == 0)[0].tolist()) == sorted(refined), (tag, marks.tolist())
    for k in range(K):
        if k in refined:
            assert np.array_equal(_bits(_entry(sb, L, K, k)), _bits(_entry(base, L, K, k))), (tag, k)
        else:
            assert marks[k] == 1.0 and (_entry(sb, L, K, k)[21:24] == 0).all(), (tag, k, marks[k])
    assert sb[K:2 * K].tolist() == [float(k) for k in S.host_rank(_tm(sb, K))], tag


# ------------------------------------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("L", [8, 33, 64, 257])
def test_off_is_off(eng, L):
    """"search_refine" 0, K and K + 1: the block of a run that never set the option, bit for bit.  (On the parent commit the
    first set_option raises "unknown option": the test that fails without the feature.)"""
    c = _case(eng, L)
    assert not np.isnan(c["base"][2 * K16:26 * K16]).any() and (_mark(c["base"], K16) == 0).all()
    for refine in (0, K16, K16 + 1):
        sb = _search(eng, c["aln"], c["packed"], K16, refine=refine)
        assert np.array_equal(_bits(sb), _bits(c["base"])), (L, refine)
    assert eng.get_option("search_refine") == 0


# ------------------------------------------------------------------------------------------------ 2. R = 4 of K = 16
@pytest.mark.parametrize("L", [8, 33, 64, 257])
def test_four_of_sixteen(eng, L):
    c = _case(eng, L)
    sb, lib = c["four"], c["lib"]
    tm = _tm(sb, K16)
    print(f"search_refine L={L}: offset 21", _mark(sb, K16).astype(int).tolist(), "tm_model", np.round(tm, 4).tolist(), file=sys.stderr)
    chosen = list(RELATED)
    if c["screen"] is not None:
        # the condition on the inputs: the related entries are the four best by the screen, 0.05 above the rest
        want_tm, margins, problems = input_condition(c["model"], [lib.entry(k) for k in range(K16)], screened=c["screen"])
        print(f"search_refine L={L}: yardstick's screened tm_model", np.round(want_tm, 4).tolist(), file=sys.stderr)
        if L >= 33:
            assert not problems, ("choose another library", problems)
        else:
            # at d0 = 0.5 (L = 8, here for the smallest slots) a noisy copy of eight residues screens no better than a walk:
            # the entries chosen must be the four best by the yardstick's screen, whichever they are, the fourth further
            # from the fifth than float32 can blur (1 ulp of a tm_model is 6e-8)
            order = S.host_rank(want_tm)
            assert want_tm[order[3]] - want_tm[order[4]] >= 1e-5, "choose another library"
            chosen = sorted(order[:4].tolist())
    _check_mixed(sb, c["base"], L, K16, chosen, f"L={L} R=4")
    assert np.isfinite(tm).all() and (tm[chosen].min() > np.delete(tm, chosen)).all()
    if c["screen"] is not None:
        hits = S.unpack_search(sb, L, lib.lengths, refine=4)
        assert hits["refined"].tolist() == [k in chosen for k in range(K16)]
        worst = {}
        for k in range(K16):
            if k not in chosen:
                want, margin = c["screen"][k]
                seen = compare_alignment(hits["hits"][k], want, margin, f"L={L} screened entry {k}")
                worst = {name: max(worst.get(name, 0.0), v) for name, v in seen.items()}
        print(f"search_refine L={L}: screened entries, largest differences in float32 ulps:", worst, file=sys.stderr)


# ------------------------------------------------------------------------------------------------ 3. R does not move a screened entry
def test_screened_bits_do_not_depend_on_R(eng):
    L = 33
    c = _case(eng, L)
    one = _search(eng, c["aln"], c["packed"], K16, refine=1)
    most = _search(eng, c["aln"], c["packed"], K16, refine=15)
    assert int((_mark(one, K16) == 1).sum()) == 15 and int((_mark(most, K16) == 1).sum()) == 1
    assert _mark(one, K16)[0] == 0, "the rigid copy is the best by the screen"
    for other in (most, c["four"]):
        both = [k for k in range(K16) if _mark(one, K16)[k] == 1 and _mark(other, K16)[k] == 1]
        assert both
        for k in both:
            assert np.array_equal(_bits(_entry(one, L, K16, k)), _bits(_entry(other, L, K16, k))), k
    for k in np.nonzero(_mark(most, K16) == 0)[0]:
        assert np.array_equal(_bits(_entry(most, L, K16, k)), _bits(_entry(c["base"], L, K16, k))), k


# ------------------------------------------------------------------------------------------------ 4. chunks
def test_chunk_boundaries_change_nothing(eng):
    """R = 5 of 16 with 1 and 3 entries per chunk: both passes cross chunk boundaries (the fifth entry chosen is an unrelated
    walk somewhere behind the related four)."""
    L = 33
    c = _case(eng, L)
    whole = _search(eng, c["aln"], c["packed"], K16, refine=5)
    assert eng.get_option("search_chunk_used") >= K16
    chosen = np.nonzero(_mark(whole, K16) == 0)[0].tolist()
    assert len(chosen) == 5 and chosen[:4] == list(RELATED) and chosen[4] > 4
    for chunk in (1, 3):
        sb = _search(eng, c["aln"], c["packed"], K16, refine=5, chunk=chunk)
        assert eng.get_option("search_chunk_used") == chunk
        assert np.array_equal(_bits(sb), _bits(whole)), chunk


# ------------------------------------------------------------------------------------------------ 5. ties
def test_a_tie_at_the_boundary_goes_to_the_lower_index(eng):
    L = 33
    c = _case(eng, L)
    lib = S.Library.from_traces([c["lib"].entry(k) for k in (5, 1, 7, 1)])
    packed = S.pack_library(lib, L)
    base = _search(eng, c["aln"], packed, 4)
    sb = _search(eng, c["aln"], packed, 4, refine=1)
    _check_mixed(sb, base, L, 4, (1,), "tie")
    for k, src in ((0, 5), (2, 7), (3, 1)):
        want, margin = c["screen"][src]
        compare_alignment(S.unpack_search(sb, L, lib.lengths)["hits"][k], want, margin, f"tie: entry {k}")
    both = _search(eng, c["aln"], packed, 4, refine=2)
    _check_mixed(both, base, L, 4, (1, 3), "tie, R = 2")
    assert np.array_equal(_bits(_entry(both, L, 4, 1)), _bits(_entry(both, L, 4, 3)))


# ------------------------------------------------------------------------------------------------ 6. spoiled entries, short supply
def test_spoiled_entries_and_short_supply(eng):
    L = 33
    c = _case(eng, L)
    lib = c["lib"]
    packed = c["packed"].copy()
    spoiled = (1, 6)
    for k in spoiled:
        packed[26 * K16 + 2 * L * K16 + 3 * int(lib.lengths[:k].sum()) + 3 * 4 + 1] = np.nan
    valid = [k for k in range(K16) if k not in spoiled]
    base = _search(eng, c["aln"], packed, K16)
    for k in range(K16):
        assert np.array_equal(_bits(_entry(base, L, K16, k)), _bits(_entry(c["base"], L, K16, k))) != (k in spoiled), k
    # R up to the number of valid entries: the spoiled ones are never chosen
    four = _search(eng, c["aln"], packed, K16, refine=4)
    chosen = np.nonzero(_mark(four, K16) == 0)[0].tolist()
    assert len(chosen) == 4 and chosen[:3] == [0, 2, 3] and chosen[3] not in spoiled
    for k in range(K16):
        e = _entry(four, L, K16, k)
        if k in spoiled:
            assert np.isnan(e).all(), k
        else:
            same = c["base"] if k in chosen else c["four"]
            assert np.array_equal(_bits(e), _bits(_entry(same, L, K16, k))), k
    assert four[K16:2 * K16].tolist() == [float(k) for k in S.host_rank(_tm(four, K16))] and four[2 * K16 - 2:2 * K16].tolist() == [1.0, 6.0]
    all_valid = _search(eng, c["aln"], packed, K16, refine=14)
    assert np.array_equal(_bits(all_valid), _bits(base))
    # R above it: a spoiled entry is chosen, stays NaN, and the run ends clean
    short = _search(eng, c["aln"], packed, K16, refine=15)
    assert np.array_equal(_bits(short), _bits(base))
    # a bad m_k: today's all-NaN answer
    lengths = lib.lengths.astype(np.float32)
    lengths[3] = 2.0
    bad = S.pack_library(lib, L, lengths=lengths)
    sb = _search(eng, c["aln"], bad, K16, refine=4)
    assert np.isnan(sb[2 * K16:26 * K16 + 2 * L * K16]).all() and sb[K16:2 * K16].tolist() == [float(k) for k in range(K16)]


# ------------------------------------------------------------------------------------------------ 7. smallest
def test_one_of_two(eng):
    L = 33
    c = _case(eng, L)
    lib = S.Library.from_traces([c["lib"].entry(9), c["lib"].entry(0)])
    packed = S.pack_library(lib, L)
    base = _search(eng, c["aln"], packed, 2)
    sb = _search(eng, c["aln"], packed, 2, refine=1)
    _check_mixed(sb, base, L, 2, (1,), "K = 2")
    compare_alignment(S.unpack_search(sb, L, lib.lengths)["hits"][0], *c["screen"][9], "K = 2: entry 0")
    assert sb[2:4].tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------ 8. beside the other options
@pytest.mark.parametrize("align_m", ["valid", "zero"])
def test_beside_the_other_options(eng, align_m):
    L = 33
    c = _case(eng, L)
    native = random_walk(L, 21)
    native[::9] = np.nan
    sblock = S.pack_native(native, 0.0, L)
    if align_m == "valid":
        ablock = S.pack_structure(indel_copy(c["model"], 52, m=40)[0], L)
    else:
        ablock = S.pack_structure(random_walk(10, 6), L, m_value=0)
    c0, h0, n0, _, _, bits0 = _raw(eng, c["aln"], None, 0, emit=True, score_block=sblock, align_block=ablock)
    c1, h1, n1, b0, n_out, bits1 = _raw(eng, c["aln"], c["packed"], K16, refine=4, emit=True, score_block=sblock, align_block=ablock)
    assert bits0 == 0 and bits1 == 0 and n0 == n1
    a0 = S.align_offset(L, True, True)
    assert b0 == a0 + 25 + 2 * L + (3 * 40 if align_m == "valid" else 0)
    assert np.array_equal(_bits(c0), _bits(c1)) and np.array_equal(_bits(c1[:15 * L]), _bits(c["coords"]))
    assert np.array_equal(_bits(h0[:a0 + 25 + 2 * L]), _bits(h1[:a0 + 25 + 2 * L]))
    if align_m == "valid":
        assert np.array_equal(_bits(h0[:n0]), _bits(h1[:n0])) and not np.isnan(h1[a0 + 1:a0 + 21]).any()
    else:
        assert np.isnan(h1[a0 + 1:a0 + 25 + 2 * L]).all()
    assert np.array_equal(_bits(h1[b0:n_out]), _bits(c["four"]))
    assert np.isnan(h1[n_out:]).all() and np.isnan(h0[n0:]).all(), "a guard float was written"


# ------------------------------------------------------------------------------------------------ 9. capacity
def test_capacity_L2048(synth_sd):
    """The only place the screen kernel's 50 KB of dynamic LDS is reached: a rigid copy (refined) and a walk of 2048 rows
    (screened)."""
    from dmpfold2_amd.predict import Engine
    L = 2048
    e = Engine("cuda:0", L, 1)
    try:
        e.set_weights(_tensors(synth_sd))
        e.set_option("precision", 2)
        aln = _one_row(L)
        coords0, _ = e.predict(aln, None, 0, 0)
        e.sync_check()
        model = coords0[:, 1].cpu().numpy()
        lib = S.Library.from_traces([random_walk(L, 77), moved(model, 9)[2]])
        lib.refine = 1
        coords, _ = e.predict(aln, None, 0, 0, library=lib)
        e.sync_check()
        assert torch.equal(coords, coords0) and e.get_option("search_refine") == 0
        hits = e.hits
        assert sorted(hits) == ["hits", "names", "rank", "refine", "refined"] and hits["refine"] == 1
        walk, copy = hits["hits"]
        print("search_refine L=2048: walk (screened) tm_model", walk["tm_model"], "n_ali", walk["n_ali"], "copy (refined) tm_model",
              copy["tm_model"], file=sys.stderr)
        assert hits["refined"].tolist() == [False, True] and hits["rank"].tolist() == [1, 0]
        assert copy["tm_model"] >= 1.0 - 1e-6 and copy["n_ali"] == L and np.array_equal(copy["ali"], np.arange(L))
        assert 0.0 < walk["tm_model"] < 0.5 and walk["n_ali"] >= L // 2
        ali = walk["ali"][walk["ali"] >= 0]
        assert len(ali) == walk["n_ali"] and (np.diff(ali) == 1).all(), "a screened alignment is gapless"
        assert (walk["ali"] >= 0).sum() == np.isfinite(walk["deviation"]).sum()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 10. pipeline, front ends, values
def test_pipeline(synth_sd):
    from dmpfold2_amd.predict import Engine, Pipeline
    dev = torch.device("cuda:0")
    sdt = _tensors(synth_sd)
    single = Engine(dev, 64, 1)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 64, 1, sdt, streams=2, precision=2)
    try:
        alns = [_one_row(L) for L in (33, 48)]
        first, _ = single.predict(alns[0], None, 1, 0)
        single.sync_check()
        model = first[:, 1].cpu().numpy()
        lib = S.Library.from_traces(library_traces(model, cap=64))
        plain, refs = [], []
        for aln in alns:
            single.predict(aln, None, 1, 0, library=lib)
            single.sync_check()
            plain.append(single.search_block.clone())
        lib.refine = 4
        for aln in alns:
            cc, ff = single.predict(aln, None, 1, 0, library=lib)
            single.sync_check()
            assert single.get_option("search_refine") == 0
            refs.append((cc.clone(), ff.clone(), single.search_block.clone()))
        assert int((_mark(refs[0][2].cpu().numpy(), K16) == 0).sum()) == 4
        assert not np.array_equal(_bits(refs[0][2]), _bits(plain[0]))
        pipe.set_search(lib)
        assert all(e.get_option("search_refine") == 4 and e.get_option("search_structures") == K16 for e in pipe.engines)
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), 1, 0) for a in alns]
        res = pipe.collect(tickets)
        for t, ref in zip(tickets, refs):
            assert not isinstance(res[t], Exception), res[t]
            coords, confs, block = res[t]
            assert torch.equal(coords, ref[0]) and torch.equal(confs, ref[1]) and np.array_equal(_bits(block), _bits(ref[2]))
        lib.refine = 0
        pipe.set_search(lib)
        assert all(e.get_option("search_refine") == 0 for e in pipe.engines)
        out = pipe.run([torch.from_numpy(alns[1]).to(dev)], 1, 0)
        pipe.sync_check()
        assert np.array_equal(_bits(out[0][2]), _bits(plain[1]))
        lib.refine = 4
        pipe.set_search(lib)
        pipe.set_search(None)
        assert all(e.get_option("search_refine") == 0 and e.get_option("search_structures") == 0 for e in pipe.engines)
    finally:
        pipe.close()
        single.close()


def test_option_values(eng):
    from dmpfold2_amd import _lib
    for bad in (-1, 4097):
        with pytest.raises(_lib.DmpError, match=f"search_refine must be 0 or 1 .. 4096, got {bad}"):
            eng.set_option("search_refine", bad)
    assert eng.get_option("search_refine") == 0
    for value in (1, 4096, 0):
        eng.set_option("search_refine", value)
        assert eng.get_option("search_refine") == value
    assert eng.lib.dmp_abi_version() == 5


def _write_pdb(path, ca, chain="A"):
    with open(path, "w") as fh:
        for k, xyz in enumerate(ca):
            fh.write("ATOM  %5d  CA  %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n"
                     % (k + 1, S.AA3[k % 20], chain, k + 1, xyz[0], xyz[1], xyz[2]))
        fh.write("TER\nEND\n")


def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --search DIR --search-refine 1` and `dmpfold-batch --library FILE.npz --search-refine 1`: stdout byte for byte
    the run's without the search, the JSON with "refine" and "refined", the rigid copy refined and equal to the full search's."""
    import dmpfold2_amd.predict as P
    from dmpfold2_amd import aln_to_coords, run_dmpfold
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        p = tmp_path / "pf.aln"
        p.write_text("\n".join(golden_rows(load_golden("pf10963_n3_m0"))) + "\n")
        kw = dict(device="cuda:0", iterations=1, minsteps=0, weights_file=weights_file)
        plain = aln_to_coords(str(p), **kw)
        L = plain[0].shape[0]
        model = plain[0][:, 1].cpu().numpy()
        folds = tmp_path / "folds"
        folds.mkdir()
        _write_pdb(str(folds / "b_copy.pdb"), moved(model, 5)[2])
        _write_pdb(str(folds / "a_walk.pdb"), random_walk(L + 11, 1))
        _write_pdb(str(folds / "c_walk.pdb"), random_walk(25, 2))
        S.Library.from_dir(str(folds)).save(str(tmp_path / "folds.npz"))
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file]
        texts, lines = [], []
        for extra in ([], ["--search", str(folds), "--search-top", "3"],
                      ["--search", str(tmp_path / "folds.npz"), "--search-top", "3", "--search-refine", "1"]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            lines.append(json.loads(err.getvalue().strip().split("\n")[-1]) if extra else None)
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        full, got = lines[1], lines[2]
        assert list(full) == ["entries", "hits"] and all("refined" not in h for h in full["hits"])
        assert list(got) == ["entries", "refine", "hits"] and got["refine"] == 1 and got["entries"] == 3
        assert [(h["name"], h["refined"]) for h in got["hits"]][0] == ("b_copy", True)
        assert sorted((h["name"], h["refined"]) for h in got["hits"]) == [("a_walk", False), ("b_copy", True), ("c_walk", False)]
        assert {k: v for k, v in got["hits"][0].items() if k != "refined"} == full["hits"][0]
        assert P._ENGINES[0].get_option("search_refine") == 0
        brief = [{k: v for k, v in h.items() if k not in ("R", "t")} for h in got["hits"]]
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--library", str(tmp_path / "folds.npz"), "--search-top", "3",
                                 "--search-refine", "1"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 1 and summary["searched_targets"] == 1 and summary["hits"] == {"pf": brief}
            if fmt == "pdb":
                assert (out_dir / "pf.pdb").read_text() == texts[0]
                assert json.loads((out_dir / "pf.hits.json").read_text()) == got
            else:
                z = np.load(str(out_dir / "pf.npz"))
                assert z["hit_refined"].dtype == np.bool_ and z["hit_refined"].tolist() == [False, True, False]
                assert z["hit_rank"].tolist()[0] == 1
        out_dir = tmp_path / "out_plain"
        with contextlib.redirect_stdout(io.StringIO()):
            assert batch.main(["-i", str(p), "-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", "npz",
                               "--streams", "2", "--library", str(tmp_path / "folds.npz")]) == 0
        assert "hit_refined" not in np.load(str(out_dir / "pf.npz")).files
    finally:
        P._ENGINES.clear()
