"""The fold library searched with every domain of the model on the GPU (option "search_domains"; include/dmpfold_hip.h).

Pair (d, k) is defined as what "align_structure" gives for the domain's gathered trace and entry k.  Two yardsticks: where the
model is one domain, the whole-model search of the same call, bit for bit (1); where it has several, the float64 definition
restated in tests/search_domains_ref.py, by the 1 float32 ulp rule of test_align_cpu.compare_alignment with ali, n_ali and the
seed exact (2).  One engine (max_L = 257, synthetic weights, precision 2), one-row alignments, 0 recycling passes and 0
minimiser steps throughout.  On the parent commit the option is unknown and every test here fails."""
import contextlib
import io
import json
import sys

import numpy as np
import pytest
import torch

import domains_ref as R
import search_domains_ref as SR
from conftest import load_golden, golden_rows
from test_align_cpu import compare_alignment, indel_copy, moved, random_walk
from test_gpu_search import _library_for

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

MAX_L = 257
GUARD = 4096
DEFAULTS = dict(tau=0.25, min_size=40, min_segment=10)
FORCED = dict(tau=1.0, min_size=8, min_segment=2)            # every admissible cut is accepted
FORCED_REF = dict(tau_milli=1000, min_size=8, min_segment=2)
MULTI = (17, 65, 257)                                        # of the LENGTHS sweep of tests/test_gpu_domains.py


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


def _search(eng, aln, lib, mode=1, params=DEFAULTS, chunk=0, refine=0):
    """One prediction with the library searched - with `mode` also by every domain - -> dict of host copies.  Every option is
    as it was afterwards."""
    lib.domains, lib.refine = bool(mode), refine
    try:
        if mode == 2:
            eng.set_option("search_domains", 2)
        eng.set_option("search_chunk", chunk)
        with eng.with_domains(**params):
            coords, confs = eng.predict(aln, None, 0, 0, library=lib)
            eng.sync_check()
    finally:
        eng.set_option("search_chunk", 0)
        eng.set_option("search_domains", 0)
        lib.domains, lib.refine = False, 0
    assert [eng.get_option(k) for k in ("search_domains", "domains", "search_structures", "search_refine")] == [0, 0, 0, 0]
    ds = eng.domain_search_block
    return dict(coords=coords.clone(), confs=confs.clone(), dom=eng.domains_block.cpu().numpy().copy(),
                search=eng.search_block.cpu().numpy().copy(), ds=None if ds is None else ds.cpu().numpy().copy(),
                hits=eng.domain_hits if mode else None)


def _parts(ds, L, K):
    """rank (16, K), headers (16, K, 24), res (K, 2, L) of a domain-search block, as views."""
    r = 16 * K
    return ds[:r].reshape(16, K), ds[r:25 * r].reshape(16, K, 24), ds[25 * r:].reshape(K, 2, L)


def _pair_floats(ds, L, K, d, k, idx):
    """Pair (d, k)'s 24 header floats, then ali and deviation of the domain's residues."""
    _, headers, res = _parts(ds, L, K)
    return np.concatenate([headers[d, k], res[k, 0, idx], res[k, 1, idx]])


# ------------------------------------------------------------------------------------------------ 1. one domain: the whole search
@pytest.mark.parametrize("L", [16, 65, 257])
def test_gather_path_equals_the_whole_search(eng, L):
    aln, coords0, confs0, model = _plain(eng, L)
    lib, K = _library_for(model), 7
    whole = _search(eng, aln, lib, mode=0)
    assert whole["ds"] is None and whole["dom"][0] == 1.0, "the default parse keeps this model whole"
    sb = whole["search"]
    gathered = _search(eng, aln, lib, mode=2)
    copied = _search(eng, aln, lib, mode=1)
    for tag, got in (("gather", gathered), ("copy", copied)):
        assert got["dom"][0] == 1.0 and got["ds"].shape == (S.domain_search_floats(L, K),), tag
        rank, headers, res = _parts(got["ds"], L, K)
        assert np.array_equal(_bits(rank[0]), _bits(sb[K:2 * K])), tag
        assert np.array_equal(_bits(headers[0]), _bits(sb[2 * K:26 * K])), (tag, np.flatnonzero(_bits(headers[0]) != _bits(sb[2 * K:26 * K]))[:8])
        assert np.array_equal(_bits(res), _bits(sb[26 * K:26 * K + 2 * L * K])), tag
        assert np.isnan(rank[1:]).all() and np.isnan(headers[1:]).all(), tag
        assert not np.isnan(headers[0, :, :20]).any(), tag
        for name in ("dom", "search"):
            assert np.array_equal(_bits(got[name]), _bits(whole[name])), (tag, name)
        assert torch.equal(got["coords"], coords0) and torch.equal(got["confs"], confs0), tag
    assert np.array_equal(_bits(gathered["ds"]), _bits(copied["ds"]))
    hits = copied["hits"]
    assert hits["domains"] == 1 and hits["names"] == lib.names and hits["rank"][0].tolist() == sb[K:2 * K].astype(int).tolist()


# ------------------------------------------------------------------------------------------------ 2. several domains: the definition
_MULTI = {}


def _domain_library(model, parse, L):
    """Per domain an indel copy of its gathered trace (two foreign rows inserted, noise, moved); a rigid copy of the first
    domain of several segments; an unrelated walk; a 3-row entry; an entry of m = 257; entry 0 once more (equal values for
    the ranking) -> (score.Library, the domain that has the rigid copy)."""
    labels, D = parse["labels"], parse["header"][0]
    traces, names = [], []
    for d in range(D):
        own = SR.gather(model, labels, d)
        traces.append(indel_copy(own, 4000 + 16 * L + d, m=len(own) + 2, noise=0.15)[0])
        names.append(f"copy{d}")
    split = [d for d in range(D) if parse["table"][d, 1] > 1]
    rigid_of = split[0] if split else 0
    traces += [moved(SR.gather(model, labels, rigid_of), 9)[2], random_walk(41, 50 + L), random_walk(3, 60 + L),
               random_walk(MAX_L, 70 + L), traces[0].copy()]
    names += ["rigid", "walk41", "tiny", "walk257", "copy0_again"]
    return S.Library.from_traces(traces, names), rigid_of


def _multi(eng, L):
    """Made once per length and left unchanged: the forced parse of the plain prediction (tests/domains_ref.py), the library
    built from its domains, the search with every domain."""
    if L not in _MULTI:
        aln, coords0, confs0, model = _plain(eng, L)
        parse = R.parse(model, **FORCED_REF)
        labels, D = parse["labels"], parse["header"][0]
        lib, rigid_of = _domain_library(model, parse, L)
        got = _search(eng, aln, lib, mode=1, params=FORCED)
        _MULTI[L] = dict(aln=aln, model=model, parse=parse, labels=labels, D=D, lib=lib, rigid_of=rigid_of, got=got)
    return _MULTI[L]


@pytest.mark.parametrize("L", MULTI)
def test_every_domain_against_the_definition(eng, L):
    c = _multi(eng, L)
    lib, labels, D, got, K = c["lib"], c["labels"], c["D"], c["got"], len(c["lib"])
    assert got["dom"][0] == D and np.array_equal(got["dom"][32:32 + L], labels.astype(np.float32)), "the library's parse is the restatement's"
    ds = got["hits"]
    assert ds["domains"] == D and np.isnan(ds["rank_raw"][D:]).all() and np.isnan(ds["headers"][D:]).all()
    assert not np.isnan(ds["headers"][:D, :, :20]).any()
    walk = lib.names.index("walk41")
    pairs = [(d, d) for d in range(D)] + [(c["rigid_of"], lib.names.index("rigid")), (0, walk)] + ([(1, 0)] if D > 1 else [])
    for d, k in pairs:
        want, margin, idx = SR.pair(c["model"], labels, d, lib.entry(k))
        seen = compare_alignment(SR.hit_of(ds, d, k, labels), want, margin, f"L={L} domain {d} entry {lib.names[k]}")
        print(f"L={L} domain {d} (n={len(idx)}) entry {lib.names[k]}: tm_domain {want['tm_model']:.4f} margin {margin:.2e} ulps", seen, file=sys.stderr)
        assert SR.hit_of(ds, d, k, labels)["ali"].shape == (len(idx),)
    # every domain's best hit is a copy of itself: its own, or - for the one that has it - the rigid copy
    for d in range(D):
        best = lib.names[ds["rank"][d][0]]
        assert best == ("rigid" if d == c["rigid_of"] else f"copy{d}"), (d, best, [lib.names[k] for k in ds["rank"][d][:3]])
        if d == c["rigid_of"]:
            assert ds["hits"][d][lib.names.index("rigid")]["tm_model"] >= 1.0 - 1e-5
            assert lib.names[ds["rank"][d][1]] == f"copy{d}", "behind the rigid copy, the domain's own indel copy"
            idx = SR.residues(labels, d)
            assert ds["ali"][lib.names.index("rigid")][idx].tolist() == list(range(len(idx))), "the identity on the domain's residues"
    # entry 0 carries, for the residues of every other domain, that domain's own pair (checked above for domain 1); nothing is
    # left unwritten: a residue is aligned or -1, and its deviation is NaN exactly where it is -1
    _, _, res = _parts(got["ds"], L, K)
    assert not np.isnan(res[:, 0]).any() and np.array_equal(np.isnan(res[:, 1]), res[:, 0] == -1.0)


def test_the_sweep_met_every_path(eng):
    """So that a change of weights cannot hollow case 2 out: sixteen domains, a domain of several segments, a domain of
    exactly min_size = 8 residues, and grids sized for more domains than there are (Dmax > D)."""
    cases = [_multi(eng, L) for L in MULTI]
    tables = [c["parse"]["table"] for c in cases]
    print("domains:", {L: c["D"] for L, c in zip(MULTI, cases)}, "sizes:", [t[:, 0].tolist() for t in tables], file=sys.stderr)
    assert any(c["D"] == 16 for c in cases)
    assert any((t[:, 1] > 1).any() for t in tables)
    assert any((t[:, 0] == 8).any() for t in tables)
    assert any(max(1, min(16, L // 8)) > c["D"] for L, c in zip(MULTI, cases))
    assert all(c["D"] >= 2 for c in cases)


# ------------------------------------------------------------------------------------------------ 3. ranking
@pytest.mark.parametrize("L", MULTI)
def test_ranking(eng, L):
    c = _multi(eng, L)
    K, D = len(c["lib"]), c["D"]
    rank, headers, _ = _parts(c["got"]["ds"], L, K)
    for d in range(D):
        assert rank[d].tolist() == [float(k) for k in S.host_rank(headers[d, :, 2])], d
        # the duplicated entry: equal values, the lower index first and the other right behind it
        assert np.array_equal(_bits(headers[d, 0]), _bits(headers[d, K - 1])), d
        order = rank[d].tolist()
        assert order.index(float(K - 1)) == order.index(0.0) + 1, d
    assert np.isnan(rank[D:]).all()


# ------------------------------------------------------------------------------------------------ 4. search_refine
def test_refine_per_domain(eng):
    L, K = 65, 7
    aln, _, _, model = _plain(eng, L)
    lib = _library_for(model)
    labels = R.parse(model, **FORCED_REF)["labels"]
    D = int(labels.max()) + 1
    assert D >= 2
    full = _search(eng, aln, lib, mode=1, params=FORCED)["ds"]
    runs = {Rn: _search(eng, aln, lib, mode=1, params=FORCED, refine=Rn)["ds"] for Rn in (1, 2, 5, 7, 0)}
    assert np.array_equal(_bits(runs[7]), _bits(full)) and np.array_equal(_bits(runs[0]), _bits(full))
    for Rn in (2, 5):
        _, headers, _ = _parts(runs[Rn], L, K)
        for d in range(D):
            idx = SR.residues(labels, d)
            refined = [k for k in range(K) if headers[d, k, 20] == 0.0]
            screened = [k for k in range(K) if headers[d, k, 20] == 1.0]
            assert len(refined) == Rn and len(screened) == K - Rn, (Rn, d, headers[d, :, 20].tolist())
            for k in refined:
                assert np.array_equal(_bits(_pair_floats(runs[Rn], L, K, d, k, idx)), _bits(_pair_floats(full, L, K, d, k, idx))), (Rn, d, k)
            for k in screened:
                assert np.array_equal(_bits(_pair_floats(runs[Rn], L, K, d, k, idx)), _bits(_pair_floats(runs[1], L, K, d, k, idx))), (Rn, d, k)
            # the R refined are the R that screen best for this domain: R = 1's run holds every screened value but its one winner's
            rank, _, _ = _parts(runs[Rn], L, K)
            assert rank[d].tolist() == [float(k) for k in S.host_rank(headers[d, :, 2])]
    un = S.unpack_domain_search(runs[2], L, K, refine=2)
    assert un["refined"].shape == (D, K) and (un["refined"].sum(1) == 2).all()


# ------------------------------------------------------------------------------------------------ 5. chunks
def test_chunk_boundaries_change_nothing(eng):
    L = 65
    aln, _, _, model = _plain(eng, L)
    lib = _library_for(model)
    for refine in (0, 2):
        want = _search(eng, aln, lib, mode=1, params=FORCED, refine=refine)["ds"]
        for chunk in (1, 3):                                 # 3 does not divide K = 7 (nor R = 2): chunks straddle domains
            got = _search(eng, aln, lib, mode=1, params=FORCED, chunk=chunk, refine=refine)["ds"]
            assert np.array_equal(_bits(got), _bits(want)), (refine, chunk)


# ------------------------------------------------------------------------------------------------ 6. nothing else moves
def test_the_other_blocks_keep_their_bits(eng):
    for L in (65, 257):
        c = _multi(eng, L)
        aln, coords0, confs0, _ = _plain(eng, L)
        without = _search(eng, aln, c["lib"], mode=0, params=FORCED)
        got = c["got"]
        assert without["ds"] is None
        assert torch.equal(got["coords"], coords0) and torch.equal(got["confs"], confs0)
        assert torch.equal(without["coords"], coords0) and torch.equal(without["confs"], confs0)
        for name in ("dom", "search"):
            assert np.array_equal(_bits(got[name]), _bits(without[name])), (L, name)


def test_beside_every_other_block_engine_and_pipeline(synth_sd):
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, Pipeline
    L, N, ITERATIONS, MINSTEPS = 24, 4, 1, 5
    OTHERS = ("score_block", "align_block", "search_block", "map_score_block", "pass_block", "ss_block", "exposure_block", "domains_block")
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
        with eng.with_domains(**FORCED):
            without = [x.clone() for x in eng.predict(aln, None, ITERATIONS, MINSTEPS, **everything)]
            eng.sync_check()
            blocks = {name: getattr(eng, name).clone() for name in OTHERS}
            assert eng.domain_search_block is None and eng.domain_hits is None and blocks["domains_block"][0].item() >= 2.0
            library.domains = True
            full = [x.clone() for x in eng.predict(aln, None, ITERATIONS, MINSTEPS, **everything)]
            eng.sync_check()
            assert eng.get_option("search_domains") == 0 and eng.get_option("domains") == 1
        assert len(full) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(full, without))
        for name in OTHERS:
            assert np.array_equal(_bits(getattr(eng, name)), _bits(blocks[name])), name
        alone = eng.domain_search_block.clone()
        assert tuple(alone.shape) == (S.domain_search_floats(L, 2),) and eng.domain_hits["domains"] == int(blocks["domains_block"][0].item())
        # the engine turns "domains" on itself, with the defaults: the 24 residues then stay whole, and row 0 is the whole search
        eng.predict(aln, None, ITERATIONS, MINSTEPS, library=library)
        eng.sync_check()
        assert eng.get_option("domains") == 0 and eng.domains_block[0].item() == 1.0 and eng.domain_hits["domains"] == 1
        assert np.array_equal(_bits(eng.domain_search_block[:2]), _bits(eng.search_block[2:4]))
        # the pipeline of two engines
        pipe.use_domains(True, **FORCED)
        pipe.set_search(library)
        assert all(e.get_option("search_domains") == 1 for e in pipe.engines)
        tickets = [pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure) for _ in range(2)]
        kept = {t: pipe.outputs_of(t) for t in tickets}
        got = pipe.collect(tickets)
        for t in tickets:
            assert not isinstance(got[t], Exception), got[t]
            assert len(got[t]) == 4 + len(OTHERS)
            for name, a, b in zip(("coords", "confs", "distmap", "info") + OTHERS, got[t], without + [blocks[n] for n in OTHERS]):
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), name
            assert np.array_equal(_bits(kept[t].domain_search_block), _bits(alone))
            assert np.array_equal(_bits(pipe.collected[t].domain_search_block), _bits(alone))
        library.domains = False
        pipe.set_search(library)
        assert all(e.get_option("search_domains") == 0 and e.get_option("domains") == 1 for e in pipe.engines)
    finally:
        library.domains = False
        pipe.close()
        eng.close()


def _raw(eng, aln, lib, lengths=None, fill=-7777.0, iterations=0, bits=0):
    """dmp_predict with "domains", "search_structures" and "search_domains" into a poisoned buffer with a guard ->
    (coords, host buffer, Layout)."""
    L, K = aln.shape[1], len(lib)
    lay = S.Layout(L, search=(K, lib.rows), max_L=MAX_L, domains=True, search_domains=True)
    packed = S.pack_library(lib, L, lengths=lengths)
    packed[K:26 * K + 2 * L * K] = fill
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.full((15 * L + GUARD,), fill, dtype=torch.float32, device=eng.device)
    buf = torch.full((lay.total + GUARD,), fill, dtype=torch.float32, device=eng.device)
    buf[lay.search_off:lay.search_off + len(packed)] = torch.from_numpy(packed).to(eng.device)
    opts = (("domains_tau_milli", 1000), ("domains_min_size", 8), ("domains_min_segment", 2), ("domains", 1),
            ("search_max_m", lib.max_m), ("search_structures", K), ("search_domains", 1))
    before = [(k, eng.get_option(k)) for k, _ in opts]
    try:
        for k, v in opts:
            eng.set_option(k, v)
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), aln.shape[0], L, None, 0, iterations, 0, coords.data_ptr(), buf.data_ptr(),
                                 eng.stream())
        assert rc == 0, eng.lib.dmp_last_error()
        assert eng.sync_faults() == bits
    finally:
        for k, v in reversed(before):
            eng.set_option(k, v)
    return coords, buf.cpu().numpy(), lay, packed


def test_raw_call_writes_its_out_slots_only(eng):
    L = 65
    c = _multi(eng, L)
    lib, K, fill = c["lib"], len(c["lib"]), np.float32(-7777.0)
    coords, h, lay, packed = _raw(eng, c["aln"], lib)
    assert lay.domain_search_off == L + S.domains_floats(L) == lay.align_off - S.domain_search_floats(L, K) and lay.search_off == lay.align_off
    assert (h[lay.total:] == fill).all() and (coords[15 * L:] == float(fill)).all(), "a guard float was written"
    sb = h[lay.search_off:lay.search_end]
    assert np.array_equal(_bits(sb[:K]), _bits(packed[:K])) and np.array_equal(_bits(sb[26 * K + 2 * L * K:]), _bits(packed[26 * K + 2 * L * K:]))
    assert np.array_equal(_bits(coords[:15 * L]), _bits(c["got"]["coords"])) and np.array_equal(_bits(h[:L]), _bits(c["got"]["confs"]))
    assert np.array_equal(_bits(h[L:lay.domain_search_off]), _bits(c["got"]["dom"]))
    assert np.array_equal(_bits(h[lay.domain_search_off:lay.align_off]), _bits(c["got"]["ds"]))
    assert np.array_equal(_bits(sb), _bits(c["got"]["search"]))
    assert not (h[:lay.total] == fill).any(), "an out slot was left unwritten"
    # an invalid m_k: NaN in the whole new block, no fault, the guard untouched
    lengths = lib.lengths.astype(np.float32)
    lengths[3] = 2.0
    coords, h, lay, packed = _raw(eng, c["aln"], lib, lengths=lengths)
    assert np.isnan(h[lay.domain_search_off:lay.align_off]).all()
    assert (h[lay.total:] == fill).all() and np.array_equal(_bits(h[L:lay.domain_search_off]), _bits(c["got"]["dom"]))
    assert np.isnan(h[lay.search_off + 2 * K:lay.search_off + 26 * K + 2 * L * K]).all()


def test_latched_fault_gives_nan_in_the_whole_block(eng):
    """A residue code of 22 raises the device-side flag DMP_FAULT_BAD_CODE (a software flag, not a GPU fault): the latch
    covers the block like every other block inside the layout's total."""
    from dmpfold2_amd.predict import FAULT_BAD_CODE
    L = 65
    c = _multi(eng, L)
    aln = c["aln"].copy()
    aln[0, 5] = 22
    fill, K = np.float32(-7777.0), len(c["lib"])
    coords, h, lay, packed = _raw(eng, aln, c["lib"], iterations=1, bits=FAULT_BAD_CODE)
    assert np.isnan(h[:lay.align_off]).all() and bool(torch.isnan(coords[:15 * L]).all())
    sb = h[lay.search_off:lay.search_end]
    assert np.isnan(sb[K:26 * K + 2 * L * K]).all() and np.array_equal(_bits(sb[:K]), _bits(packed[:K]))
    assert (h[lay.total:] == fill).all(), "the NaN fill went past the buffer"
    # the next prediction on the engine is whole again
    again = _search(eng, c["aln"], c["lib"], mode=1, params=FORCED)
    assert np.array_equal(_bits(again["ds"]), _bits(c["got"]["ds"]))


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors(eng):
    from dmpfold2_amd import _lib
    for bad in (-1, 3):
        with pytest.raises(_lib.DmpError, match="search_domains"):
            eng.set_option("search_domains", bad)
    assert eng.get_option("search_domains") == 0
    aln, coords0, _, model = _plain(eng, 17)
    lib = S.Library.from_traces([random_walk(9, 1), random_walk(12, 2)])
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.empty((17 * 15,), dtype=torch.float32, device=eng.device)
    buf = torch.empty((S.Layout(17, search=(2, lib.rows), domains=True, search_domains=True).total,), dtype=torch.float32, device=eng.device)
    for on in (("domains",), ("search_structures",)):
        try:
            eng.set_option("search_domains", 1)
            for name in on:
                eng.set_option(name, 2 if name == "search_structures" else 1)
            rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, 17, None, 0, 0, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
            assert rc == -1, "DMP_ERR_ARG: the prediction does not begin"
            assert "search_domains" in eng.lib.dmp_last_error().decode()
        finally:
            for name in on + ("search_domains",):
                eng.set_option(name, 0)
    # the engine is whole again, and the host layers leave the options as they were
    lib.domains = True
    c, _ = eng.predict(aln, None, 0, 0, library=lib)
    eng.sync_check()
    assert torch.equal(c, coords0) and eng.domain_hits["domains"] == 1
    assert [eng.get_option(k) for k in ("search_domains", "domains", "search_structures")] == [0, 0, 0]
    eng.predict(aln, None, 0, 0)
    eng.sync_check()
    assert eng.domain_search_block is None and eng.domain_hits is None


def test_scratch_is_counted_when_the_option_is_first_turned_on(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 64, 1)
    try:
        base = e.get_option("device_mib")
        e.set_option("search_domains", 1)
        grown = e.get_option("device_mib")
        # 2 x 16 x 4096 x 4 bytes of tables, 128 of counts, 4 max_L of list: half a MiB and a little, counted in bytes and read
        # back in whole MiB rounded up - so one more, or the same
        assert base <= grown <= base + 1
        e.set_option("search_domains", 0)
        e.set_option("search_domains", 2)
        assert e.get_option("device_mib") == grown
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 8. front ends
def _write_pdb(path, ca, chain="A"):
    with open(path, "w") as fh:
        for k, xyz in enumerate(ca):
            fh.write("ATOM  %5d  CA  %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n"
                     % (k + 1, S.AA3[k % 20], chain, k + 1, xyz[0], xyz[1], xyz[2]))
        fh.write("TER\nEND\n")


def test_front_ends(tmp_path, weights_file, monkeypatch):
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
        parse = R.parse(model, **FORCED_REF)
        D = parse["header"][0]
        folds = tmp_path / "folds"
        folds.mkdir()
        _write_pdb(str(folds / "a_walk.pdb"), random_walk(L + 11, 1))
        _write_pdb(str(folds / "b_copy.pdb"), moved(model, 5)[2])
        _write_pdb(str(folds / "c_part.pdb"), moved(SR.gather(model, parse["labels"], D - 1), 6)[2])
        lib = S.Library.from_dir(str(folds))
        lib.save(str(tmp_path / "folds.npz"))
        args = ["-i", str(p), "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file, "--search", str(folds), "--search-top", "2",
                "--domains", "--domains-tau", "1.0", "--domains-min-size", "8", "--domains-min-segment", "2"]
        texts, errs = [], []
        for extra in ([], ["--search-domains"], ["--search-domains", "--hits", str(tmp_path / "hits.json"), "--domains-file", str(tmp_path / "dom.json")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        first = [json.loads(line) for line in errs[0].strip().split("\n")]
        second = [json.loads(line) for line in errs[1].strip().split("\n")]
        assert "domain_hits" not in first[0] and first[1] == second[1], "the domains line"
        dh = second[0].pop("domain_hits")
        assert second[0] == first[0], "the hits line but for its new key"
        assert json.loads((tmp_path / "hits.json").read_text())["domain_hits"] == dh
        assert len(dh) == D >= 2 and [d["domain"] for d in dh] == list(range(D))
        assert [d["size"] for d in dh] == parse["table"][:, 0].tolist()
        assert all(len(d["hits"]) == 2 and set(d["hits"][0]) == {"name", "index", "tm_domain", "tm_struct", "rmsd_ali", "n_ali", "R", "t"} for d in dh)
        assert dh[D - 1]["hits"][0]["name"] == "c_part" and dh[D - 1]["hits"][0]["tm_domain"] > 0.99
        assert dh[D - 1]["segments"] == S._segments(parse["labels"], D - 1)
        assert P._ENGINES[0].get_option("search_domains") == 0 and P._ENGINES[0].get_option("domains") == 0
        with pytest.raises(SystemExit):
            with contextlib.redirect_stderr(io.StringIO()):
                run_dmpfold(["-i", str(p), "--search-domains"])
        common = ["-i", str(p), "-n", "1", "-m", "0", "-w", weights_file, "--streams", "2", "--library", str(tmp_path / "folds.npz"),
                  "--search-top", "2", "--domains", "--domains-tau", "1.0", "--domains-min-size", "8", "--domains-min-segment", "2"]
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(common + ["-o", str(out_dir), "--format", fmt, "--search-domains"])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 1 and summary["domain_searched_targets"] == 1
            assert [b["name"] for b in summary["domain_hits"]["pf"]] == [d["hits"][0]["name"] for d in dh]
            if fmt == "pdb":
                assert (out_dir / "pf.pdb").read_text() == texts[0]
                assert json.loads((out_dir / "pf.domain_hits.json").read_text())["domains"] == dh
            else:
                z = np.load(str(out_dir / "pf.npz"))
                assert z["dom_hit_rank"].shape == (D, 3) and z["dom_hit_tm"].shape == (D, 3) and z["dom_hit_rank"].dtype == np.int32
                assert [lib.names[k] for k in z["dom_hit_rank"][:, 0]] == [d["hits"][0]["name"] for d in dh]
                assert np.float32(z["dom_hit_tm"][D - 1, 2]) == np.float32(dh[D - 1]["hits"][0]["tm_domain"])
    finally:
        P._ENGINES.clear()
