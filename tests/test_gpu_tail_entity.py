"""The native entity that "assign_ss", "exposure" and "domains" share: prepared once, whichever of the three are on.

With "score_native" on, the three options read one preparation of the score block's native trace (is it whole, its rebuilt
backbone) and one capture of the alignment's first row.  Through the public Python API only, and bit for bit (the yardstick is
the library itself: every fact here holds on the commit before the three shared anything):

  * every non-empty subset of the three gives the blocks of the call with all three on;
  * a shorter prediction after a longer one gives what a fresh engine gives - nothing of the longer first row or backbone is read;
  * the two predicates stay two: a native with a NaN only in one y is whole to "assign_ss" and "exposure" (no NaN x) and not
    to "domains" (no NaN coordinate); one with a row of NaN is whole to none of them;
  * a pipeline of two streams gives every target the blocks the lone engine gives.

Engines of max_L = 33 (synthetic weights, precision 2), one-row alignments of L = 8, 9 and 33, one iteration.
"""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from test_align_cpu import moved

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

MAX_L = 33
THREE = ("ss", "exposure", "domains")
DOMAINS = (1.0, 8, 2)               # tau, min_size, min_segment


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _engine(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", MAX_L, 1)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    e.set_option("tridiag_cluster", 0)          # (as the pipeline's engines)
    return e


@pytest.fixture(scope="module")
def eng(synth_sd):
    e = _engine(synth_sd)
    yield e
    e.close()


def _bits(x):
    return x.detach().cpu().numpy().reshape(-1).view(np.uint32).copy()


def _aln(L):
    from dmpfold2_amd import synth
    return np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L)))


_NATIVES = {}


def _native(eng, L):
    """A whole native of length L, made once from the plain prediction's own trace."""
    if L not in _NATIVES:
        coords, _ = eng.predict(_aln(L), None, 1, 0)
        eng.sync_check()
        model = coords[:, 1].cpu().numpy().astype(np.float64)
        _NATIVES[L] = moved(model + np.random.default_rng(L).normal(scale=0.8, size=model.shape), 3)[2].astype(np.float32)
    return _NATIVES[L].copy()


def _call(e, L, native, on=THREE):
    """One prediction with the options `on` -> {block name: bits} of the blocks it left (coords and confs among them)."""
    with e.with_domains(*DOMAINS) if "domains" in on else contextlib.nullcontext():
        coords, confs = e.predict(_aln(L), None, 1, 0, native=native, ss="ss" in on, exposure="exposure" in on)
    e.sync_check()
    got = {"coords": _bits(coords), "confs": _bits(confs), "score_block": _bits(e.score_block)}
    for name in THREE:
        block = getattr(e, name + "_block")
        assert (block is not None) == (name in on), (name, on)
        if block is not None:
            got[name + "_block"] = _bits(block)
    return got


def _same(got, want, tag):
    for name in got:
        assert np.array_equal(got[name], want[name]), "%s: %s differs" % (tag, name)


def test_every_subset_of_the_three_gives_the_blocks_of_all_three(eng):
    L = 9
    native = _native(eng, L)
    full = _call(eng, L, native)
    assert eng.ss_block[11].item() == 1.0 and eng.exposure_block[8].item() == 1.0 and eng.domains_block[16].item() >= 1.0
    for k in (1, 2):
        for on in itertools.combinations(THREE, k):
            _same(_call(eng, L, native, on), full, "+".join(on))
    _same(_call(eng, L, native), full, "all three again")


def test_a_shorter_prediction_after_a_longer_one_reads_nothing_stale(eng, synth_sd):
    on = ("ss", "exposure")
    long_native, short_native = _native(eng, 33), _native(eng, 8)
    fresh = _engine(synth_sd)
    try:
        want = _call(fresh, 8, short_native, on)
    finally:
        fresh.close()
    _call(eng, 33, long_native, on)
    _same(_call(eng, 8, short_native, on), want, "L = 8 after L = 33")


def test_the_two_predicates_stay_two(eng):
    L = 9
    # a NaN only in y of row 5: no NaN x, so whole to "assign_ss" and "exposure"; a NaN coordinate, so not whole to "domains"
    native = _native(eng, L)
    native[5, 1] = np.nan
    first = _call(eng, L, native)
    assert eng.ss_block[11].item() == 1.0 and eng.exposure_block[8].item() == 1.0
    dom = eng.domains_block.cpu().numpy()
    assert not dom[16:32].any() and np.isnan(dom[32 + L:32 + 2 * L]).all() and dom[0] >= 1.0
    _same(_call(eng, L, native), first, "NaN in one y, again")
    # a row of NaN: whole to none of them
    native = _native(eng, L)
    native[5] = np.nan
    first = _call(eng, L, native)
    assert eng.ss_block[11].item() == 0.0 and eng.exposure_block[8].item() == 0.0
    assert bool(torch.isnan(eng.ss_block[32 + 7 * L:]).all()) and bool(torch.isnan(eng.exposure_block[32 + 8 * L:]).all())
    dom = eng.domains_block.cpu().numpy()
    assert not dom[16:32].any() and np.isnan(dom[32 + L:32 + 2 * L]).all() and dom[0] >= 1.0
    _same(_call(eng, L, native), first, "a row of NaN, again")


def test_pipeline_of_two_streams_gives_the_engine_s_blocks(eng, synth_sd):
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Pipeline
    L = 9
    alns = [np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 2000 + k))) for k in range(3)]
    natives = [_native(eng, L) + np.float32(k) for k in range(3)]
    natives[1][5, 1] = np.nan                   # (one target whose native the two predicates see differently)
    names = ("coords", "confs", "score_block", "ss_block", "exposure_block", "domains_block")
    refs = []
    for aln, native in zip(alns, natives):
        with eng.with_domains(*DOMAINS):
            coords, confs = eng.predict(aln, None, 1, 0, native=native, ss=True, exposure=True)
        eng.sync_check()
        refs.append([_bits(x) for x in (coords, confs, eng.score_block, eng.ss_block, eng.exposure_block, eng.domains_block)])
    dev = torch.device("cuda:0")
    pipe = Pipeline(dev, MAX_L, 1, _tensors(synth_sd), streams=2, precision=2)
    try:
        pipe.set_score(True)
        pipe.set_ss(True)
        pipe.set_exposure(True)
        pipe.use_domains(True, *DOMAINS)
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), 1, 0, native=n) for a, n in zip(alns, natives)]
        res = pipe.collect(tickets)
        for k, (t, ref) in enumerate(zip(tickets, refs)):
            assert not isinstance(res[t], Exception), res[t]
            assert len(res[t]) == len(names)
            for name, got, want in zip(names, res[t], ref):
                assert np.array_equal(_bits(got), want), "target %d: %s differs from the engine's" % (k, name)
    finally:
        pipe.close()
