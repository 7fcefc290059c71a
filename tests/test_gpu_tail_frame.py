"""Every option at a prediction's end on at once: the scratch of each lies beside the others', and its head is zero again.

The options at the end of a prediction ("emit_distmap", "score_native", "score_map", "score_passes", "assign_ss", "exposure",
"domains", "align_structure", "search_structures") each own one device scratch carved by a layout function, a head in front of
it zero between launches.  Two properties of that frame, through the public Python API only (the yardstick is the library itself: the
test passes unchanged on the commit before the frame):

  * each block of a call with every extra on equals, bit for bit, the block of a call with that extra alone (plus the extras
    it needs) - a carved part that overlapped its neighbour would show here;
  * the same call made a second time equals the first, bit for bit - a head that was not left zero would show here.

One engine of max_L = 33 (synthetic weights, precision 2), one-row alignments of L = 8, 9 and 33, two iterations (three
passes), "search_chunk" 2 for the library of three and "score_passes_chunk" 2 for the three passes: two chunks each.
"""
import contextlib

import numpy as np
import pytest
import torch

from test_align_cpu import indel_copy, moved, random_walk

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

MAX_L = 33
BLOCKS = ("score_block", "map_score_block", "pass_block", "ss_block", "exposure_block", "domains_block", "align_block", "search_block")
DOMAINS = (1.0, 8, 2)               # tau, min_size, min_segment: every admissible cut is accepted, L = 33 has some


@pytest.fixture(scope="module")
def eng(synth_sd):
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", MAX_L, 1)
    e.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()})
    e.set_option("precision", 2)
    e.set_option("search_chunk", 2)
    e.set_option("score_passes_chunk", 2)
    yield e
    e.close()


def _bits(x):
    return x.detach().cpu().numpy().reshape(-1).view(np.uint32).copy()


def _call(eng, aln, domains=False, **extras):
    """One prediction -> {name: bits} of what it returned and of every block it left (`domains`: inside with_domains)."""
    with eng.with_domains(*DOMAINS) if domains else contextlib.nullcontext():
        ret = eng.predict(aln, None, 2, 0, **extras)
    eng.sync_check()
    got = {name: _bits(t) for name, t in zip(("coords", "confs", "distmap", "info"), ret)}
    for name in BLOCKS:
        block = getattr(eng, name)
        if block is not None:
            got[name] = _bits(block)
    return got


def _inputs(eng, L):
    """The extras of length L, made from the plain prediction's own trace: a whole native (so that "assign_ss" assigns it too),
    a structure of m = L + 2 rows where the engine holds that many, else L - 2, and a library of three."""
    from dmpfold2_amd import synth
    aln = np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L)))
    coords, _ = eng.predict(aln, None, 2, 0)
    eng.sync_check()
    model = coords[:, 1].cpu().numpy()
    native = moved(model.astype(np.float64) + np.random.default_rng(L).normal(scale=0.8, size=model.shape), 3)[2]
    m = L + 2 if L + 2 <= MAX_L else L - 2
    structure = indel_copy(model, 100 + L, m=m)[0]
    library = S.Library.from_traces([indel_copy(model, 200 + L, m=max(L - 3, 3))[0], random_walk(MAX_L, 50 + L), moved(model, 9)[2]],
                                    ["shorter", "capacity", "rigid"])
    return aln, native, structure, library


@pytest.mark.parametrize("L", [8, 9, 33])
def test_every_extra_at_once_equals_each_alone_and_repeats(eng, L):
    aln, native, structure, library = _inputs(eng, L)
    every = dict(distmap=True, native=native, structure=structure, library=library, score_map=True, score_passes=True, ss=True,
                 exposure=True)
    first = _call(eng, aln, domains=True, **every)
    assert set(first) == {"coords", "confs", "distmap", "info"} | set(BLOCKS)
    assert first["pass_block"].size == S.pass_floats(3) and first["search_block"].size == S.search_floats(L, 3, library.rows)

    # each block against the call with that extra alone, plus the extras it needs
    alone = {"distmap": dict(distmap=True),
             "info": dict(distmap=True),
             "score_block": dict(native=native),
             "map_score_block": dict(native=native, score_map=True),
             "pass_block": dict(native=native, score_passes=True),
             "ss_block": dict(native=native, ss=True),          # (with a native the block holds the native's assignment too)
             "exposure_block": dict(native=native, exposure=True),
             "domains_block": dict(native=native, domains=True),
             "align_block": dict(structure=structure),
             "search_block": dict(library=library)}
    calls = {}
    for name, extras in alone.items():
        key = tuple(sorted(extras))
        if key not in calls:
            calls[key] = _call(eng, aln, **extras)
        solo = calls[key]
        assert np.array_equal(solo[name], first[name]), "L = %d: %s differs from the call with %s alone" % (L, name, key)
        assert np.array_equal(solo["coords"], first["coords"]) and np.array_equal(solo["confs"], first["confs"])

    # the same call again
    second = _call(eng, aln, domains=True, **every)
    for name in first:
        assert np.array_equal(second[name], first[name]), "L = %d: %s differs in the second call" % (L, name)
