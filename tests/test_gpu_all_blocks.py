"""All seven blocks behind the confidences on together, through one `Engine` call and through one `Pipeline` submission: the
pipeline's blocks are the engine's bit for bit, and each is the block of a run with that option (and what it needs) alone.
The one place where a wrong walk of score.BLOCKS - an offset, an order, a block handed out under another's name - shows
against the real library.  L = 16, N = 4, one recycling pass, five minimisation steps; the native lacks a row, so neither the
SS nor the exposure block carries a native leg and both are what a run without a native gives."""
import numpy as np
import pytest
import torch

from test_align_cpu import random_walk

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

L, N, ITERATIONS, MINSTEPS = 16, 4, 1, 5
# the engine's name of every block, in the order a pipeline hands them out
BLOCKS = ("score_block", "align_block", "search_block", "map_score_block", "pass_block", "ss_block", "exposure_block")


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).reshape(-1).view(np.uint32)


def test_all_seven_blocks_engine_pipeline_and_each_alone(synth_sd):
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, Pipeline
    aln = np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, N, 1016)))
    native = random_walk(L, 1).astype(np.float32)
    native[5] = np.nan
    structure = random_walk(12, 2).astype(np.float32)
    library = S.Library.from_traces([random_walk(8, 3), random_walk(12, 4)])
    alone = {"score_block": dict(native=native), "map_score_block": dict(native=native, score_map=True),
             "pass_block": dict(native=native, score_passes=True), "ss_block": dict(ss=True), "exposure_block": dict(exposure=True),
             "align_block": dict(structure=structure), "search_block": dict(library=library)}
    everything = dict(distmap=True, native=native, structure=structure, library=library, score_map=True, score_passes=True, ss=True,
                      exposure=True)
    dev, sdt = torch.device("cuda:0"), {k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()}
    eng = Engine(dev, L, N)
    eng.set_weights(sdt)
    eng.set_option("precision", 2)
    eng.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, L, N, sdt, streams=2, precision=2, distmap=True, score=True, align=True, search=library, score_map=True,
                    score_passes=True, ss=True, exposure=True)
    try:
        full = [x.clone() for x in eng.predict(aln, None, ITERATIONS, MINSTEPS, **everything)]
        eng.sync_check()
        blocks = {name: getattr(eng, name).clone() for name in BLOCKS}
        sizes = {"score_block": 5 * L + 24, "map_score_block": 64 + L, "pass_block": 16 + 8 * 2, "ss_block": 32 + 8 * L,
                 "exposure_block": 32 + 16 * L, "align_block": 25 + 2 * L + 3 * 12, "search_block": 26 * 2 + 2 * L * 2 + 3 * 20}
        assert len(full) == 4 and {name: tuple(b.shape) for name, b in blocks.items()} == {name: (n,) for name, n in sizes.items()}
        assert all(eng.get_option(row.option) == 0 for row in S.BLOCKS) and eng.get_option("emit_distmap") == 0
        # the pipeline: everything the engine gave, in the hand-out order
        ticket = pipe.submit(torch.from_numpy(aln).to(dev), ITERATIONS, MINSTEPS, native=native, structure=structure)
        res = pipe.collect([ticket])[ticket]
        assert not isinstance(res, Exception), res
        assert len(res) == 4 + len(BLOCKS)
        for name, got, want in zip(("coords", "confs", "distmap", "info") + BLOCKS, res, full + [blocks[name] for name in BLOCKS]):
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), name
        # each block alone: the option and what it needs, nothing else
        for name, asked in alone.items():
            coords, confs = eng.predict(aln, None, ITERATIONS, MINSTEPS, **asked)
            eng.sync_check()
            assert np.array_equal(_bits(coords), _bits(full[0])) and np.array_equal(_bits(confs), _bits(full[1])), name
            assert np.array_equal(_bits(getattr(eng, name)), _bits(blocks[name])), name
            needs = {"map_score_block": {"score_block"}, "pass_block": {"score_block"}}.get(name, set())
            assert all((getattr(eng, other) is None) == (other != name and other not in needs) for other in BLOCKS), name
    finally:
        pipe.close()
        eng.close()
