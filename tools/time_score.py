"""What scoring a prediction against a native trace (option "score_native") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, option on minus option off in alternating runs, for a one-row
    alignment at L = 96, 300, 1000 and 2048 (-n 0 -m 0: the end is the backbone builder, the fault latch and - with the
    option on - score_prep, score_lddt and score_search);
  * beside it the CPU time of the float64 NumPy yardstick of tests/test_score_cpu.py on the same traces (up to
    --yardstick-max-L: it is a test oracle, not a product).

    python tools/time_score.py [--repeats 15] [--precision 2] [--lengths 96 300 1000 2048] [--yardstick-max-L 1000]

The native is the model's own trace rigidly moved with 1.5 A of noise and a displaced stretch: a good model, where the
search runs its longest.  Prints one line per length; profiles/score.txt keeps a run.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dmpfold2_amd import score as S                              # noqa: E402
from dmpfold2_amd import synth                                   # noqa: E402
from dmpfold2_amd.predict import Engine, encode_aln              # noqa: E402
from test_score_cpu import seed_fragments, yardstick             # noqa: E402  (the test suite's float64 restatement)


def end_ms(eng, d_msa, coords, conf):
    """One prediction through the unit calls; returns the milliseconds dmp_predict_end's work took on the stream."""
    lib, s = eng.lib, eng.stream()
    n, L = d_msa.shape
    assert lib.dmp_predict_begin_units(eng.ctx, d_msa.data_ptr(), n, L, None, 0, 0, 0) == 0, lib.dmp_last_error()
    while lib.dmp_predict_next_unit(eng.ctx) != 0:
        assert lib.dmp_predict_issue_unit(eng.ctx, s) == 0, lib.dmp_last_error()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert lib.dmp_predict_end(eng.ctx, coords.data_ptr(), conf.data_ptr(), s) == 0, lib.dmp_last_error()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    eng = Engine("cuda:0", L, 1, precision=args.precision)
    eng.set_weights(weights)
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
    conf = torch.empty((S.Layout(L, score=True).total,), dtype=torch.float32, device=eng.device)
    end_ms(eng, d_msa, coords, conf)
    model = coords[:, 1].cpu().numpy()
    rng = np.random.default_rng(L)
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    native = model.astype(np.float64) @ R.T + 7.0 + rng.normal(scale=1.5 / np.sqrt(3.0), size=model.shape)
    native[L // 3:L // 3 + L // 8] += 9.0
    native = native.astype(np.float32)
    conf[L:] = torch.from_numpy(S.pack_native(native, 0.0, L)).to(eng.device)
    ts = {0: [], 1: []}
    for rep in range(args.repeats + 3):
        for on in (0, 1):
            eng.set_option("score_native", on)
            t = end_ms(eng, d_msa, coords, conf)
            if rep >= 3:
                ts[on].append(t)
    eng.set_option("score_native", 0)
    sc = S.unpack_scores(conf[L:], L)
    off, on = np.array(ts[0]), np.array(ts[1])
    line = ("L=%d (%d seeds) precision %d, %d runs: dmp_predict_end off median %.3f ms (min %.3f, max %.3f); on median %.3f ms "
            "(min %.3f, max %.3f); difference of medians %+.3f ms; tm %.4f lddt %.4f"
            % (L, len(seed_fragments(sc["n_pairs"])), args.precision, args.repeats, np.median(off),
               off.min(), off.max(), np.median(on), on.min(), on.max(), np.median(on) - np.median(off), sc["tm"], sc["lddt"]))
    if L <= args.yardstick_max_L:
        t0 = time.perf_counter()
        want, _ = yardstick(model, native, 0.0)
        line += "; yardstick on the CPU %.0f ms (tm %.4f)" % ((time.perf_counter() - t0) * 1e3, want["tm"])
    print(line, flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--lengths", type=int, nargs="*", default=[96, 300, 1000, 2048])
    ap.add_argument("--yardstick-max-L", type=int, default=1000)
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    for L in args.lengths:
        measure(L, args, weights)


if __name__ == "__main__":
    main()
