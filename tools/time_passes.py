"""What scoring every recycling pass against a native trace (option "score_passes") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, "score_passes" + "score_native" on minus "score_native" alone on, in
    alternating runs (three contexts that hold the same finished prediction), for a one-row alignment at (L, nloops) =
    (96, 10), (300, 10), (1000, 10), (2048, 10) and (300, 100), -m 0;
  * beside it R times the single-trace cost of "score_native" from the same runs ("score_native" on minus off): what R
    separate scorings of the recorded traces would take.

    python tools/time_passes.py [--repeats 9] [--precision 2] [--cases 96:10 300:10 1000:10 2048:10 300:100]

The trunk passes before the end are not timed.  The native is the final model's own trace rigidly moved with 1.5 A of
noise and a displaced stretch, as in tools/time_score.py.  Prints one line per case; profiles/passes.txt keeps a run.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dmpfold2_amd import score as S                              # noqa: E402
from dmpfold2_amd import synth                                   # noqa: E402
from dmpfold2_amd.predict import Engine, encode_aln              # noqa: E402


def run_passes(eng, d_msa, nloops):
    """Every unit of a prediction but its end."""
    lib, s = eng.lib, eng.stream()
    n, L = d_msa.shape
    assert lib.dmp_predict_begin_units(eng.ctx, d_msa.data_ptr(), n, L, None, 0, nloops, 0) == 0, lib.dmp_last_error()
    while lib.dmp_predict_next_unit(eng.ctx) != 0:
        assert lib.dmp_predict_issue_unit(eng.ctx, s) == 0, lib.dmp_last_error()
    torch.cuda.synchronize()


def end_ms(eng, coords, conf):
    """dmp_predict_end of the prediction the engine holds (it may be called again: the same launches on the same state);
    returns the milliseconds its work took on the stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert eng.lib.dmp_predict_end(eng.ctx, coords.data_ptr(), conf.data_ptr(), eng.stream()) == 0, eng.lib.dmp_last_error()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(L, nloops, args, weights):
    """Three contexts hold the same finished prediction, begun with nothing, "score_native", and "score_native" +
    "score_passes" on; their ends are timed in turn."""
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    R = S.pass_rows(nloops)
    lay = S.Layout(L, score=True, passes=R)
    settings = {"off": (0, 0), "score": (1, 0), "passes": (1, 1)}
    engs, bufs = {}, {}
    native = None
    for name, (score, passes) in settings.items():
        eng = Engine("cuda:0", L, 1, precision=args.precision)
        eng.set_weights(weights)
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
        eng.set_option("score_native", score)
        eng.set_option("score_passes", passes)                   # (the scratch is allocated here, outside the timed region)
        run_passes(eng, d_msa, nloops)
        if native is None:                                       # the first context runs without scoring: its model makes the native
            end_ms(eng, coords, conf)
            model = coords[:, 1].cpu().numpy()
            rng = np.random.default_rng(L)
            q = rng.normal(size=4)
            w, x, y, z = q / np.linalg.norm(q)
            rot = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                            [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                            [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
            native = model.astype(np.float64) @ rot.T + 7.0 + rng.normal(scale=1.5 / np.sqrt(3.0), size=model.shape)
            native[L // 3:L // 3 + L // 8] += 9.0
            native = torch.from_numpy(S.pack_native(native.astype(np.float32), 0.0, L))
        conf[lay.score_off:lay.mapscore_off] = native.to(eng.device)
        engs[name], bufs[name] = eng, (d_msa, coords, conf)
    ts = {k: [] for k in settings}
    for rep in range(args.repeats + 2):
        for name in settings:
            t = end_ms(engs[name], *bufs[name][1:])
            if rep >= 2:
                ts[name].append(t)
    ps = S.unpack_pass_scores(bufs["passes"][2][lay.pass_off:lay.align_off], R)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    one = med["score"] - med["off"]
    extra = med["passes"] - med["score"]
    print("L=%d nloops=%d R=%d rows=%d precision %d, %d runs: dmp_predict_end medians off %.3f ms, score_native %.3f ms, "
          "+ score_passes %.3f ms (min %.3f, max %.3f); score_passes costs %+.3f ms; one trace costs %+.3f ms, R x that "
          "%.3f ms; ratio %.2f; best_pass %s tm_pass %s regret_tm %.4f"
          % (L, nloops, R, ps["rows"], args.precision, args.repeats, med["off"], med["score"], med["passes"],
             min(ts["passes"]), max(ts["passes"]), extra, one, R * one, extra / (R * one) if one > 0 else float("nan"),
             ps["best_pass"], ps["tm_pass"], ps["regret_tm"]), flush=True)
    for eng in engs.values():
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--cases", nargs="*", default=["96:10", "300:10", "1000:10", "2048:10", "300:100"], metavar="L:NLOOPS")
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    for case in args.cases:
        L, nloops = (int(v) for v in case.split(":"))
        measure(L, nloops, args, weights)


if __name__ == "__main__":
    main()
