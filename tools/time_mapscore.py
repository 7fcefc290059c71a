"""What scoring the predicted distance map against the native (option "score_map") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, for a one-row alignment at L = 96, 300, 1000 and 2048 (-n 0 -m 0), in
    alternating runs of three settings: "emit_distmap" alone, that with "score_native", and those two with "score_map".
    Medians of --repeats runs each; the second minus the first is score_native's own cost, the third minus the second what
    score_map adds to the end of a prediction that already has the two options it needs;
  * the block the last run left is compared with the NumPy yardstick of tests/test_mapscore_cpu.py (every count equal, the
    floats within one float32 ulp) - the only place L = 2048, 2.1 M pairs in the long class, is checked;
  * --tie-sweep: the head of tests/test_gpu_mapscore.py::test_tie_heavy_map (resnet.17.weight times 2^-k, distance bias 5)
    for k = 0 .. 30 at L = 64 - whether the plain prediction is finite and what share of the candidates share their map
    value with another pair.

  * --tie-head K: the timing with that head at shrink 2^-K instead of the plain weights - runs of equal map values at
    every list end, so the selection reads each class 8 times instead of 5: its worst case.

    python tools/time_mapscore.py [--repeats 5] [--precision 2] [--lengths 96 300 1000 2048] [--tie-sweep] [--tie-head K]

The native is the model's own trace rigidly moved with 1.5 A of noise and a displaced stretch, as in tools/time_score.py.
Prints one line per length; profiles/mapscore.txt keeps a run.
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
from test_mapscore_cpu import compare_with_yardstick, yardstick  # noqa: E402  (the test suite's restatement)

SETTINGS = (("emit_distmap",), ("emit_distmap", "score_native"), ("emit_distmap", "score_native", "score_map"))


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


def set_options(eng, names):
    for k in ("score_map", "score_native", "emit_distmap"):
        eng.set_option(k, 1 if k in names else 0)


def measure(L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    eng = Engine("cuda:0", L, 1, precision=args.precision)
    eng.set_weights(weights)
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
    lay = S.Layout(L, distmap=True, score=True, score_map=True)
    conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
    set_options(eng, SETTINGS[0])
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
    conf[lay.score_off:lay.mapscore_off] = torch.from_numpy(S.pack_native(native, 0.0, L)).to(eng.device)
    ts = [[], [], []]
    for rep in range(args.repeats + 2):
        for k, names in enumerate(SETTINGS):
            set_options(eng, names)
            t = end_ms(eng, d_msa, coords, conf)
            if rep >= 2:
                ts[k].append(t)
    set_options(eng, ())
    med = [float(np.median(t)) for t in ts]
    ms = S.unpack_map_scores(lay.split(conf).map_block, L)
    line = ("L=%d precision %d, medians of %d: dmp_predict_end with emit_distmap %.3f ms (min %.3f, max %.3f); + score_native %.3f ms "
            "(min %.3f, max %.3f): its own cost %+.3f ms; + score_map %.3f ms (min %.3f, max %.3f): its cost %+.3f ms; "
            "map_lddt %.4f mae %.3f long L/5 %d of %d"
            % (L, args.precision, args.repeats, med[0], min(ts[0]), max(ts[0]), med[1], min(ts[1]), max(ts[1]), med[1] - med[0],
               med[2], min(ts[2]), max(ts[2]), med[2] - med[1], ms["map_lddt"], ms["map_mae"], ms["classes"]["long"]["hits"][2],
               ms["classes"]["long"]["taken"][2]))
    t0 = time.perf_counter()
    dm = conf[L:L + L * L].view(L, L).cpu().numpy()
    want, margin = yardstick(dm, native, 0.0)
    try:
        seen = compare_with_yardstick(ms, want, margin, "L=%d" % L)
        line += "; equal to the yardstick (%.0f ms on the CPU; margin %.1e A; ulps %s)" % ((time.perf_counter() - t0) * 1e3, margin, seen)
    except AssertionError as exc:
        line += "; DIFFERS FROM THE YARDSTICK: %s" % (exc,)
    print(line, flush=True)
    eng.close()


def tie_head(weights, k):
    sd = dict(weights)
    sd["resnet.17.weight"] = weights["resnet.17.weight"] * float(2.0 ** -k)
    b = weights["resnet.17.bias"].clone()
    b[0] = 5.0
    sd["resnet.17.bias"] = b
    return sd


def tie_sweep(weights, L=64):
    alnmat = np.ascontiguousarray(encode_aln(synth.synth_msa(L, 1, 1000 + L)))
    i, j = np.triu_indices(L, 6)
    for k in range(0, 31, 2):
        sd = tie_head(weights, k)
        eng = Engine("cuda:0", L, 1, precision=2)
        eng.set_weights(sd)
        coords, confs, dm, info = eng.predict(alnmat, None, 0, 0, distmap=True)
        bits = eng.sync_faults()
        if bits:
            print("tie sweep L=%d shrink 2^-%d: fault bits %d" % (L, k, bits), flush=True)
        h = dm.cpu().numpy()[i, j]
        _, counts = np.unique(h, return_counts=True)
        print("tie sweep L=%d shrink 2^-%d: finite %s; %.3f of %d candidates share their value; %d distinct values in [%r, %r]"
              % (L, k, bool(torch.isfinite(coords).all() and torch.isfinite(confs).all() and torch.isfinite(dm).all()),
                 counts[counts > 1].sum() / h.size, h.size, counts.size, float(np.nanmin(h)), float(np.nanmax(h))), flush=True)
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--lengths", type=int, nargs="*", default=[96, 300, 1000, 2048])
    ap.add_argument("--tie-sweep", action="store_true")
    ap.add_argument("--tie-head", type=int, default=None, metavar="K")
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    if args.tie_sweep:
        tie_sweep(weights)
    if args.tie_head is not None:
        weights = tie_head(weights, args.tie_head)
        print("tie head: resnet.17.weight times 2^-%d, distance bias 5" % args.tie_head, flush=True)
    for L in args.lengths:
        measure(L, args, weights)


if __name__ == "__main__":
    main()
