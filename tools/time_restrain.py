"""What restraining the final refinement to the predicted distance map (option "restrain_milli") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, for a one-row alignment at L = 96, 300, 1000 and 2048 (-n 0 -m 100), in
    alternating runs of three settings: the plain end, "emit_distmap" alone, and that with "restrain_milli" = 1000 (cutoff
    15 A).  Medians of --repeats runs each; the third minus the second is what the restraint term adds to the 100 steps of
    the minimiser - one more read of the map per pair and step, a compare, and for the restrained pairs a clamp, a divide
    per component and three multiply-subtracts;
  * the restrained share of the pairs, map_rms of both ends and the report (predict.restrain_report) of the last run;
  * --parity: the step against the NumPy restatement of tests/restrain_ref.py at the lengths and step counts of
    tests/test_gpu_restrain.py, both forms of the minimiser - the deviation from the float64 restatement and the bound
    max(1e-5 A, 4 x the float32 restatement's own deviation).

    python tools/time_restrain.py [--repeats 5] [--precision 2] [--lengths 96 300 1000 2048] [--steps 100] [--parity]

Prints one line per length; profiles/restrain.txt keeps a run.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restrain_ref as R                                         # noqa: E402  (the test suite's restatement)
from dmpfold2_amd import score as S                              # noqa: E402
from dmpfold2_amd import synth                                   # noqa: E402
from dmpfold2_amd.predict import Engine, encode_aln, restrain_report  # noqa: E402

SETTINGS = ((0, 0), (1, 0), (1, 1000))          # ("emit_distmap", "restrain_milli")


def end_ms(eng, d_msa, steps, coords, conf):
    """One prediction through the unit calls; returns the milliseconds dmp_predict_end's work took on the stream."""
    lib, s = eng.lib, eng.stream()
    n, L = d_msa.shape
    assert lib.dmp_predict_begin_units(eng.ctx, d_msa.data_ptr(), n, L, None, 0, 0, steps) == 0, lib.dmp_last_error()
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
    lay = S.Layout(L, distmap=True)
    conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
    ts, rms = [[], [], []], [None, None, None]
    for rep in range(args.repeats + 2):
        for k, (emit, milli) in enumerate(SETTINGS):
            eng.set_option("emit_distmap", emit)
            eng.set_option("restrain_milli", milli)
            t = end_ms(eng, d_msa, args.steps, coords, conf)
            if rep >= 2:
                ts[k].append(t)
            if emit:
                rms[k] = float(conf[lay.info_off + 2].item())
    bits = eng.sync_faults()
    med = [float(np.median(t)) for t in ts]
    out = lay.split(conf)
    rep = restrain_report(1.0, 15.0, args.steps, out.distmap, rms[2], coords)
    far = L * (L - 1) // 2 - (L - 1)
    print("L=%d precision %d -m %d, medians of %d: dmp_predict_end plain %.3f ms (min %.3f, max %.3f); + emit_distmap %.3f ms (min %.3f, "
          "max %.3f); + restrain_milli 1000 %.3f ms (min %.3f, max %.3f): the restraints cost %+.3f ms, %+.1f %% of the plain end; "
          "restrained %.3f of %d pairs; map_rms %.3f -> %.3f A (ratio %.3f); clashes %d, bond_dev_max %.3f A; fault bits %d"
          % (L, args.precision, args.steps, args.repeats, med[0], min(ts[0]), max(ts[0]), med[1], min(ts[1]), max(ts[1]), med[2],
             min(ts[2]), max(ts[2]), med[2] - med[1], 100.0 * (med[2] - med[1]) / med[0], rep["restrained_pairs"] / far, far,
             rms[1], rms[2], rms[2] / rms[1], rep["clashes"], rep["bond_dev_max"], bits), flush=True)
    eng.set_option("emit_distmap", 0)
    eng.set_option("restrain_milli", 0)
    eng.close()


def parity(weights, lengths=(8, 31, 32, 33, 64, 65, 257), steps=(1, 3, 10)):
    eng = Engine("cuda:0", 300, 3000)
    eng.set_weights(weights)
    for single in (0, 1):
        eng.set_option("refine_single", single)
        for L in lengths:
            alnmat = np.ascontiguousarray(encode_aln(synth.synth_msa(L, 8 if L == 65 else 1, 1000 + L)))
            for m in steps:
                coords, confs, dm, info = eng.predict(alnmat, None, 1, m, distmap=True, restrain=1.0)
                bits = eng.sync_faults()
                start = eng.fetch("best_ca", 3 * L).cpu().numpy().reshape(L, 3)
                kept = dm.cpu().numpy()
                r64 = R.refine(start, m, kept, 1.0, 15.0, np.float64)
                r32 = R.refine(start, m, kept, 1.0, 15.0, np.float32)
                bound = max(1e-5, 4.0 * float(np.abs(r32.astype(np.float64) - r64).max()))
                dev = float(np.abs(coords[:, 1].cpu().numpy().astype(np.float64) - r64).max())
                share = float((kept[np.triu(np.ones((L, L), dtype=bool), 2)] < np.float32(15.0)).mean())
                print("parity %s L=%d m=%d: deviation from the float64 restatement %.3e A, bound %.3e A (%s), restrained share %.3f, "
                      "fault bits %d" % ("refine_single" if single else "default form", L, m, dev, bound,
                                         "within" if dev <= bound else "OUTSIDE", share, bits), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--lengths", type=int, nargs="*", default=[96, 300, 1000, 2048])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--parity", action="store_true")
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    if args.parity:
        parity(weights)
    for L in args.lengths:
        measure(L, args, weights)


if __name__ == "__main__":
    main()
