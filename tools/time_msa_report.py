"""What the report on the alignment (option "msa_report") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, with the option 0, 1 and 2 IN THE SAME RUN: three contexts hold the same
    finished prediction (-n 0 -m 0) and their ends are timed in turn, at (N, L) = (2000, 300), (3000, 96), (3000, 1000) and
    (3000, 2048);
  * two more contexts with "score_native" and a whole folded-like native (synth.protein_like_trace), without the report and
    with it: what the ranking of the DCA map against the native adds (the class counts and the radix select);
  * beside it one `dmp_msa_weights` of the same alignment: the report's pair kernel repeats its N^2 L byte compares;
  * what "device_mib" (whole MiB, rounded up) shows of the scratch the option allocates, 320 + 16 max_N bytes.

    python tools/time_msa_report.py [--repeats 9] [--precision 2] [--shapes 2000x300 3000x96 ...] [--out profiles/msa_report.txt]

The front end and the trunk before the end are not timed.  The alignment is synth.synth_msa's.  Two untimed rounds come first
(code objects, clocks); the figures are medians with their extremes.  Prints one line per shape and, with --out, appends them
to a file.
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
from tools.time_passes import end_ms, run_passes                 # noqa: E402


def weights_ms(eng, d_msa, w):
    """One dmp_msa_weights of the alignment on the engine's stream -> milliseconds."""
    n, L = d_msa.shape
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert eng.lib.dmp_msa_weights(eng.ctx, d_msa.data_ptr(), n, L, w.data_ptr(), eng.stream()) == 0, eng.lib.dmp_last_error()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(N, L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, N, 1000 + L))
    N = alnmat.shape[0]
    engs, bufs, lays, mib = {}, {}, {}, {}
    folded = synth.protein_like_trace(L, 1).astype(np.float32)
    # name: (score_native, msa_report)
    settings = {0: (0, 0), 1: (0, 1), 2: (0, 2), "score": (1, 0), "native": (1, 1)}
    for value, (score, report) in settings.items():
        eng = Engine("cuda:0", L, N, precision=args.precision)
        eng.set_weights(weights)
        lay = S.Layout(L, score=bool(score), msa_report=report)
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
        before = eng.device_bytes
        eng.set_option("score_native", score)
        eng.set_option("msa_report", report)                     # (the scratch is allocated here, outside the timed region)
        mib[value] = int(round((eng.device_bytes - before) / float(1 << 20)))
        run_passes(eng, d_msa, 0)
        if score:
            conf[lay.score_off:lay.mapscore_off] = torch.from_numpy(S.pack_native(folded, 0.0, L)).to(eng.device)
        engs[value], bufs[value], lays[value] = eng, (d_msa, coords, conf), lay
    w = torch.empty((N,), dtype=torch.float32, device=engs[0].device)
    ts = {k: [] for k in list(settings) + ["weights"]}
    for rep in range(args.repeats + 2):
        for value in settings:
            t = end_ms(engs[value], *bufs[value][1:])
            if rep >= 2:
                ts[value].append(t)
        t = weights_ms(engs[0], bufs[0][0], w)
        if rep >= 2:
            ts["weights"].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    one = S.unpack_msa_report(lays[1].msa_report_block(bufs[1][2]), L)
    two = S.unpack_msa_report(lays[2].msa_report_block(bufs[2][2]), L)
    assert one["N"] == N and one["neff_80"] == two["neff_80"] and two["dca_map"].shape == (L, L)
    nat = S.unpack_msa_report(lays["native"].msa_report_block(bufs["native"][2]), L)
    assert nat["has_native"] and nat["n"] == L and nat["neff_80"] == one["neff_80"]
    assert abs(one["neff_80"] - float(w.double().sum().item())) <= 1e-6 * one["neff_80"]

    def spread(name):
        return "%.3f ms (min %.3f, max %.3f)" % (med[name], min(ts[name]), max(ts[name]))
    line = ("N=%d L=%d precision %d, %d runs: dmp_predict_end medians off %s, msa_report 1 %s, msa_report 2 %s; the report costs "
            "%+.3f ms, the map %+.3f ms more; one dmp_msa_weights of that alignment %s: the report is %.2f of it; with a native: score_native %s, with the report %s, the report then costs %+.3f ms (long-range top-L precision of the DCA map %.3f); device_mib (whole MiB) %+d with the option; "
            "neff_62 %.1f neff_80 %.1f neff_90 %.1f, median coverage %.3f, copies %d"
            % (N, L, args.precision, args.repeats, spread(0), spread(1), spread(2), med[1] - med[0], med[2] - med[1],
               spread("weights"), (med[1] - med[0]) / med["weights"], spread("score"), spread("native"), med["native"] - med["score"],
               nat["classes"]["long"]["precision"][0], mib[1], one["neff_62"], one["neff_80"], one["neff_90"],
               one["median_coverage"], one["copies"]))
    print(line, flush=True)
    for eng in engs.values():
        eng.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--shapes", nargs="*", default=["2000x300", "3000x96", "3000x1000", "3000x2048"], help="NxL")
    ap.add_argument("--out", default=None, help="append the lines to this file too")
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    for shape in args.shapes:
        N, L = (int(v) for v in shape.lower().split("x"))
        line = measure(N, L, args, weights)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
