"""What splitting the final C-alpha trace into structural domains (option "domains") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, with the option off and on IN THE SAME RUN: six contexts hold the same
    finished prediction - nothing on, "exposure" and "align_structure" (the yardsticks: the other tail options on the same
    model), "domains" at the defaults, "domains" forced (tau 1, min_size 8, min_segment 2: every admissible cut is accepted,
    so all four levels run on sixteen domains), and "domains" forced with "score_native" and a whole native (both legs) -
    and their ends are timed in turn, for a one-row alignment at L = 96, 300, 1000 and 2048, -n 0 -m 0;
  * the scratch the option allocates ("device_mib" before and after).

    python tools/time_domains.py [--repeats 9] [--precision 2] [--lengths 96 300 1000 2048] [--out profiles/domains.txt]

The trunk before the end is not timed.  The model is what the synthetic weights give, the collapsed chain profiles/exposure.txt
was measured on; the native of the two-leg run and the structure of "align_structure" are a folded-like chain
(synth.protein_like_trace).  Prints one line per length and, with --out, appends them to a file.  Which kernel a long run spends
its time in is a question for a kernel trace of this script (one length, few repeats), kept apart from any counter run.
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

FORCED = (1000, 8, 2)
DEFAULTS = (250, 40, 10)


def measure(L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    folded = synth.protein_like_trace(L, 1).astype(np.float32)
    # name: (score_native, exposure, align_structure, domains parameters or None)
    settings = {"off": (0, 0, 0, None), "exposure": (0, 1, 0, None), "align": (0, 0, 1, None), "domains": (0, 0, 0, DEFAULTS),
                "forced": (0, 0, 0, FORCED), "score": (1, 0, 0, None), "forced+native": (1, 0, 0, FORCED)}
    engs, bufs, lays, mib = {}, {}, {}, {}
    for name, (score, exposure, align, dom) in settings.items():
        eng = Engine("cuda:0", L, 1, precision=args.precision)
        eng.set_weights(weights)
        lay = S.Layout(L, score=bool(score), exposure=bool(exposure), align_m=L if align else None, domains=dom is not None)
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
        eng.set_option("score_native", score)
        eng.set_option("exposure", exposure)
        eng.set_option("align_structure", align)
        before = eng.device_bytes
        if dom is not None:
            eng.set_domains(True, dom[0] * 1e-3, dom[1], dom[2])  # (the scratch is allocated here, outside the timed region)
        mib[name] = (eng.device_bytes - before) / float(1 << 20)
        run_passes(eng, d_msa, 0)
        if score:
            conf[lay.score_off:lay.mapscore_off] = torch.from_numpy(S.pack_native(folded, 0.0, L)).to(eng.device)
        if align:
            conf[lay.align_off:lay.align_end] = torch.from_numpy(S.pack_structure(folded, L)).to(eng.device)
        engs[name], bufs[name], lays[name] = eng, (d_msa, coords, conf), lay
    ts = {k: [] for k in settings}
    for rep in range(args.repeats + 2):
        for name in settings:
            t = end_ms(engs[name], *bufs[name][1:])
            if rep >= 2:
                ts[name].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    parse = {name: S.unpack_domains(lays[name].domains_block(bufs[name][2]), L) for name in ("domains", "forced", "forced+native")}
    assert np.array_equal(parse["forced"]["labels"], parse["forced+native"]["labels"]) and parse["forced+native"]["has_native"]

    def spread(name):
        return "%.3f ms (min %.3f, max %.3f)" % (med[name], min(ts[name]), max(ts[name]))
    line = ("L=%d precision %d, %d runs: dmp_predict_end medians off %.3f ms, exposure %.3f ms, align_structure %.3f ms, domains at the "
            "defaults %s, forced %s, score_native %.3f ms, forced with a native's leg %s; the option costs %+.3f ms at the defaults, "
            "%+.3f ms forced, a native's leg %+.3f ms more (24 launches each way, and the native entity's one in front with the native); scratch %.1f MiB; domains: defaults %d, forced %d "
            "(depth %d, %d discontinuous), the forced native %d; contact pairs %d"
            % (L, args.precision, args.repeats, med["off"], med["exposure"], med["align"], spread("domains"), spread("forced"),
               med["score"], spread("forced+native"), med["domains"] - med["off"], med["forced"] - med["off"],
               med["forced+native"] - med["score"] - (med["forced"] - med["off"]), mib["forced"], parse["domains"]["domains"],
               parse["forced"]["domains"], parse["forced"]["depth"], parse["forced"]["discontinuous"],
               parse["forced+native"]["native"]["domains"], parse["forced"]["contacts"]))
    print(line, flush=True)
    for eng in engs.values():
        eng.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--lengths", nargs="*", type=int, default=[96, 300, 1000, 2048])
    ap.add_argument("--out", default=None, help="append the lines to this file too")
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    for L in args.lengths:
        line = measure(L, args, weights)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
