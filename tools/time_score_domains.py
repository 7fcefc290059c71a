"""What scoring every domain against the native (option "score_domains") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, with the option off and on IN THE SAME RUN: six contexts hold the same
    finished prediction - nothing on, "score_native" alone (the yardstick), "score_native" + "domains" at the defaults (the model
    stays one domain) without and with "score_domains", and the same pair forced through all four levels (tau 1, min_size 8,
    min_segment 2) - and their ends are timed in turn, for a one-row alignment at L = 96, 300, 1000 and 2048, -n 0 -m 0, with a
    whole native, so that both legs run;
  * the scratch the option allocates ("device_mib" before and after).

    python tools/time_score_domains.py [--repeats 9] [--precision 2] [--lengths 96 300 1000 2048] [--out profiles/score_domains.txt]

The trunk before the end is not timed.  The model is what the synthetic weights give, the collapsed chain profiles/exposure.txt
was measured on; the native is a folded-like chain (synth.protein_like_trace).  Prints one line per length and, with --out,
appends them to a file.  Which kernel a long run spends its time in is a question for a kernel trace of this script (one length,
few repeats), kept apart from any counter run.  Measured (profiles/score_domains.txt, MI355X, precision 2): the option costs 0.24, 0.60,
2.55 and 5.63 ms at L = 96, 300, 1000 and 2048 with the model one domain (1.9 to 2.6 times "score_native" alone), 0.20, 0.40, 1.71
and 4.46 ms forced through all four levels (1.3 to 2.1 times).
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
    # name: (score_native, domains parameters or None, score_domains)
    settings = {"off": (0, None, 0), "score": (1, None, 0), "domains": (1, DEFAULTS, 0), "domains+sd": (1, DEFAULTS, 1),
                "forced": (1, FORCED, 0), "forced+sd": (1, FORCED, 1)}
    engs, bufs, lays, mib = {}, {}, {}, {}
    for name, (score, dom, sd) in settings.items():
        eng = Engine("cuda:0", L, 1, precision=args.precision)
        eng.set_weights(weights)
        lay = S.Layout(L, score=bool(score), domains=dom is not None, score_domains=bool(sd))
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
        eng.set_option("score_native", score)
        if dom is not None:
            eng.set_domains(True, dom[0] * 1e-3, dom[1], dom[2])
        before = eng.device_bytes
        eng.set_option("score_domains", sd)                       # (the scratch is allocated here, outside the timed region)
        mib[name] = (eng.device_bytes - before) / float(1 << 20)
        run_passes(eng, d_msa, 0)
        if score:
            conf[lay.score_off:lay.mapscore_off] = torch.from_numpy(S.pack_native(folded, 0.0, L)).to(eng.device)
        engs[name], bufs[name], lays[name] = eng, (d_msa, coords, conf), lay
    ts = {k: [] for k in settings}
    for rep in range(args.repeats + 2):
        for name in settings:
            t = end_ms(engs[name], *bufs[name][1:])
            if rep >= 2:
                ts[name].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    un = {name: S.unpack_domain_scores(lays[name].domain_score_block(bufs[name][2]), L) for name in ("domains+sd", "forced+sd")}
    assert un["domains+sd"]["domains"] == 1 and len(un["forced+sd"]["legs"]) == 2

    def spread(name):
        return "%.3f ms (min %.3f, max %.3f)" % (med[name], min(ts[name]), max(ts[name]))
    score_alone = med["score"] - med["off"]
    at_defaults, forced = med["domains+sd"] - med["domains"], med["forced+sd"] - med["forced"]
    line = ("L=%d precision %d, %d runs: dmp_predict_end medians off %.3f ms, score_native %s, + domains at the defaults %.3f ms, "
            "+ score_domains %s, + domains forced %.3f ms, + score_domains %s; score_native alone costs %+.3f ms, the option %+.3f ms at "
            "the defaults (%.2f x score_native), %+.3f ms forced (%.2f x); scratch %.1f MiB; domains: defaults %d + %d, forced %d + %d; "
            "tm_domains forced %.3f / %.3f"
            % (L, args.precision, args.repeats, med["off"], spread("score"), med["domains"], spread("domains+sd"), med["forced"],
               spread("forced+sd"), score_alone, at_defaults, at_defaults / score_alone, forced, forced / score_alone, mib["forced+sd"],
               un["domains+sd"]["domains"], un["domains+sd"]["domains_native"], un["forced+sd"]["domains"],
               un["forced+sd"]["domains_native"], un["forced+sd"]["legs"][0]["tm_domains"], un["forced+sd"]["legs"][1]["tm_domains"]))
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
