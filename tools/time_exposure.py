"""What counting the solvent exposure of the final backbone (option "exposure") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, with the option off and on IN THE SAME RUN: five contexts hold the same
    finished prediction - nothing on, "score_native", "exposure", and both with a folded-like and with a collapsed native -
    and their ends are timed in turn, for a one-row alignment at L = 96, 300, 1000 and 2048, -n 0 -m 0;
  * the scratch the option allocates ("device_mib" before and after).

    python tools/time_exposure.py [--repeats 9] [--precision 2] [--lengths 96 300 1000 2048] [--out profiles/exposure.txt]

The trunk before the end is not timed.  The model's leg runs on what the synthetic weights give (the line says how buried it
is); the native's leg runs on a folded-like chain (synth.protein_like_trace: 3.8 A bonds, self-avoiding, the density of a
compact protein) and on a collapsed one (a Gaussian blob, sigma 3 A: more than a thousand candidates per atom), so the
difference to "score_native" alone is the cost of one leg on that kind of structure.  Prints one line per length and, with
--out, appends them to a file; profiles/exposure.txt keeps a run beside the figures of "assign_ss" from profiles/ss.txt.
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


def blob(L, sigma=3.0, seed=0):
    return (np.random.default_rng(seed).standard_normal((L, 3)) * sigma).astype(np.float32)


def measure(L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    natives = {"folded": synth.protein_like_trace(L, 1).astype(np.float32), "collapsed": blob(L)}
    settings = {"off": (0, 0, None), "score": (1, 0, "folded"), "exposure": (0, 1, None), "exposure+folded": (1, 1, "folded"),
                "exposure+collapsed": (1, 1, "collapsed")}
    engs, bufs, lays, mib = {}, {}, {}, {}
    for name, (score, exposure, native) in settings.items():
        eng = Engine("cuda:0", L, 1, precision=args.precision)
        eng.set_weights(weights)
        lay = S.Layout(L, score=bool(score), exposure=bool(exposure))
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
        before = eng.device_bytes
        eng.set_option("score_native", score)
        eng.set_option("exposure", exposure)                     # (the scratch is allocated here, outside the timed region)
        mib[name] = (eng.device_bytes - before) >> 20
        run_passes(eng, d_msa, 0)
        if score:
            conf[lay.score_off:lay.mapscore_off] = torch.from_numpy(S.pack_native(natives[native], 0.0, L)).to(eng.device)
        engs[name], bufs[name], lays[name] = eng, (d_msa, coords, conf), lay
    ts = {k: [] for k in settings}
    for rep in range(args.repeats + 2):
        for name in settings:
            t = end_ms(engs[name], *bufs[name][1:])
            if rep >= 2:
                ts[name].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    one = S.unpack_exposure(lays["exposure"].exposure_block(bufs["exposure"][2]), L)
    fol = S.unpack_exposure(lays["exposure+folded"].exposure_block(bufs["exposure+folded"][2]), L)
    col = S.unpack_exposure(lays["exposure+collapsed"].exposure_block(bufs["exposure+collapsed"][2]), L)
    assert np.array_equal(one["n"], fol["n"]) and np.array_equal(one["n"], col["n"]) and fol["has_native"] and col["has_native"]

    def buried(e):
        return e["buried_atoms"] / float(max(e["atoms"], 1))
    line = ("L=%d precision %d, %d runs: dmp_predict_end medians off %.3f ms, score_native %.3f ms, exposure %.3f ms (min %.3f, max "
            "%.3f), exposure + folded native %.3f ms (min %.3f, max %.3f), exposure + collapsed native %.3f ms (min %.3f, max %.3f); "
            "the model's leg costs %+.3f ms (2 launches), a folded-like native's %+.3f ms, a collapsed native's %+.3f ms (2 + the native entity's 2 launches "
            "each); scratch %d MiB; atoms without an exposed point: model %.2f, folded %.2f, collapsed %.2f; area model %.0f, folded "
            "%.0f, collapsed %.0f A^2"
            % (L, args.precision, args.repeats, med["off"], med["score"], med["exposure"], min(ts["exposure"]), max(ts["exposure"]),
               med["exposure+folded"], min(ts["exposure+folded"]), max(ts["exposure+folded"]), med["exposure+collapsed"],
               min(ts["exposure+collapsed"]), max(ts["exposure+collapsed"]), med["exposure"] - med["off"],
               med["exposure+folded"] - med["score"] - (med["exposure"] - med["off"]),
               med["exposure+collapsed"] - med["score"] - (med["exposure"] - med["off"]), mib["exposure"], buried(one),
               buried(fol["native"]), buried(col["native"]), one["area"], fol["native"]["area"], col["native"]["area"]))
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
