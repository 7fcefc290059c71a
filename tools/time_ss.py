"""What assigning secondary structure to the final backbone (option "assign_ss") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, with the option off and on in the same process (four contexts that hold
    the same finished prediction: nothing on, "score_native", "assign_ss", both - the last one runs the native's leg too),
    timed in turn, for a one-row alignment at L = 96, 300, 1000 and 2048, -n 0 -m 0;
  * the launches the option adds and the scratch it allocates ("device_mib" before and after).

    python tools/time_ss.py [--repeats 9] [--precision 2] [--lengths 96 300 1000 2048]

The trunk before the end is not timed.  The model is the synthetic weights' (a collapsed chain: hydrogen bonds by the
hundred thousand at L = 2048, the dense end of what ss_assign can meet); the native is an ideal alpha helix of length L.
Prints one line per length; profiles/ss.txt keeps a run.
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


def ideal_helix(L, radius=2.3, turn=100.0, rise=1.5):
    k = np.arange(L)
    a = np.deg2rad(turn) * k
    return np.stack([radius * np.cos(a), radius * np.sin(a), rise * k], axis=1).astype(np.float32)


def measure(L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    settings = {"off": (0, 0), "score": (1, 0), "ss": (0, 1), "ss+native": (1, 1)}
    native = torch.from_numpy(S.pack_native(ideal_helix(L), 0.0, L))
    engs, bufs, lays, mib = {}, {}, {}, {}
    for name, (score, ss) in settings.items():
        eng = Engine("cuda:0", L, 1, precision=args.precision)
        eng.set_weights(weights)
        lay = S.Layout(L, score=bool(score), ss=bool(ss))
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
        before = eng.device_bytes
        eng.set_option("score_native", score)
        eng.set_option("assign_ss", ss)                          # (the scratch is allocated here, outside the timed region)
        mib[name] = (eng.device_bytes - before) >> 20
        run_passes(eng, d_msa, 0)
        if score:
            conf[lay.score_off:lay.mapscore_off] = native.to(eng.device)
        engs[name], bufs[name], lays[name] = eng, (d_msa, coords, conf), lay
    ts = {k: [] for k in settings}
    for rep in range(args.repeats + 2):
        for name in settings:
            t = end_ms(engs[name], *bufs[name][1:])
            if rep >= 2:
                ts[name].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    one = S.unpack_ss(lays["ss"].ss_block(bufs["ss"][2]), L)
    two = S.unpack_ss(lays["ss+native"].ss_block(bufs["ss+native"][2]), L)
    assert one["ss8"] == two["ss8"] and two["has_native"]
    print("L=%d precision %d, %d runs: dmp_predict_end medians off %.3f ms, score_native %.3f ms, assign_ss %.3f ms (min %.3f, "
          "max %.3f), both %.3f ms (min %.3f, max %.3f); the model's leg costs %+.3f ms (3 launches), with the native's %+.3f ms "
          "(5 launches, two of them the native entity's); score_native alone costs %+.3f ms; scratch %d MiB; n_hb %d, helix %.2f strand %.2f, native helix %.2f"
          % (L, args.precision, args.repeats, med["off"], med["score"], med["ss"], min(ts["ss"]), max(ts["ss"]), med["ss+native"],
             min(ts["ss+native"]), max(ts["ss+native"]), med["ss"] - med["off"], med["ss+native"] - med["score"],
             med["score"] - med["off"], mib["ss"], one["n_hb"], one["helix"], one["strand"],
             sum(two["counts_native"][c] for c in "HGI") / float(L)), flush=True)
    for eng in engs.values():
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--lengths", nargs="*", type=int, default=[96, 300, 1000, 2048])
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    for L in args.lengths:
        measure(L, args, weights)


if __name__ == "__main__":
    main()
