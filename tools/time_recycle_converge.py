"""What the convergence stop (option "recycle_tol_mA") costs and saves, on one GPU:

  * cost of having it on without triggering: the reference's example alignment (PF10963, L = 82, -n 10 -m 0) with a
    tolerance nothing meets (1 mA) against the option off, alternating runs;
  * gain: the L = 500 fixture of BASELINE configs[2] (3000 rows, -n 30 -m 200) plain and at 180 mA.

    python tools/time_recycle_converge.py [--repeats 15] [--precision 2]

Prints one line per measurement (host wall time of predict + synchronise, ms); profiles/recycle_converge.txt keeps a run.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dmpfold2_amd import synth                                   # noqa: E402
from dmpfold2_amd.predict import Engine, encode_aln              # noqa: E402


def golden(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return {k: g[k] for k in g.files}


def timed(eng, alnmat, n, m, converge):
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.predict_device(d_msa, None, n, m, converge=converge)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, eng.passes_run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--skip-l500", action="store_true")
    args = ap.parse_args()

    g = golden("pf10963_n10_m0")
    eng = Engine("cuda:0", 82, g["alnmat"].shape[0], precision=args.precision)
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()})
    for _ in range(3):
        timed(eng, g["alnmat"], 10, 0, None)
        timed(eng, g["alnmat"], 10, 0, 0.001)
    off, on = [], []
    for _ in range(args.repeats):
        off.append(timed(eng, g["alnmat"], 10, 0, None)[0])
        t, passes = timed(eng, g["alnmat"], 10, 0, 0.001)
        assert passes == 11
        on.append(t)
    off, on = np.array(off), np.array(on)
    print("pf10963 L=82 -n 10 -m 0 precision %d, %d alternating runs: off median %.3f ms (min %.3f, max %.3f); "
          "tol 1 mA (never met, 11 passes) median %.3f ms (min %.3f, max %.3f); difference of medians %+.3f ms = %+.2f %% "
          "(%.1f us per pass boundary)" % (args.precision, args.repeats, np.median(off), off.min(), off.max(), np.median(on),
                                           on.min(), on.max(), np.median(on) - np.median(off),
                                           100.0 * (np.median(on) - np.median(off)) / np.median(off),
                                           1e3 * (np.median(on) - np.median(off)) / 10.0), flush=True)
    eng.close()
    if args.skip_l500:
        return
    g = golden("fit_L500_N5000_n30_m200")
    sd = synth.headline_fixture_weights(g["coord_fc"], float(g["coord_gru_mds_scale"]), seed=int(g["weights_seed"]))
    alnmat = encode_aln(synth.synth_msa(500, int(g["msa_rows"]), int(g["msa_seed"])))
    eng = Engine("cuda:0", 500, alnmat.shape[0], precision=args.precision)
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    timed(eng, alnmat, 30, 200, None)
    plain = [timed(eng, alnmat, 30, 200, None) for _ in range(3)]
    conv = [timed(eng, alnmat, 30, 200, 0.18) for _ in range(3)]
    tp, tc = np.median([t for t, _ in plain]), np.median([t for t, _ in conv])
    print("fit_L500 (3000 x 500) -n 30 -m 200 precision %d, median of 3: plain %.1f ms (%d passes); at 180 mA %.1f ms "
          "(%d passes); ratio %.3f (passes %d -> %d = %.3f)" % (args.precision, tp, plain[0][1], tc, conv[0][1], tc / tp,
                                                                 plain[0][1], conv[0][1], conv[0][1] / plain[0][1]), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
