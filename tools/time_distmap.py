"""What returning the chosen pass's distance map (option "emit_distmap") costs, on one GPU:

  * one target at L = 300, N = 2000, -n 10 -m 100 (the flagship workload of bench.py), option off against option on,
    alternating runs;
  * the same at L = 1000, N = 2000, -n 1 -m 0, where the map is 4 MB.

    python tools/time_distmap.py [--repeats 15] [--precision 2] [--skip-l1000] [--off-only] [--once]

Prints one line per measurement (host wall time of predict + synchronise, ms); profiles/distmap.txt keeps a run.
`--off-only` measures the option-off runs alone (a build without the option: the parent of the change, for the
comparison "off on this build against the build before it").  `--once` makes one prediction per size with the option
on and nothing else - the run to put under `rocprofv3 --kernel-trace --stats` for the kernel times of keep_best_dm_kernel
and emit_distmap_kernel.
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


def timed(eng, d_msa, n, m, on):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.predict_device(d_msa, None, n, m, distmap=True) if on else eng.predict_device(d_msa, None, n, m)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(L, N, n, m, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, N, 0))
    eng = Engine("cuda:0", L, N, precision=args.precision)
    eng.set_weights(weights)
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    tag = "L=%d N=%d -n %d -m %d precision %d" % (L, N, n, m, args.precision)
    if args.once:
        t, out = timed(eng, d_msa, n, m, True)
        print("%s: one run with the option on, %.2f ms; info = %s" % (tag, t, out[3].tolist()), flush=True)
        eng.close()
        return
    modes = (False,) if args.off_only else (False, True)
    for _ in range(3):
        for on in modes:
            timed(eng, d_msa, n, m, on)
    ts = {on: [] for on in modes}
    ref = None
    for _ in range(args.repeats):
        for on in modes:
            t, out = timed(eng, d_msa, n, m, on)
            ts[on].append(t)
            if ref is None:
                ref = (out[0].clone(), out[1].clone())
            assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])      # on or off: the same structure
    off = np.array(ts[False])
    line = "%s, %d runs: off median %.3f ms (min %.3f, max %.3f)" % (tag, args.repeats, np.median(off), off.min(), off.max())
    if not args.off_only:
        on = np.array(ts[True])
        d = np.median(on) - np.median(off)
        line += ("; on median %.3f ms (min %.3f, max %.3f); difference of medians %+.3f ms = %+.2f %% (%.1f us per pass)"
                 % (np.median(on), on.min(), on.max(), d, 100.0 * d / np.median(off), 1e3 * d / (n + 1)))
    print(line, flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--skip-l1000", action="store_true")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    measure(300, 2000, 10, 100, args, weights)
    if not args.skip_l1000:
        measure(1000, 2000, 1, 0, args, weights)


if __name__ == "__main__":
    main()
