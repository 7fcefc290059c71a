"""What the Gaussian network model of the final C-alpha trace (option "flex") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, with the option off and on IN THE SAME RUN: four contexts hold the same
    finished prediction - nothing on, "flex" (the model's leg), "score_native" with a whole native (the yardstick of the
    two-leg run), and "flex" with "score_native" and that native (both legs) - and their ends are timed in turn, for a one-row
    alignment at L = 96, 300, 1000 and 2048, -n 0 -m 0;
  * beside it one `dmp_eigh_top8` of the same order, on the matrix sigma I - Gamma of the native: a leg is that solve with
    another epilogue plus the three small kernels around it;
  * the scratch the option allocates ("device_mib" before and after).

    python tools/time_flex.py [--repeats 9] [--precision 2] [--lengths 96 300 1000 2048] [--out profiles/flex.txt]

The trunk before the end is not timed.  The model is what the synthetic weights give, the collapsed chain profiles/exposure.txt
was measured on - a nearly complete contact graph; the native is a folded-like chain (synth.protein_like_trace).  Prints one
line per length and, with --out, appends them to a file.
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


def shifted_kirchhoff(ca, cutoff):
    """sigma I - Gamma of a trace as the option forms it, float32 (L, L)."""
    x = np.asarray(ca, dtype=np.float32).astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    a = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] < cutoff * cutoff) & ~np.eye(len(x), dtype=bool)
    deg = a.sum(1)
    return (a + np.diag(2 * deg.max() - deg)).astype(np.float32)


def eigh_ms(eng, M):
    """One dmp_eigh_top8 of the matrix M on the engine's stream -> milliseconds."""
    L = M.shape[0]
    out = torch.empty((L, 8), dtype=torch.float32, device=eng.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert eng.lib.dmp_eigh_top8(eng.ctx, M.data_ptr(), L, out.data_ptr(), eng.stream()) == 0, eng.lib.dmp_last_error()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    folded = synth.protein_like_trace(L, 1).astype(np.float32)
    # name: (score_native, flex)
    settings = {"off": (0, 0), "flex": (0, 1), "score": (1, 0), "flex+native": (1, 1)}
    engs, bufs, lays, mib = {}, {}, {}, {}
    for name, (score, flex) in settings.items():
        eng = Engine("cuda:0", L, 1, precision=args.precision)
        eng.set_weights(weights)
        lay = S.Layout(L, score=bool(score), flex=bool(flex))
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        conf = torch.empty((lay.total,), dtype=torch.float32, device=eng.device)
        eng.set_option("score_native", score)
        before = eng.device_bytes
        if flex:
            eng.set_flex(True, args.cutoff)                       # (the scratch is allocated here, outside the timed region)
        mib[name] = (eng.device_bytes - before) / float(1 << 20)
        run_passes(eng, d_msa, 0)
        if score:
            conf[lay.score_off:lay.mapscore_off] = torch.from_numpy(S.pack_native(folded, 0.0, L)).to(eng.device)
        engs[name], bufs[name], lays[name] = eng, (d_msa, coords, conf), lay
    M = torch.from_numpy(shifted_kirchhoff(folded, args.cutoff)).to(engs["off"].device)
    ts = {k: [] for k in list(settings) + ["eigh"]}
    for rep in range(args.repeats + 2):
        for name in settings:
            t = end_ms(engs[name], *bufs[name][1:])
            if rep >= 2:
                ts[name].append(t)
        t = eigh_ms(engs["off"], M)
        if rep >= 2:
            ts["eigh"].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    one = S.unpack_flex(lays["flex"].flex_block(bufs["flex"][2]), L)
    two = S.unpack_flex(lays["flex+native"].flex_block(bufs["flex+native"][2]), L)
    assert not one["has_native"] and two["has_native"] and np.array_equal(one["modes"], two["modes"])

    def spread(name):
        return "%.3f ms (min %.3f, max %.3f)" % (med[name], min(ts[name]), max(ts[name]))
    nat = two["native"]
    line = ("L=%d precision %d, cutoff %.1f A, %d runs: dmp_predict_end medians off %.3f ms, flex (the model's leg) %s, score_native %.3f ms, "
            "flex with a native's leg %s; the model's leg costs %+.3f ms, the native's %+.3f ms more; one dmp_eigh_top8 of that order "
            "(the native's matrix) %s: the native's leg is %.2f of it; scratch %.1f MiB; model: %d contacts, sigma %d, components %d, "
            "lambda_1 %.4g; native: %d contacts, sigma %d, components %d, lambda_1 %.4g, %d hinges, r_msf %.3f, rmsip %.3f"
            % (L, args.precision, args.cutoff, args.repeats, med["off"], spread("flex"), med["score"], spread("flex+native"),
               med["flex"] - med["off"], med["flex+native"] - med["score"] - (med["flex"] - med["off"]), spread("eigh"),
               (med["flex+native"] - med["score"] - (med["flex"] - med["off"])) / med["eigh"], mib["flex"],
               one["contacts"], one["sigma"], one["components"], one["eigenvalues"][min(one["components"], 7)],
               nat["contacts"], nat["sigma"], nat["components"], nat["eigenvalues"][min(nat["components"], 7)], len(nat["hinges"]),
               two["r_msf"], two["rmsip"]))
    print(line, flush=True)
    for eng in engs.values():
        eng.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--cutoff", type=float, default=7.3)
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
