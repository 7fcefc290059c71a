"""What option "search_refine" saves of a library search (option "search_structures"), on one GPU:

  * `dmp_predict_end` alone, HIP events around it, at L = 300 with a library of K entries of m rows each (the library of
    tools/time_search.py: every entry a gapped copy of a stretch of the model), "search_refine" 0 and each R of --refine in
    alternating runs of one process: the median in ms, us per entry, and the ratio to R = 0;
  * that the refined entries' tm_model are the R = 0 run's, bit for bit;
  * with --recall: a library of K = 256 at m = L made of 8 gapped copies of the model among 248 unrelated walks - how many
    of the R = 0 run's best 8 are among the entries refined at each R;
  * with --once R: one warm-up and one run at that R and nothing else, for a kernel trace of the launches
    (rocprofv3 --kernel-trace --stats -- python tools/time_search_refine.py --m 300 --entries 1024 --once 64).

    python tools/time_search_refine.py --m 150 --entries 1024 [--refine 16,64] [--repeats 5] [--precision 2] [--length 300]

One (m, K) per invocation, as tools/time_search.py.  Prints one line per R; profiles/search_refine.txt keeps a run.
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
from time_align import end_ms, gapped_copy                       # noqa: E402
from time_search import entry                                    # noqa: E402


def walk(m, seed):
    """An unrelated chain of m rows: steps of 3.8 A in random directions."""
    v = np.random.default_rng(50_000 + seed).normal(size=(m, 3))
    return np.cumsum(3.8 * v / np.linalg.norm(v, axis=1, keepdims=True), axis=0).astype(np.float32)


def recall_library(model):
    """8 gapped copies of the model at every 32nd place among 248 unrelated walks of as many rows."""
    L = len(model)
    return S.Library.from_traces([gapped_copy(model, 900 + k)[:L] if k % 32 == 5 else walk(L, k) for k in range(256)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--m", type=int, default=None)
    ap.add_argument("--entries", type=int, default=None)
    ap.add_argument("--refine", type=str, default="16,64")
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--once", type=int, default=None)
    args = ap.parse_args()
    L = args.length
    m, K = (L, 256) if args.recall else (args.m, args.entries)
    refines = [int(r) for r in args.refine.split(",")] if args.once is None else [args.once]
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    eng = Engine("cuda:0", max(L, m), 1, precision=args.precision)
    eng.set_weights(weights)
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
    conf = torch.empty((L + S.search_floats(L, K, K * m),), dtype=torch.float32, device=eng.device)
    end_ms(eng, d_msa, coords, conf)
    model = coords[:, 1].cpu().numpy()
    lib = recall_library(model) if args.recall else S.Library.from_traces([entry(model, m, k) for k in range(K)])
    assert len(lib) == K and lib.rows == K * m
    block = conf[L:]
    eng.set_option("search_max_m", m)
    eng.set_option("search_structures", K)

    def run(R):
        lib.fill_block(block, L)
        eng.set_option("search_refine", R)
        return end_ms(eng, d_msa, coords, conf)

    if args.once is not None:
        run(args.once)
        print("L=%d m=%d K=%d search_refine %d: one run after one warm-up, %.3f ms" % (L, m, K, args.once, run(args.once)), flush=True)
        eng.close()
        return 0
    settings = [0] + refines
    ts, blocks = {R: [] for R in settings}, {}
    for rep in range(args.repeats + 2):
        for R in settings:
            t = run(R)
            if rep >= 2:
                ts[R].append(t)
            blocks[R] = block.cpu().numpy().copy()
    C = eng.get_option("search_chunk_used")
    eng.set_option("search_refine", 0)
    eng.set_option("search_structures", 0)
    full = S.unpack_search(blocks[0], L, lib.lengths)
    tm_full = np.array([h["tm_model"] for h in full["hits"]], dtype=np.float32)
    base = float(np.median(ts[0]))
    print("L=%d m=%d K=%d precision %d, %d runs, chunk C %d: search_refine 0 median %.3f ms (min %.3f, max %.3f) = %.1f us per entry; "
          "best tm_model %.4f" % (L, m, K, args.precision, args.repeats, C, base, min(ts[0]), max(ts[0]), 1e3 * base / K,
                                  tm_full[full["rank"][0]]), flush=True)
    ok = True
    for R in refines:
        un = S.unpack_search(blocks[R], L, lib.lengths, refine=R)
        refined = un["refined"] if "refined" in un else np.ones(K, dtype=bool)
        tm = np.array([h["tm_model"] for h in un["hits"]], dtype=np.float32)
        same = bool(np.array_equal(tm[refined].view(np.uint32), tm_full[refined].view(np.uint32)))
        ok = ok and same and int(refined.sum()) == min(R, K)
        t = float(np.median(ts[R]))
        line = ("  search_refine %d: median %.3f ms (min %.3f, max %.3f) = %.1f us per entry; ratio to R = 0 %.3f; %d entries refined, "
                "their tm_model equal to the R = 0 run's: %s; the best entry of R = 0 is %s"
                % (R, t, min(ts[R]), max(ts[R]), 1e3 * t / K, t / base, int(refined.sum()), same,
                   "refined" if refined[full["rank"][0]] else "NOT refined"))
        if args.recall:
            line += "; of the R = 0 run's best 8, refined: %d" % int(refined[full["rank"][:8]].sum())
        print(line, flush=True)
    if args.recall:
        print("  the R = 0 run's best 8: entries %s, tm_model %s; the ninth %.4f"
              % (full["rank"][:8].tolist(), np.round(tm_full[full["rank"][:8]], 4).tolist(), tm_full[full["rank"][8]]), flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
