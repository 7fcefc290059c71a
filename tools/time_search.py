"""What searching a library of structures with a prediction (option "search_structures") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, at L = 300 with a library of K entries of m rows each: option on minus
    option off in alternating runs (-n 0 -m 0: the end is the backbone builder, the fault latch and - with the option on -
    search_prep, the three align kernels per chunk and search_rank);
  * in the same run, the same K entries one at a time: K calls of `dmp_predict_end` with option "align_structure", summed;
  * the chunk size C the library chose and the resident align_refine workgroups per CU for the shape.

    python tools/time_search.py --m 150 --entries 256 [--repeats 5] [--precision 2] [--length 300]

One (m, K) per invocation, so that a job can run each size under its own time limit and stop at the first that fails:

    for m in 150 300; do for K in 1 16 256 1024; do
        timeout -k 10 300 python tools/time_search.py --m $m --entries $K || break 2; done; done

Every entry is a stretch of m rows of the model's own trace (extended by a foreign loop where m rows are not there) with a
deleted and an inserted stretch, 0.4 A of noise and a rigid motion, each with its own seed.  Prints one line;
profiles/search.txt keeps a run.
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


def entry(model, m, seed):
    """A related structure of exactly m rows: gapped_copy of a window of the model."""
    L = len(model)
    rng = np.random.default_rng(10_000 + seed)
    a = int(rng.integers(0, L - m + 1)) if m < L else 0
    out = gapped_copy(model[a:a + m], seed)
    assert out.shape == (m, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--m", type=int, required=True)
    ap.add_argument("--entries", type=int, required=True)
    args = ap.parse_args()
    L, m, K = args.length, args.m, args.entries
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    eng = Engine("cuda:0", max(L, m), 1, precision=args.precision)
    eng.set_weights(weights)
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
    floats = L + max(S.search_floats(L, K, K * m), S.align_floats(L, m))
    conf = torch.empty((floats,), dtype=torch.float32, device=eng.device)
    end_ms(eng, d_msa, coords, conf)
    model = coords[:, 1].cpu().numpy()
    lib = S.Library.from_traces([entry(model, m, k) for k in range(K)])
    # one at a time: K calls with "align_structure", each with its own block in place before the clock starts
    eng.set_option("align_structure", 1)
    blocks = [torch.from_numpy(S.pack_structure(lib.entry(k), L)).to(eng.device) for k in range(K)]
    single, tm_single = [], []
    for rep in range(2):
        single = []
        for k in range(K):
            conf[L:L + blocks[k].shape[0]] = blocks[k]
            single.append(end_ms(eng, d_msa, coords, conf))
            if rep == 1:
                tm_single.append(float(conf[L + 3]))
    eng.set_option("align_structure", 0)
    del blocks
    # the batch
    block = conf[L:L + S.search_floats(L, K, lib.rows)]
    eng.set_option("search_max_m", m)
    ts = {0: [], 1: []}
    for rep in range(args.repeats + 2):
        for on in (0, 1):
            lib.fill_block(block, L)
            eng.set_option("search_structures", K if on else 0)
            t = end_ms(eng, d_msa, coords, conf)
            if rep >= 2:
                ts[on].append(t)
    un = S.unpack_search(block, L, lib.lengths)
    same = [np.float32(h["tm_model"]) for h in un["hits"]] == [np.float32(v) for v in tm_single]
    C, wg = eng.get_option("search_chunk_used"), eng.get_option("search_wg_per_cu")
    mib = eng.get_option("device_mib")
    eng.set_option("search_structures", 0)
    off, on = np.array(ts[0]), np.array(ts[1])
    diff = float(np.median(on) - np.median(off))
    one = float(np.sum(single))
    print("L=%d m=%d K=%d precision %d, %d runs: dmp_predict_end off median %.3f ms; search on median %.3f ms (min %.3f, max %.3f); "
          "difference %+.3f ms = %.1f us per entry; one at a time (K calls, align_structure) %.3f ms = %.1f us per entry; ratio %.1f; "
          "chunk C %d (%d launches of each align kernel), align_refine workgroups per CU %d; tm_model equal to one at a time: %s; "
          "best tm_model %.4f; device_mib %d"
          % (L, m, K, args.precision, args.repeats, np.median(off), np.median(on), on.min(), on.max(), diff, 1e3 * diff / K, one,
             1e3 * one / K, one / diff, C, -(-K // C), wg, same, un["hits"][int(un["rank"][0])]["tm_model"], mib), flush=True)
    eng.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
