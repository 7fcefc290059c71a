"""What option "search_domains" costs beside a library search (option "search_structures"), on one GPU:

  * `dmp_predict_end` alone, HIP events around it, at L = 300 with a library of K entries of m rows each (the library of
    tools/time_search.py: every entry a gapped copy of a stretch of the model), in alternating runs of one process:
    "search_structures" alone; with "domains" beside it; with "domains" and "search_domains" - the medians in ms, the sweep's
    cost (the third less the second) as a multiple of the whole search's, and the chunk count;
  * per model: `whole` - the default parse, which leaves the collapsed model of the synthetic weights in one piece: the
    one-domain shortcut, whose expectation is a copy's cost - and the parse pushed by its parameters, as profiles/domains.txt
    forces its levels (tau 1: every admissible cut is accepted): min_size L / 2, L / 4 and 8 - Dmax = 2, 4 and 16;
  * "search_refine" 0 and each R of --refine;
  * with --once MODEL: one warm-up and one run with the sweep on and nothing else, for a kernel trace of the launches
    (rocprofv3 --kernel-trace --stats -- python tools/time_search_domains.py --m 300 --entries 256 --once dmax).

    python tools/time_search_domains.py [--m 300,150] [--entries 16,256,1024] [--refine 0,64] [--repeats 5] [--length 300]

Prints one line per (m, K, R, model); profiles/search_domains.txt keeps a run.
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
from time_align import end_ms                                    # noqa: E402
from time_search import entry                                    # noqa: E402


def models(L):
    """name -> (tau_milli, min_size, min_segment) of the parse."""
    return {"whole": (250, 40, 10), "dmax2": (1000, L // 2, 2), "dmax4": (1000, L // 4, 2), "dmax": (1000, 8, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--m", type=str, default="300,150")
    ap.add_argument("--entries", type=str, default="16,256,1024")
    ap.add_argument("--refine", type=str, default="0,64")
    ap.add_argument("--models", type=str, default="whole,dmax2,dmax4,dmax")
    ap.add_argument("--once", type=str, default=None)
    args = ap.parse_args()
    L = args.length
    ms, Ks, Rs = ([int(v) for v in text.split(",")] for text in (args.m, args.entries, args.refine))
    names = [args.once] if args.once else args.models.split(",")
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    eng = Engine("cuda:0", max([L] + ms), 1, precision=args.precision)
    eng.set_weights(weights)
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
    plain = torch.empty((L,), dtype=torch.float32, device=eng.device)
    end_ms(eng, d_msa, coords, plain)
    model = coords[:, 1].cpu().numpy()
    base_mib = eng.get_option("device_mib")
    ok = True
    for m in ms:
        for K in Ks:
            lib = S.Library.from_traces([entry(model, m, k) for k in range(K)])
            lays = {"search": S.Layout(L, search=(K, K * m)), "domains": S.Layout(L, search=(K, K * m), domains=True),
                    "sweep": S.Layout(L, search=(K, K * m), domains=True, search_domains=True)}
            bufs = {k: torch.empty((lay.total,), dtype=torch.float32, device=eng.device) for k, lay in lays.items()}
            eng.set_option("search_max_m", m)
            eng.set_option("search_structures", K)

            def run(what, R, parse):
                lay, buf = lays[what], bufs[what]
                lib.fill_block(buf[lay.search_off:lay.search_end], L)
                for name, value in zip(("domains_tau_milli", "domains_min_size", "domains_min_segment"), parse):
                    eng.set_option(name, value)
                eng.set_option("search_refine", R)
                eng.set_option("domains", int(what != "search"))
                eng.set_option("search_domains", int(what == "sweep"))
                return end_ms(eng, d_msa, coords, buf)

            for R in Rs:
                if R >= K:
                    continue
                for name in names:
                    parse = models(L)[name]
                    if args.once:
                        run("sweep", R, parse)
                        print("L=%d m=%d K=%d search_refine %d model %s: one run after one warm-up, %.3f ms"
                              % (L, m, K, R, name, run("sweep", R, parse)), flush=True)
                        continue
                    ts = {what: [] for what in lays}
                    for rep in range(args.repeats + 2):
                        for what in lays:
                            t = run(what, R, parse)
                            if rep >= 2:
                                ts[what].append(t)
                    med = {what: float(np.median(v)) for what, v in ts.items()}
                    dom = S.unpack_domains(lays["sweep"].domains_block(bufs["sweep"]), L)
                    ds = S.unpack_domain_search(lays["sweep"].domain_search_block(bufs["sweep"]), L, K, refine=R)
                    whole = S.unpack_search(bufs["search"][lays["search"].search_off:lays["search"].search_end], L, lib.lengths, refine=R)
                    D, C = dom["domains"], eng.get_option("search_chunk_used")
                    dmax = max(1, min(16, L // parse[1]))
                    per = R if R else K
                    if D == 1:                                   # the shortcut: row 0 is the whole search's ranking
                        ok = ok and ds["domains"] == 1 and ds["rank"][0].tolist() == whole["rank"].tolist()
                    else:
                        ok = ok and ds["domains"] == D and not np.isnan(ds["headers"][:D, :, 2]).any()
                    sweep = med["sweep"] - med["domains"]
                    print("L=%d m=%d K=%d search_refine %d model %s (tau_milli %d, min_size %d): D %d of Dmax %d, sizes %s; search alone median "
                          "%.3f ms (min %.3f, max %.3f), with domains %.3f ms, with the sweep %.3f ms (min %.3f, max %.3f): the sweep costs "
                          "%+.3f ms = %.2f times the whole search; chunk C %d: %d chunks of the whole search, %d of the sweep's %d virtual "
                          "entries (%d of them of domains d >= D); best tm per domain %s"
                          % (L, m, K, R, name, parse[0], parse[1], D, dmax, [row["size"] for row in dom["table"]], med["search"],
                             min(ts["search"]), max(ts["search"]), med["domains"], med["sweep"], min(ts["sweep"]), max(ts["sweep"]), sweep,
                             sweep / med["search"], C, (-(-K // C) if R else 0) + -(-per // C),
                             (-(-(dmax * K) // C) if R else 0) + -(-(dmax * per) // C), dmax * per, (dmax - D) * per,
                             np.round([ds["hits"][d][ds["rank"][d][0]]["tm_model"] for d in range(ds["domains"])], 3).tolist()), flush=True)
            eng.set_option("search_domains", 0)
            eng.set_option("domains", 0)
            eng.set_option("search_refine", 0)
            eng.set_option("search_structures", 0)
            del bufs
    print("device_mib: %d without, %d with the scratches of the search, the domains and the sweep" % (base_mib, eng.get_option("device_mib")), flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
