"""What aligning a prediction with a structure (option "align_structure") costs, on one GPU:

  * `dmp_predict_end` alone, HIP events around it, option on minus option off in alternating runs, for a one-row
    alignment at L = 96, 300, 1000 and 2048 with m = L (-n 0 -m 0: the end is the backbone builder, the fault latch and -
    with the option on - align_prep, align_thread and align_refine).

    python tools/time_align.py [--repeats 7] [--precision 2] [--lengths 96 300 1000 2048]

The structure is the model's own trace with a deleted and an inserted stretch (so m = L), 0.4 A of noise and a rigid
motion: a related structure with gaps, where the refinement needs several rounds.  Prints one line per length;
profiles/align.txt keeps a run.
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


def end_ms(eng, d_msa, coords, conf):
    """One prediction through the unit calls; returns the milliseconds dmp_predict_end's work took on the stream."""
    lib, s = eng.lib, eng.stream()
    n, L = d_msa.shape
    assert lib.dmp_predict_begin_units(eng.ctx, d_msa.data_ptr(), n, L, None, 0, 0, 0) == 0, lib.dmp_last_error()
    while lib.dmp_predict_next_unit(eng.ctx) != 0:
        assert lib.dmp_predict_issue_unit(eng.ctx, s) == 0, lib.dmp_last_error()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert lib.dmp_predict_end(eng.ctx, coords.data_ptr(), conf.data_ptr(), s) == 0, lib.dmp_last_error()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def gapped_copy(model, seed):
    """The model with L // 12 rows deleted at a third, as many foreign rows inserted at two thirds, noise, a rigid motion."""
    L = len(model)
    rng = np.random.default_rng(seed)
    g = max(4, L // 12)
    rows = model.astype(np.float64) + rng.normal(scale=0.4, size=model.shape)
    v = rng.normal(size=(g, 3))
    loop = rows[2 * L // 3] + 6.0 + np.cumsum(3.8 * v / np.linalg.norm(v, axis=1, keepdims=True), axis=0)
    rows = np.concatenate([rows[:L // 3], rows[L // 3 + g:2 * L // 3], loop, rows[2 * L // 3:]])
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    return (rows @ R.T + 7.0).astype(np.float32)


def measure(L, args, weights):
    alnmat = encode_aln(synth.synth_msa(L, 1, 1000 + L))
    eng = Engine("cuda:0", L, 1, precision=args.precision)
    eng.set_weights(weights)
    d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
    coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
    conf = torch.empty((S.Layout(L, align_m=L).total,), dtype=torch.float32, device=eng.device)
    end_ms(eng, d_msa, coords, conf)
    structure = gapped_copy(coords[:, 1].cpu().numpy(), L)
    assert structure.shape == (L, 3)
    conf[L:] = torch.from_numpy(S.pack_structure(structure, L)).to(eng.device)
    ts = {0: [], 1: []}
    for rep in range(args.repeats + 2):
        for on in (0, 1):
            eng.set_option("align_structure", on)
            t = end_ms(eng, d_msa, coords, conf)
            if rep >= 2:
                ts[on].append(t)
    eng.set_option("align_structure", 0)
    al = S.unpack_alignment(conf[L:], L)
    off, on = np.array(ts[0]), np.array(ts[1])
    print("L=%d m=%d (%d seeds) precision %d, %d runs: dmp_predict_end off median %.3f ms (min %.3f, max %.3f); on median %.3f ms "
          "(min %.3f, max %.3f); difference of medians %+.3f ms; n_ali %d tm_model %.4f rmsd_ali %.3f; device_mib %d"
          % (L, L, al["seeds"], args.precision, args.repeats, np.median(off), off.min(), off.max(), np.median(on), on.min(),
             on.max(), np.median(on) - np.median(off), al["n_ali"], al["tm_model"], al["rmsd_ali"], eng.get_option("device_mib")),
          flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--lengths", type=int, nargs="*", default=[96, 300, 1000, 2048])
    args = ap.parse_args()
    weights = {k: torch.from_numpy(np.array(v)) for k, v in synth.synth_weights(0, coord_scale=5.0).items()}
    for L in args.lengths:
        measure(L, args, weights)


if __name__ == "__main__":
    main()
