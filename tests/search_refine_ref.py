"""Option "search_refine" restated in NumPy: the screen - stage 1 of the definition in include/dmpfold_hip.h with stage 2 left
out - from the pieces of tests/test_align_cpu.py, and the library of 16 entries that the CPU and the GPU tests share.

A screened entry is the best gapless threading A* (largest tm by the stage-1 normalisation, ties to the lower seed number)
with the final formulae applied to it: tm_model = superpose(A*, d0(n), n), tm_struct, R, t = superpose(A*, d0(m), m).
"""
import numpy as np

from test_align_cpu import _Margin, _dev, _packed, d0_of, indel_copy, moved, random_walk, superpose, yardstick

RELATED = (0, 1, 2, 3)               # the entries of `library_traces` made from the model
SCREEN_GAP = 0.05                    # the fourth and the fifth screened tm_model lie at least this far apart


def screen_yardstick(model, structure):
    """The screen on float32 traces (n, 3) and (m, 3), in float64 -> (dict in the shape of `yardstick`'s, margin)."""
    P = np.asarray(model, dtype=np.float32).astype(np.float64)
    Q = np.asarray(structure, dtype=np.float32).astype(np.float64)
    n, m = len(P), len(Q)
    mg = _Margin()
    lmin = min(n, m)
    d0s = d0_of(lmin)
    d_cut = min(max(d0s, 4.5), 8.0)
    minov = max(lmin // 2, min(5, lmin))
    offsets = list(range(-(n - minov), m - minov + 1))

    def seed_pairs(k):
        i0 = max(0, -k)
        return [(i, i + k) for i in range(i0, min(n, m - k))]
    tms = np.array([superpose(*_packed(P, Q, seed_pairs(k)), d0s, lmin, d_cut, mg)[0] for k in offsets])
    order = sorted(range(len(offsets)), key=lambda s: (-tms[s], s))
    mg.gaps([tms[order[0]] - tms[s] for s in order[1:]])             # the best seed against every other
    A = seed_pairs(offsets[order[0]])
    PA, QA = _packed(P, Q, A)
    tm_model, _, _, rmsd = superpose(PA, QA, d0_of(n), n, d_cut, mg)
    tm_struct, R, t, _ = superpose(PA, QA, d0_of(m), m, d_cut, mg)
    ali = np.full(n, -1, dtype=np.int64)
    dev = np.full(n, np.nan)
    ii = np.array([a[0] for a in A])
    ali[ii] = [a[1] for a in A]
    dev[ii] = _dev(R, t, PA, QA)
    out = {"n_ali": len(A), "rmsd_ali": rmsd, "tm_model": tm_model, "tm_struct": tm_struct, "d0_model": d0_of(n),
           "d0_struct": d0_of(m), "seed_offset": offsets[order[0]], "seeds": len(offsets), "R": R, "t": t, "ali": ali,
           "deviation": dev}
    return out, mg.value


def library_traces(model, cap=None):
    """The 16 entries for a model trace of L rows: four made from the model (RELATED) - a rigid copy and three indel copies
    of L, L + 5 and max(L - 3, 3) rows - then 12 unrelated walks of L - 3 .. L + 3 rows.  `cap`: no entry longer than this
    (an engine's capacity)."""
    L = len(model)
    longer = L + 5 if cap is None else min(L + 5, cap)
    traces = [moved(model, 9)[2], indel_copy(model, 100 + L)[0], indel_copy(model, 200 + L, m=longer)[0],
              indel_copy(model, 300 + L, m=max(L - 3, 3))[0]]
    for s in range(12):
        m = L + s % 7 - 3
        traces.append(random_walk(m if cap is None else min(m, cap), 1000 + s))
    return traces


def input_condition(model, traces, full=False, screened=None):
    """The condition on the inputs of the selection tests -> (screened tm_model (K,), margins (K,), problems: a list of
    strings, empty if the condition holds).  The RELATED entries must be the best by the screen (and, with `full`, by the
    whole definition too), and the last of them at least SCREEN_GAP above the best of the others.  `screened`: what
    screen_yardstick gave for every trace, if the caller has it."""
    screened = [screen_yardstick(model, t) for t in traces] if screened is None else screened
    tm = np.array([s[0]["tm_model"] for s in screened])
    margins = np.array([s[1] for s in screened])
    rest = [k for k in range(len(traces)) if k not in RELATED]
    problems = []
    if not tm[list(RELATED)].min() - tm[rest].max() >= SCREEN_GAP:
        problems.append(f"screen: related {tm[list(RELATED)].min():.4f} against unrelated {tm[rest].max():.4f}")
    if full:
        whole = np.array([yardstick(model, t)[0]["tm_model"] for t in traces])
        if not whole[list(RELATED)].min() > whole[rest].max():
            problems.append(f"full: related {whole[list(RELATED)].min():.4f} against unrelated {whole[rest].max():.4f}")
    return tm, margins, problems
