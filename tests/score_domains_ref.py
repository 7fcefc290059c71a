"""Option "score_domains" restated in NumPy (include/dmpfold_hip.h has the definition).

Row (leg, d) is what "score_native" returns for the same model trace and a native in which every row outside P(leg, d) - the
residues that carry label d in that leg and have a native row - is NaN, with lnorm 0: `masked` makes that native,
test_score_cpu.yardstick (float64) scores it, and `leg` scatters the per-residue arrays back to the residues.  The counts the
masked call cannot give - the ordered pairs (i, j), i in the domain, j present and outside it, native distance below 15 A, and
the thresholds 0.5, 1, 2, 4 A they preserve - are plain integer loops over float64 distances formed as the library forms them.
"""
import numpy as np

from dmpfold2_amd import score as S
from test_score_cpu import _pairdist, yardstick

RADIUS = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def masked(native, labels, d):
    """The native with every row outside domain d NaN (float32 (L, 3))."""
    out = np.asarray(native, dtype=np.float32).copy()
    out[np.asarray(labels) != d] = np.nan
    return out


def pair_counts(model, native, labels, d):
    """(preserved, pairs inside the domain, outer_preserved, outer_pairs, margin) of domain d: integer loops over the ordered
    pairs of present rows; `margin` is the smallest distance of a compared value from its cutoff."""
    model, native = np.asarray(model, dtype=np.float32), np.asarray(native, dtype=np.float32)
    labels = np.asarray(labels)
    present = np.flatnonzero(~np.isnan(native[:, 0]))
    dn = _pairdist(native[present].astype(np.float64))
    dm = _pairdist(model[present].astype(np.float64))
    counts, margin = [0, 0, 0, 0], float("inf")
    for a, i in enumerate(present):
        if labels[i] != d:
            continue
        for b, j in enumerate(present):
            if i == j:
                continue
            margin = min(margin, abs(dn[a, b] - RADIUS))
            if dn[a, b] < RADIUS:
                e = abs(dm[a, b] - dn[a, b])
                margin = min(margin, min(abs(e - t) for t in THRESHOLDS))
                kept = sum(1 for t in THRESHOLDS if e < t)
                at = 0 if labels[j] == d else 2
                counts[at] += kept
                counts[at + 1] += 1
    return counts[0], counts[1], counts[2], counts[3], margin


def near_pairs(native):
    """The ordered pairs of present native rows below 15 A."""
    native = np.asarray(native, dtype=np.float32)
    q = native[~np.isnan(native[:, 0])].astype(np.float64)
    dn = _pairdist(q)
    return int(((dn < RADIUS) & ~np.eye(len(q), dtype=bool)).sum())


def leg(model, native, labels, D):
    """One leg: {"rows": per domain (scores of the masked call, n, size, the four counts, margin), "lddt_res", "deviation"}."""
    model, native = np.asarray(model, dtype=np.float32), np.asarray(native, dtype=np.float32)
    labels = np.asarray(labels)
    L = len(labels)
    out = {"rows": [], "lddt_res": np.full(L, np.nan), "deviation": np.full(L, np.nan)}
    for d in range(D):
        want, margin = yardstick(model, masked(native, labels, d), 0.0)
        pres, pairs, opres, opairs, m2 = pair_counts(model, native, labels, d)
        mine = labels == d
        out["lddt_res"][mine] = want["lddt_res"][mine]
        out["deviation"][mine] = want["deviation"][mine]
        out["rows"].append(dict(want, n=want["n_pairs"], size=int(mine.sum()), preserved=pres, pairs=pairs, outer_preserved=opres,
                                outer_pairs=opairs, margin=min(margin, m2)))
    return out


def row_floats(row):
    """The 32 floats of a row (float32) from a dict of `leg`."""
    h = np.zeros(S.DOMSCORE_ROW, dtype=np.float32)
    h[0] = h[1] = row["n"]
    h[2:7] = [row[k] for k in ("rmsd", "tm", "gdt_ts", "gdt_ha", "lddt")]
    h[7:12] = row["counts"]
    h[12:21] = np.asarray(row["R"]).reshape(-1)
    h[21:24] = row["t"]
    h[24:29] = [row["preserved"], row["pairs"], row["outer_preserved"], row["outer_pairs"], row["size"]]
    return h


def block(model, native, label_model, D_model, label_native=None, D_native=0):
    """The whole block (float32 (1040 + 4L,)) -> (block, the two legs' dicts)."""
    L = len(label_model)
    native = np.asarray(native, dtype=np.float32)
    header = np.zeros(S.DOMSCORE_HEADER, dtype=np.float32)
    header[:3] = [D_model, D_native, int((~np.isnan(native[:, 0])).sum())]
    table = np.full((2, S.DOMAINS_MAX, S.DOMSCORE_ROW), np.nan, dtype=np.float32)
    res = np.full((4, L), np.nan, dtype=np.float32)
    legs = []
    for e, (labels, D) in enumerate(((label_model, D_model), (label_native, D_native))):
        if not D:
            continue
        one = leg(model, native, labels, D)
        for d, row in enumerate(one["rows"]):
            table[e, d] = row_floats(row)
        res[2 * e], res[2 * e + 1] = one["lddt_res"], one["deviation"]
        legs.append(one)
    return S.pack_domain_scores(L, header, table, res), legs


def moved_by_domain(trace, labels, noise=0.0, seed=0):
    """The trace with each domain moved by its own rigid transform - `_rotation(10 + d)` about the domain's centroid, then a
    shift of (9, -6, 4) (d + 1) - and, with `noise`, every residue displaced by a normal vector of that scale (float32)."""
    from test_score_cpu import _rotation
    trace = np.asarray(trace, dtype=np.float64)
    labels = np.asarray(labels)
    out = trace.copy()
    for d in range(int(labels.max()) + 1):
        mine = labels == d
        c = trace[mine].mean(0)
        out[mine] = (trace[mine] - c) @ _rotation(10 + d).T + c + np.asarray([9.0, -6.0, 4.0]) * (d + 1)
    if noise:
        out += np.random.default_rng(seed).normal(scale=noise, size=out.shape)
    return out.astype(np.float32)
