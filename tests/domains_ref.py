"""Option "domains" restated in NumPy: the one definition of include/dmpfold_hip.h, evaluated on the host.  The library must
agree with this in every label and count (all of it is integer arithmetic behind one float64 comparison per residue pair).

    parse(ca)            -> the parse of one C-alpha trace (float32 (L, 3)) as a dict
    block(model, native) -> the domain block (32 + 2L + 256 floats) the library writes for those two parses

No GPU, no library."""
import numpy as np

LEVELS = 4                 # levels examined: at most 2 ** 4 domains
MAX_DOMAINS = 1 << LEVELS
HEADER, ROW = 32, 8
CUTOFF2 = 100.0            # Angstrom^2
MIN_SEPARATION = 3


def contact_table(ca):
    """bool (L, L): |i - j| >= 3 and d^2 < 100, d^2 in float64 from the float32 coordinates as (dx*dx + dy*dy) + dz*dz."""
    x = np.asarray(ca, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    with np.errstate(invalid="ignore"):
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = d2 < CUTOFF2
    i = np.arange(x.shape[0])
    return near & (np.abs(i[:, None] - i[None, :]) >= MIN_SEPARATION)


def cut_counts(table, idx):
    """(ext, int_A, int_B) as int64 (n + 1, n + 1) arrays over every (I, J) of the domain whose residues are `idx` (ascending),
    from the summed-area table of its sub-matrix: five reads per cut.  Entries with I >= J mean nothing."""
    n = len(idx)
    S = np.zeros((n + 1, n + 1), dtype=np.int64)
    S[1:, 1:] = table[np.ix_(idx, idx)].astype(np.int64).cumsum(0).cumsum(1)
    I, J = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    full_a = S[J, J] - 2 * S[I, J] + S[I, I]                   # both orders of every pair inside A
    ext = (S[J, n] - S[I, n]) - full_a
    int_a = full_a // 2
    int_b = S[n, n] // 2 - int_a - ext
    return ext, int_a, int_b


def admissible(n, min_size, min_segment):
    """bool (n + 1, n + 1): the cuts (I, J) of a domain of n residues that the size and segment rules admit."""
    I, J = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    size = J - I
    return ((I < J) & (size >= min_size) & (n - size >= min_size) & ((I == 0) | (I >= min_segment))
            & ((J == n) | (n - J >= min_segment)) & ~((I == 0) & (J == n)))


def best_cut(table, idx, min_size=40, min_segment=10):
    """The best admissible cut of a domain -> (I, J, ext, den) with den = min(int_A, int_B) + ext, or None without one.  The
    smallest ext / den by exact comparison, ties to the smallest (I, J).  Every product of the cross-multiplication is below
    2^44, so two different ratios differ by more than 2^-44 and their float64 quotients - correctly rounded - stand in the same
    order, equal ratios giving equal quotients; the choice is checked by the int64 cross-multiplication all the same."""
    n = len(idx)
    ext, int_a, int_b = cut_counts(table, idx)
    least = np.minimum(int_a, int_b)
    ok = admissible(n, min_size, min_segment) & (least > 0)
    if not ok.any():
        return None
    den = np.where(ok, least + ext, 1)
    q = np.where(ok, ext / den, np.inf)
    I, J = (int(v) for v in np.argwhere(q == q.min())[0])      # (row-major: the smallest I, then the smallest J)
    e, d = int(ext[I, J]), int(den[I, J])
    assert (ext[ok] * d >= e * den[ok]).all()
    return I, J, e, d


def parse(ca, min_size=40, min_segment=10, tau_milli=250):
    """The domains of a C-alpha trace -> dict: `labels` (int (L,), domains numbered by their lowest residue), `header` (the
    eight integers of the block's header), `table` (int (domains, 8): size, segments, lowest residue, contact pairs inside,
    contact pairs to the rest of the chain, ext and denominator of the cut that made the domain, level), `splits` (per split
    in the order made: level, node, I, J, ext, den) and `nodes` (the tree node of every residue: 1 the chain, 2k and 2k + 1
    the parts A and B of node k)."""
    table = contact_table(ca)
    L = table.shape[0]
    node = np.ones(L, dtype=np.int64)
    made = {1: (0, 0)}
    splits = []
    for level in range(LEVELS):
        for slot in range(1 << level):
            k = (1 << level) + slot
            idx = np.flatnonzero(node == k)
            if len(idx) < 2 * min_size:
                continue
            cut = best_cut(table, idx, min_size, min_segment)
            if cut is None:
                continue
            I, J, ext, den = cut
            if ext * 1000 < tau_milli * den:
                node[idx] = 2 * k + 1
                node[idx[I:J]] = 2 * k
                made[2 * k] = made[2 * k + 1] = (ext, den)
                splits.append((level, k, I, J, ext, den))
    kept = sorted(set(node.tolist()), key=lambda k: int(np.flatnonzero(node == k)[0]))
    labels = np.zeros(L, dtype=np.int64)
    rows = []
    for label, k in enumerate(kept):
        mine = node == k
        labels[mine] = label
        idx = np.flatnonzero(mine)
        segments = 1 + int((np.diff(idx) > 1).sum())
        inside = int(table[np.ix_(idx, idx)].sum()) // 2
        outside = int(table[mine][:, ~mine].sum())
        rows.append([len(idx), segments, int(idx[0]), inside, outside, made[k][0], made[k][1], k.bit_length() - 1])
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, ROW)
    final_large = any(k >= MAX_DOMAINS and int((node == k).sum()) >= 2 * min_size for k in kept)
    header = [len(kept), int(table.sum()) // 2, tau_milli, min_size, min_segment, int((rows[:, 1] > 1).sum()),
              int(rows[:, 7].max()), int(final_large)]
    return {"labels": labels, "header": header, "table": rows, "splits": splits, "nodes": node}


def block(model, native=None):
    """The domain block of a prediction of length L from the parse of its model and, with a native leg, of its native:
    float32 (32 + 2L + 256,)."""
    L = len(model["labels"])
    out = np.zeros(HEADER + 2 * L + 2 * MAX_DOMAINS * ROW, dtype=np.float32)
    out[HEADER + L:HEADER + 2 * L] = np.nan
    for leg, p in enumerate((model, native)):
        if p is None:
            continue
        out[16 * leg:16 * leg + 8] = p["header"]
        out[HEADER + leg * L:HEADER + (leg + 1) * L] = p["labels"]
        rows = p["table"]
        at = HEADER + 2 * L + leg * MAX_DOMAINS * ROW
        out[at:at + rows.size] = rows.reshape(-1)
    return out


def beside(a, b):
    """Globule `b` moved beside globule `a` along x so that they interpenetrate slightly: the centres 0.75 (r_a + r_b) + 2
    Angstrom apart, r the largest distance of a residue from its globule's centre (float32)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ca, cb = a.mean(0), b.mean(0)
    shift = 0.75 * (np.linalg.norm(a - ca, axis=1).max() + np.linalg.norm(b - cb, axis=1).max()) + 2.0
    return (b - cb + ca + np.asarray([shift, 0.0, 0.0])).astype(np.float32)


def globule(L, seed):
    """The compact self-avoiding trace the known answers were found on (float32 (L, 3))."""
    from dmpfold2_amd import synth
    return np.asarray(synth.protein_like_trace(L, seed, radius=3.0 * L ** (1 / 3) + 2.0), dtype=np.float32)


def chain(*globules):
    """The globules as one chain, each moved beside the one before it as that one was placed."""
    placed = [np.asarray(globules[0], dtype=np.float32)]
    for g in globules[1:]:
        placed.append(beside(placed[-1], g))
    return np.concatenate(placed)


def inserted(host, guest, at):
    """`guest` beside `host` and spliced into its chain in front of residue `at`: the host becomes a domain of two segments."""
    host = np.asarray(host, dtype=np.float32)
    return np.concatenate([host[:at], beside(host, guest), host[at:]])


def constructed(name):
    """The constructed traces of the known answers by name -> (trace, the label of every residue as built)."""
    if name == "80+80":
        return chain(globule(80, 0), globule(80, 10)), np.repeat([0, 1], 80)
    if name == "100+150":
        return chain(globule(100, 0), globule(150, 10)), np.repeat([0, 1], [100, 150])
    if name == "3x80":
        return chain(globule(80, 0), globule(80, 1), globule(80, 2)), np.repeat([0, 1, 2], 80)
    if name == "insertion":
        return inserted(globule(120, 0), globule(90, 10), 50), np.repeat([0, 1, 0], [50, 90, 70])
    raise KeyError(name)
