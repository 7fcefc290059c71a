"""NumPy restatement of option "msa_report" (include/dmpfold_hip.h): every number of the report block from the alignment's residue
codes and - as an INPUT - the DCA contact map the stem was given, with the native trace where the DCA precisions are wanted.

The integers (counts, histograms, the consensus letter, the partner, N_c, the native contacts, t, h) and the copied floats
(dca_max, the map) are exact.  The floats that are sums carry bounds derived here from the number formats, u = 2^-53 and
v = 2^-24, with MARGIN on the float64 part only (the float32 rounding is what it is); no constant comes from a kernel's output.

  neff_t, neff_col   a float64 sum of N positive terms in any order is within (N - 1) u of the exact sum, relatively; every
                     term 1 / k of neff carries one more u (a weight of neff_col is a float32 and exact in float64).  Library
                     and restatement each: |lib64 - ref64| <= 2 (N + 1) u |ref|.  The library then rounds once to float32:
                     |lib32 - lib64| <= v |lib64|.  The comparison is with the restatement's FLOAT64 value, so no second float32
                     rounding enters:  bound = v |ref| (1 + 2^-20) + MARGIN 2 (N + 1) u |ref|.
  cons_freq,         p = s / tot, both such sums, one division: relative 2 (N + 1) u + u per side:
  query_freq         bound = v p (1 + 2^-20) + MARGIN 2 (2 N + 3) u p.
  entropy            H = -sum_a p_a ln p_a over at most 20 letters.  With e = (2 N + 3) u the relative error of a p:
                     d(p ln p) <= p e (|ln p| + 1), summed: e (H + 1); a double `log` is within 1 ulp in both libraries
                     (<= 2 u relative, another u for the product, another for each of the 20 additions): (3 + 20) u H.
                     Per side e (H + 1) + 23 u H:  bound = v H (1 + 2^-20) + MARGIN 2 (e (H + 1) + 23 u H).
"""
import numpy as np

MARGIN = 8.0
U = 2.0 ** -53
V = 2.0 ** -24
HEADER, COLS, HIST = 128, 8, 20
THRESHOLDS = (0.62, 0.8, 0.9)
COLUMNS = ("gaps", "neff_col", "entropy", "cons", "cons_freq", "query_freq", "dca_max", "dca_partner")
DEPTHS = (1.0, 2.0, 5.0)


def clamp(codes):
    """Codes as the network and the reweighting see them: everything above 20 is 20, the gap."""
    return np.minimum(np.asarray(codes).astype(np.int64), 20)


def pair_counts(a):
    """cnt[n, m] = #{l : a_nl == a_ml}, gaps matching gaps (the reference's count)."""
    return (a[:, None, :] == a[None, :, :]).sum(-1).astype(np.int64)


def neighbour_counts(cnt, L, t):
    """#{m : float32(cnt[n, m]) > float32(float64(L) * t)} per row."""
    return (cnt.astype(np.float32) > np.float32(float(L) * t)).sum(1).astype(np.int64)


def bin20(num, den):
    """min(19, 20 num / den) in integer division; den == 0: bin 0."""
    return 0 if den == 0 else min(19, (20 * int(num)) // int(den))


def rank_bits(x):
    """The descending key of a float32: an order-preserving map of its bit pattern, inverted; every NaN last (0xffffffff)."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    asc = np.where(u & 0x80000000, (~u) & 0xffffffff, u | 0x80000000)
    key = (~asc) & 0xffffffff
    return np.where((u & 0x7fffffff) > 0x7f800000, np.uint64(0xffffffff), key).astype(np.uint64)


def ranked_pairs(contacts, pairs):
    """`pairs` [(i, j)] ordered by (rank_bits(contacts[i, j]), i, j) ascending: strongest coupling first, NaN last."""
    c = np.asarray(contacts, dtype=np.float32)
    L = c.shape[0]
    if not pairs:
        return []
    ii, jj = np.asarray(pairs, dtype=np.int64).T
    keys = (rank_bits(c[ii, jj]).reshape(-1) << np.uint64(22)) | (ii * L + jj).astype(np.uint64)
    return [pairs[k] for k in np.argsort(keys, kind="stable")]


def native_contact(native, i, j):
    """(dx dx + dy dy) + dz dz < 64 in float32, every operation rounded ("score_map"'s test)."""
    p, q = np.asarray(native[i], dtype=np.float32), np.asarray(native[j], dtype=np.float32)
    d = p - q
    return bool(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2]) < np.float32(64.0))


def class_of(s):
    return 0 if s <= 11 else (1 if s <= 23 else 2)


def dca_vs_native(contacts, native, lnorm=0.0):
    """The 48 class floats and (n, ln): per class N_c, native contacts, h (3), t (3), four zeros."""
    native = np.asarray(native, dtype=np.float32)
    L = native.shape[0]
    present = native[:, 0] == native[:, 0]
    n = int(present.sum())
    ln = float(np.float32(lnorm)) if lnorm > 0 else float(n)
    by_class = [[], [], []]
    for i in range(L):
        for j in range(i + 6, L):
            if present[i] and present[j]:
                by_class[class_of(j - i)].append((i, j))
    by_class.append(sorted(by_class[1] + by_class[2]))
    out = np.zeros(48)
    for c, pairs in enumerate(by_class):
        nat = {p for p in pairs if native_contact(native, *p)}
        order = ranked_pairs(contacts, pairs)
        out[12 * c], out[12 * c + 1] = len(pairs), len(nat)
        for k, d in enumerate(DEPTHS):
            t = min(int(max(1.0, np.floor(ln / d))), len(pairs))
            out[12 * c + 2 + k] = sum(1 for p in order[:t] if p in nat)
            out[12 * c + 5 + k] = t
    return out, n, ln


def report(codes, contacts=None, native=None, lnorm=0.0):
    """Every number of the block, floats in float64 -> dict: `header` (128,), `columns` (8, L), `bound_header` and
    `bound_columns` (0 where the number must be exact), `nbr` (3, N) the neighbour counts."""
    a = clamp(codes)
    N, L = a.shape
    cnt = pair_counts(a)
    h = np.zeros(HEADER)
    bh = np.zeros(HEADER)
    h[0], h[1] = N, L
    nbr = np.stack([neighbour_counts(cnt, L, t) for t in THRESHOLDS])
    for k in range(3):
        h[2 + k] = float(np.sum(1.0 / nbr[k].astype(np.float64)))
        bh[2 + k] = V * h[2 + k] * (1 + 2.0 ** -20) + MARGIN * 2 * (N + 1) * U * h[2 + k]
    h[5] = int((a == 20).sum())
    other = cnt - np.diag(np.full(N, L + 1))                 # (the diagonal out of the running)
    top = other.max(1) if N > 1 else np.zeros(N, dtype=np.int64)
    h[6] = int((top == L).sum()) if N > 1 else 0
    h[7] = int((a[0] == 20).sum())
    den = int((a[0] < 20).sum())
    for n in range(N):
        h[16 + bin20(int(((a[n] == a[0]) & (a[0] < 20)).sum()), den)] += 1
        h[36 + bin20(int((a[n] < 20).sum()), L)] += 1
        if N > 1:
            h[56 + bin20(int(top[n]), L)] += 1
    has_dca = N > 1
    if native is not None and has_dca:
        h[76:124], h[124], h[125] = dca_vs_native(contacts, native, lnorm)
    h[126], h[127] = float(has_dca), float(native is not None)

    w = (np.float32(1.0) / nbr[1].astype(np.float32)).astype(np.float32)
    cols = np.zeros((COLS, L))
    bc = np.zeros((COLS, L))
    e = (2 * N + 3) * U
    for l in range(L):
        col = a[:, l]
        raw = np.bincount(col, minlength=21)
        s = np.array([w[col == k].astype(np.float64).sum() for k in range(20)])
        tot = float(s.sum())
        cols[0, l] = raw[20]
        cols[1, l] = tot
        bc[1, l] = V * tot * (1 + 2.0 ** -20) + MARGIN * 2 * (N + 1) * U * tot
        if tot > 0:
            p = s / tot
            H = float(-(p[p > 0] * np.log(p[p > 0])).sum())
            cols[2, l] = H
            bc[2, l] = V * H * (1 + 2.0 ** -20) + MARGIN * 2 * (e * (H + 1) + 23 * U * H)
        if raw[:20].sum() == 0:
            cols[3, l] = cols[4, l] = np.nan
        else:
            best = int(np.argmax(raw[:20]))                  # (the first of equals: ties to the lowest code)
            cols[3, l] = best
            cols[4, l] = s[best] / tot
            bc[4, l] = V * cols[4, l] * (1 + 2.0 ** -20) + MARGIN * 2 * e * cols[4, l]
        if a[0, l] < 20:
            cols[5, l] = s[a[0, l]] / tot
            bc[5, l] = V * cols[5, l] * (1 + 2.0 ** -20) + MARGIN * 2 * e * cols[5, l]
        else:
            cols[5, l] = np.nan
        js = [j for j in range(L) if abs(j - l) >= 6]
        if has_dca and js:
            c = np.asarray(contacts, dtype=np.float32)
            keys = (rank_bits(c[l, js]) << np.uint64(32)) | np.asarray(js, dtype=np.uint64)
            j = js[int(np.argmin(keys))]
            cols[6, l], cols[7, l] = c[l, j], j
        else:
            cols[6, l] = cols[7, l] = np.nan
    return {"header": h, "columns": cols, "bound_header": bh, "bound_columns": bc, "nbr": nbr, "weights": w}


def split(block, L):
    """A report block -> (header (128,), columns (8, L), map (L, L) or None) as float32 views."""
    b = np.asarray(block, dtype=np.float32)
    cols = b[HEADER:HEADER + COLS * L].reshape(COLS, L)
    rest = b[HEADER + COLS * L:]
    assert rest.size in (0, L * L), rest.size
    return b[:HEADER], cols, (rest.reshape(L, L) if rest.size else None)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def check(ref, block, L):
    """{check: (error / bound or, for an exact check, 0.0 / inf, note)} of a library block against `report`'s dict.  Exact
    checks compare values (NaN where NaN, dca_max by its bits)."""
    hdr, cols, _ = split(block, L)
    res = {}
    exact_h = ref["bound_header"] == 0
    bad = np.flatnonzero(exact_h & (hdr.astype(np.float64) != ref["header"]))
    res["header_exact"] = (float("inf") if bad.size else 0.0, f"offsets {bad[:8].tolist()}: {hdr[bad[:8]].tolist()} for {ref['header'][bad[:8]].tolist()}")
    for k, name in ((2, "neff_62"), (3, "neff_80"), (4, "neff_90")):
        res[name] = (abs(float(hdr[k]) - ref["header"][k]) / ref["bound_header"][k], f"{float(hdr[k])!r} for {ref['header'][k]!r}")
    for k, name in enumerate(COLUMNS):
        got, want, bound = cols[k].astype(np.float64), ref["columns"][k], ref["bound_columns"][k]
        nan_ok = np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        if not nan_ok:
            res[name] = (float("inf"), "NaN in other places")
        elif name == "dca_max":
            same = np.array_equal(_bits(cols[k][ok]), _bits(want[ok]))
            res[name] = (0.0 if same else float("inf"), "bits")
        elif not bound.any():
            bad = np.flatnonzero(ok & (got != want))
            res[name] = (float("inf") if bad.size else 0.0, f"columns {bad[:8].tolist()}")
        else:
            err = np.abs(got - want)[ok]
            ratio = np.where(bound[ok] > 0, err / np.where(bound[ok] > 0, bound[ok], 1.0), np.where(err > 0, np.inf, 0.0))
            worst = int(np.argmax(ratio)) if ratio.size else 0
            res[name] = (float(ratio.max()) if ratio.size else 0.0, f"column {np.flatnonzero(ok)[worst] if ratio.size else -1}")
    return res


def failed(res):
    return [k for k, (r, _) in res.items() if not r <= 1.0]
