"""Option "align_structure" without a GPU: the float64 yardstick - a NumPy restatement of the definition in
include/dmpfold_hip.h (Kabsch by SVD, the dynamic programme vectorised along anti-diagonals) -, sanity tests of the
definition itself, the layout functions and the host helpers of dmpfold2_amd/score.py.

The yardstick also returns `margin`: the smallest non-zero gap it saw at any decision (the three-way maximum of a DP cell,
d against d_cut, the tm of rank 16 against rank 17, the winner against the runner-up).  tests/test_gpu_align.py fails a case
whose margin is below NEAR_TIE with "choose another seed": both sides are float64, about 1e-13 apart per term, and a DP path
sums a few hundred terms.
"""
import itertools

import numpy as np
import pytest

from dmpfold2_amd import score as S
from test_score_cpu import _rotation, ulp32

NEAR_TIE = 1e-9
SURVIVORS, ROUNDS, ITERS, GAP = 16, 10, 20, -0.6


# ------------------------------------------------------------------------------------------------ the yardstick
def d0_of(length):
    return max(1.24 * float(np.cbrt(length - 15.0)) - 1.8, 0.5) if length > 15 else 0.5


def _kabsch(P, Q):
    """R, t minimising sum |R p + t - q|^2."""
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((P - pc).T @ (Q - qc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, qc - R @ pc


def _dev(R, t, P, Q):
    e = P @ R.T + t - Q
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


class _Margin:
    def __init__(self):
        self.value = np.inf

    def gaps(self, g):
        g = np.abs(np.asarray(g, dtype=np.float64)).reshape(-1)
        g = g[g > 0.0]
        if g.size:
            self.value = min(self.value, float(g.min()))


def superpose(P, Q, d0, lnorm, d_cut, mg):
    """The loop of one seed on packed pairs -> (tm, R, t, rmsd of the first superposition)."""
    sel = np.ones(len(P), dtype=bool)
    best, best_Rt, rmsd = -1.0, None, None
    for it in range(ITERS):
        R, t = _kabsch(P[sel], Q[sel])
        d = _dev(R, t, P, Q)
        tm = float((1.0 / (1.0 + (d / d0) ** 2)).sum() / lnorm)
        if it == 0:
            rmsd = float(np.sqrt((d * d).sum() / len(P)))
        if tm > best:
            best, best_Rt = tm, (R, t)
        mg.gaps(d - d_cut)
        new = d < d_cut
        if new.sum() < 3 or np.array_equal(new, sel):
            break
        sel = new
    return best, best_Rt[0], best_Rt[1], rmsd


def _dp(P, Q, R, t, d0s, mg):
    """The dynamic programme and its traceback -> [(i, j)] in increasing order."""
    n, m = len(P), len(Q)
    e = (P @ R.T + t)[:, None, :] - Q[None, :, :]
    sc = 1.0 / (1.0 + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / (d0s * d0s))
    H = np.zeros((n + 1, m + 1))
    D = np.zeros((n + 1, m + 1), dtype=bool)
    dr = np.zeros((n + 1, m + 1), dtype=np.uint8)
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        a = H[i - 1, j - 1] + sc[i - 1, j - 1]
        b = H[i - 1, j] + np.where(D[i - 1, j], GAP, 0.0)
        c = H[i, j - 1] + np.where(D[i, j - 1], GAP, 0.0)
        bc = np.maximum(b, c)
        diag = a >= bc
        up = ~diag & (b >= c)
        mg.gaps(a - bc)
        mg.gaps((b - c)[~diag])
        H[i, j] = np.where(diag, a, bc)
        D[i, j] = diag
        dr[i, j] = np.where(diag, 0, np.where(up, 1, 2))
    pairs, i, j = [], n, m
    while i > 0 and j > 0:
        if dr[i, j] == 0:
            pairs.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        elif dr[i, j] == 1:
            i -= 1
        else:
            j -= 1
    return pairs[::-1]


def _packed(P, Q, A):
    ii = np.array([a[0] for a in A], dtype=np.int64)
    jj = np.array([a[1] for a in A], dtype=np.int64)
    return P[ii], Q[jj]


def yardstick(model, structure, as_float32=True):
    """The definition of include/dmpfold_hip.h on float32 traces (n, 3) and (m, 3), in float64 -> (dict, margin).
    `as_float32` False: the traces are taken as the float64 values they are (an exact rigid copy)."""
    P = np.asarray(model, dtype=np.float32 if as_float32 else np.float64).astype(np.float64)
    Q = np.asarray(structure, dtype=np.float32 if as_float32 else np.float64).astype(np.float64)
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
    if len(order) > SURVIVORS:
        mg.gaps(tms[order[SURVIVORS - 1]] - tms[order[SURVIVORS]])
    results = []                                     # (tm, seed number, alignment)
    for s in order[:SURVIVORS]:
        A, best_tm, best_A = seed_pairs(offsets[s]), -1.0, []
        for rnd in range(ROUNDS):
            tm, R, t, _ = superpose(*_packed(P, Q, A), d0s, lmin, d_cut, mg)
            if tm > best_tm:
                best_tm, best_A = tm, A
            if rnd == ROUNDS - 1:
                break
            A2 = _dp(P, Q, R, t, d0s, mg)
            if A2 == A or len(A2) < 3:
                break
            A = A2
        results.append((best_tm, s, best_A))
    results.sort(key=lambda r: (-r[0], r[1]))
    top = results[0]
    mg.gaps([top[0] - r[0] for r in results[1:]])
    A = top[2]
    PA, QA = _packed(P, Q, A)
    tm_model, _, _, rmsd = superpose(PA, QA, d0_of(n), n, d_cut, mg)
    tm_struct, R, t, _ = superpose(PA, QA, d0_of(m), m, d_cut, mg)
    ali = np.full(n, -1, dtype=np.int64)
    dev = np.full(n, np.nan)
    ii = np.array([a[0] for a in A])
    ali[ii] = [a[1] for a in A]
    dev[ii] = _dev(R, t, PA, QA)
    out = {"n_ali": len(A), "rmsd_ali": rmsd, "tm_model": tm_model, "tm_struct": tm_struct, "d0_model": d0_of(n),
           "d0_struct": d0_of(m), "seed_offset": offsets[top[1]], "seeds": len(offsets), "R": R, "t": t, "ali": ali,
           "deviation": dev}
    return out, mg.value


def compare_alignment(got, want, margin, tag=""):
    """`got`: score.unpack_alignment of the library's block; `want`, `margin`: yardstick().  ali, n_ali, seed_offset and seeds
    must be equal; the floats lie within 1 float32 ulp of float32(yardstick) (entries of R within 1e-6 of zero: within 1e-6
    absolute) - the rule of test_score_cpu.compare_with_yardstick.  Returns the largest differences seen, in ulps."""
    if not margin >= NEAR_TIE:
        pytest.fail(f"{tag}: near tie (margin {margin:.3e}), choose another seed")
    for name in ("n_ali", "seed_offset", "seeds"):
        assert got[name] == want[name], (tag, name, got[name], want[name])
    assert np.array_equal(got["ali"], want["ali"]), (tag, "ali", np.nonzero(got["ali"] != want["ali"])[0][:10])
    seen = {}
    for name in ("tm_model", "tm_struct", "rmsd_ali", "d0_model", "d0_struct", "R", "t", "deviation"):
        g = np.asarray(got[name], dtype=np.float32).astype(np.float64).reshape(-1)
        w = np.asarray(want[name], dtype=np.float64).reshape(-1).astype(np.float32).astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, name, "NaN pattern")
        ok = ~np.isnan(w)
        diff = np.abs(g[ok] - w[ok])
        ulps = diff / ulp32(w[ok])
        fine = ulps <= 1.0
        if name == "R":
            fine |= (np.abs(w[ok]) <= 1e-6) & (diff <= 1e-6)
        seen[name] = float(ulps[np.abs(w[ok]) > 1e-6].max()) if (np.abs(w[ok]) > 1e-6).any() else 0.0
        assert bool(fine.all()), (tag, name, "max ulps", float(ulps.max()), "max abs", float(diff.max()))
    return seen


# ------------------------------------------------------------------------------------------------ test structures
def random_walk(L, seed, step=3.8, clash=3.0):
    """A self-avoiding walk of fixed step length: a step that comes within `clash` of an earlier point is drawn again."""
    rng = np.random.default_rng(seed)
    pts = [np.zeros(3)]
    while len(pts) < L:
        for _ in range(200):
            v = rng.normal(size=3)
            p = pts[-1] + step * v / np.linalg.norm(v)
            if len(pts) < 2 or np.linalg.norm(np.asarray(pts[:-1]) - p, axis=1).min() > clash:
                break
        pts.append(p)
    return np.asarray(pts, dtype=np.float32)


def moved(trace, seed, shift=(11.0, -7.0, 5.0)):
    R = _rotation(seed)
    return R, np.asarray(shift), (np.asarray(trace, dtype=np.float64) @ R.T + np.asarray(shift)).astype(np.float32)


def indel_copy(model, seed, m=None, noise=0.4):
    """A structure made from `model`: `dele` consecutive rows deleted, `ins` foreign rows inserted elsewhere, noise, a rigid
    motion -> (structure float32 (m, 3), correspondence (L,) with -1 for the deleted rows).  Without `m`: dele =
    max(4, L // 12) and ins = 7; with `m`: the pair (dele, ins) of smallest size that gives m rows."""
    model = np.asarray(model, dtype=np.float64)
    L = len(model)
    rng = np.random.default_rng(seed)
    if m is None:
        dele, ins = max(4, L // 12), 7
    else:
        dele, ins = (L - m, 0) if m < L else (0, m - L)
        if L >= 31:                                            # room for both: an indel pair
            dele, ins = dele + max(4, L // 12), ins + max(4, L // 12)
    a = L // 3                                                 # the deletion begins here
    keep = [i for i in range(L) if not (a <= i < a + dele)]
    rows = model[keep] + rng.normal(scale=noise, size=(len(keep), 3))
    corr = np.full(L, -1, dtype=np.int64)
    at = next((k for k, i in enumerate(keep) if i >= (2 * L) // 3), len(keep))       # the insertion goes in front of row `at`
    if ins:
        v = rng.normal(size=(ins, 3))
        loop = rows[max(at - 1, 0)] + np.cumsum(3.8 * v / np.linalg.norm(v, axis=1, keepdims=True), axis=0) + 6.0
        rows = np.concatenate([rows[:at], loop, rows[at:]])
    for k, i in enumerate(keep):
        corr[i] = k if k < at else k + ins
    _, _, out = moved(rows, seed)
    return out, corr


# ------------------------------------------------------------------------------------------------ sanity of the definition
def test_rigid_copy_is_the_identity_alignment():
    model = random_walk(50, 1)
    R, t, struct = moved(model.astype(np.float64), 2)
    struct64 = model.astype(np.float64) @ R.T + t
    want, _ = yardstick(model, struct)
    assert np.array_equal(want["ali"], np.arange(50)) and want["n_ali"] == 50
    # (several seeds reach the identity alignment and so the same tm; the tie goes to the lowest seed number, not to k = 0)
    assert want["seeds"] == 50 + 50 - 2 * 25 + 1
    # the float32 rounding of the moved copy costs about 1e-13 of tm; an exact copy gives 1 within 1e-12
    exact, _ = yardstick(model.astype(np.float64), struct64, as_float32=False)
    assert abs(exact["tm_model"] - 1.0) <= 1e-12 and abs(exact["tm_struct"] - 1.0) <= 1e-12
    assert abs(want["tm_model"] - 1.0) <= 1e-6


@pytest.mark.parametrize("L", [64, 120, 257])
def test_indel_copy_recovers_the_correspondence(L):
    model = random_walk(L, 10 + L)
    struct, corr = indel_copy(model, 20 + L)
    assert len(struct) == L - max(4, L // 12) + 7
    want, margin = yardstick(model, struct)
    print("L", L, "m", len(struct), "n_ali", want["n_ali"], "tm_model", want["tm_model"], "margin", margin)
    assert np.array_equal(want["ali"], corr), np.nonzero(want["ali"] != corr)[0]


def test_unrelated_walks_score_low():
    want, _ = yardstick(random_walk(100, 5), random_walk(90, 6))
    print("unrelated 100 x 90: tm_model", want["tm_model"], "tm_struct", want["tm_struct"], "n_ali", want["n_ali"])
    assert want["tm_model"] < 0.35 and want["tm_struct"] < 0.35


# ------------------------------------------------------------------------------------------------ layout and host helpers
def test_layout_functions():
    for L, m in ((8, 3), (65, 70), (257, 200)):
        assert S.align_floats(L, m) == 25 + 2 * L + 3 * m
        for emit, score, align in itertools.product((False, True), repeat=3):
            want = L + (L * L + 3 if emit else 0) + (5 * L + 24 if score else 0) + (25 + 2 * L + 3 * m if align else 0)
            assert S.conf_floats(L, emit, score, m if align else None) == want
            assert S.conf_floats(L, emit, score) == want - (25 + 2 * L + 3 * m if align else 0)      # the positional form
            assert S.align_offset(L, emit, score) == S.conf_floats(L, emit, score)
            buf = np.arange(want, dtype=np.float32)
            out = S.split_conf_buffer(buf, L, emit, score, None, m if align else None)
            assert (out.align_block is not None) == align and (out.score_block is not None) == score
            if align:
                assert out.align_block[0] == S.align_offset(L, emit, score) and out.align_block.shape == (S.align_floats(L, m),)
            pub = out._replace(coords=0).public()
            assert len(pub) == 2 + 2 * emit + score + align
            back = S.Outputs.of(pub, emit, score, align)
            assert (back.align_block is None) == (not align) and (back.score_block is None) == (not score)


def test_pack_and_unpack_round_trip():
    L, m = 9, 5
    ca = random_walk(m, 3)
    block = S.pack_structure(ca, L)
    assert block.shape == (S.align_floats(L, m),) and block[0] == 5.0 and np.isnan(block[1:25 + 2 * L]).all()
    al = S.unpack_alignment(block, L)
    assert al["n_ali"] == 0 and np.isnan(al["tm_model"]) and (al["ali"] == -1).all() and np.isnan(al["deviation"]).all()
    assert al["m"] == 5.0 and np.array_equal(al["structure"], ca)
    block[1:25] = np.arange(1, 25, dtype=np.float32)
    block[25:25 + L] = [0, 1, -1, 2, 3, -1, -1, 4, -1]
    block[25 + L:25 + 2 * L] = 0.5
    al = S.unpack_alignment(block, L)
    assert (al["n_ali"], al["rmsd_ali"], al["tm_model"], al["tm_struct"]) == (1, 2.0, 3.0, 4.0)
    assert np.array_equal(al["R"].reshape(-1), np.arange(5, 14)) and np.array_equal(al["t"], [14, 15, 16])
    assert (al["d0_model"], al["d0_struct"], al["seed_offset"], al["seeds"]) == (17.0, 18.0, 19, 20)
    assert list(al["ali"]) == [0, 1, -1, 2, 3, -1, -1, 4, -1] and al["ali"].dtype.kind == "i"
    js = S.alignment_json(al)
    assert js["n_ali"] == 1 and js["ali"][2] == -1 and js["m"] == 5.0 and js["R"][0] == [5.0, 6.0, 7.0]
    assert S.alignment_json(S.unpack_alignment(S.empty_structure(L), L))["tm_model"] is None
    assert S.pack_structure(ca, L, m_value=2.5)[0] == 2.5
    with pytest.raises(ValueError):
        S.unpack_alignment(block[:-1], L)
    with pytest.raises(ValueError):
        S.pack_structure(np.zeros((4, 2)), L)


def test_abi_is_unchanged():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5


def test_cli_parser_accepts_the_new_flags():
    from dmpfold2_amd.predict import dmpfold_parser
    p = dmpfold_parser()
    old = p.parse_args(["-i", "x.aln"])
    assert (old.compare, old.compare_chain, old.alignment) == (None, None, None)
    assert (old.native, old.native_chain, old.scores, old.distmap, old.converge) == (None, None, None, None, None)
    assert (old.iterations, old.minsteps, old.device) == (10, 100, "cuda")
    new = p.parse_args(["-i", "x.aln", "--compare", "s.pdb", "--compare-chain", "B", "--alignment", "a.json"])
    assert (new.compare, new.compare_chain, new.alignment) == ("s.pdb", "B", "a.json")
