"""Reference for dmp_eigh_top8 (csrc/mds.hip) on spectra where eigenvectors are not unique: NumPy, float64, no GPU.

dmp_eigh_top8 returns the eigenvectors of the eight largest eigenvalues of a symmetric matrix (ascending: column 7
belongs to the largest), each scaled by sqrt(max(lambda, 1e-8)) and with the component of largest magnitude positive.
Inside a cluster of (nearly) equal eigenvalues any orthonormal basis of the invariant subspace is a right answer, so a
comparison of columns with LAPACK's says nothing there.  `check` states what must hold whatever basis a solver picks;
the generators build the spectra on which a solver can go wrong.

Tolerances.  The kernel solves in float64 and rounds to float32 at the very end (backtransform_kernel):

    mds[i][k] = (float)(sgn * z[i]) * sqrtf(fmaxf(fmaxf((float)lam, 0), 1e-8f))

so an element is  z_i sqrt(c) (1 + d_i)(1 + s)  with c = max(lam, 1e-8) and, in units of EPS32 = 2^-24 (the unit
roundoff of float32):  |d_i| <= 2 (the conversion of z_i and the product, one rounding each) and, common to the column,
|s| <= 2.5 (the conversion of lam is half a unit after the square root, sqrtf itself at most 1 ulp = 2 units).  The
float64 solve behind it is backward stable: eigenvalues and residuals are off by a small multiple of n 2^-53 ||M||_2; the
multiple is taken as 1 (Householder tridiagonalisation, bisection to 4e-16 relative, inverse iteration; the textbook
bounds carry a modest polynomial in n that practice never reaches, and the float32 terms dominate all of it at the orders
used here).  Every bound below is MARGIN = 8 times its rounding bound.  No constant is taken from a kernel's output.
(A solution rounded ONCE to float32, as the rounded LAPACK answer of the CPU test, has |d_i| <= 1: the constants of (3) and
(4) below are therefore 4 where one rounding would give 2 - read from the kernel's expression above, not from its output.)
"""
import numpy as np

EPS32 = 2.0 ** -24            # unit roundoff of float32
U64 = 2.0 ** -53              # unit roundoff of float64
MARGIN = 8.0                  # every bound: 8 x its rounding bound
CLAMP = 1e-8                  # the reference's clamp of the eigenvalues (network.py: clamp(min=1e-8))
GAP = 1e-3                    # "separated": a gap of at least GAP * ||M||_2 (the solver's own ortol is 1e-3 ||T||_1 >= that)
NEV = 8

# (2) | ||g||^2 - c |:  ||g||^2 = c (1+s)^2 sum z_i^2 (1+d_i)^2, relative error 2 |s| + 2 |d| = 2 * 2.5 + 2 * 2 = 9 EPS32;
#     the float64 eigenvalue itself is off by n U64 ||M||_2 (absolute; it also decides on which side of the clamp it falls).
C_NORM = 9.0
# (3) |u_j . u_k|, u = g / ||g||:  u = z + dz with ||dz||_2 <= 2 EPS32 (the element-wise d_i; the common factor cancels),
#     so u_j . u_k = z_j . z_k + z_j . dz_k + dz_j . z_k, the last two at most 2 * 2 = 4 EPS32.  z_j . z_k in float64 is
#     rounding inside a cluster (Gram-Schmidt) and n U64 ||M||_2 / gap <= n U64 / GAP outside.
C_ORTH = 4.0
# (4) ||M u - lam u||_2 = ||(M - lam)(z + dz)||_2 <= n U64 ||M||_2 + ||M - lam||_2 ||dz||_2, ||M - lam||_2 <= 2 ||M||_2
#     and ||dz||_2 <= 2 EPS32: 4 EPS32 ||M||_2.  (One rounding, as the rounded LAPACK solution has, gives 2 EPS32.)
#     lam is the TRUE k-th eigenvalue; a column that is rotated inside a cluster of width w adds up to w / 2.  The
#     generators' exact degeneracies are split by the float32 rounding of M by at most 2 EPS32 ||M||_F <= 7 EPS32
#     ||M||_2 for their spectra (||M||_F <= 3.5 ||M||_2), i.e. 3.5 EPS32 ||M||_2 of residual: inside the bound below,
#     so a rotation there is legitimate, while clusters wider than that have to be resolved.
C_RES = 4.0
# (5), (7b): Davis-Kahan sin(Theta) theorem.  Q an orthonormal basis of the computed columns of a group, H = Q^T M Q:
#     ||sin Theta||_F <= ||M Q - Q H||_F / delta, delta = distance from the eigenvalues of H to the rest of M's spectrum.
#     With U the (nearly orthonormal) unit columns and S = U^T U:  ||M Q - Q H||_F <= ||M U - U Lam||_F ||S^-1/2||_2
#     <= sqrt(m) b4 (1 + m b3), and the eigenvalues of H are within that of the group's, so delta >= gap - sqrt(m) b4.
#     b3, b4 are the bounds of (3), (4), margin included, so the result needs none of its own.  The checker's own float64
#     arithmetic adds a floor: LAPACK's vectors V are orthonormal to n U64, so ||Q - V V^T Q||_F <= ||I - V V^T||_2 ||Q||_F
#     = sqrt(m) n U64 (x MARGIN) even where the group is the whole space and the gap infinite.
# (6) two float32 ulps = 4 EPS32 relative: each of two float64 near-ties is rounded twice.
SIGN_ULPS = 2.0
# (7a) the project's existing whole-matrix check
C_LEGACY = 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# generators

def _mirror(M):
    M = np.asarray(M, dtype=np.float64)
    return (np.triu(M) + np.triu(M, 1).T).astype(np.float32)


def _rng(name, n, salt=0):
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), n, salt])


def _dense(lam, rng):
    n = len(lam)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return _mirror((Q * np.asarray(lam, dtype=np.float64)) @ Q.T)


def _fill(top, n, below=None):
    """`top` (descending, truncated to n) followed by n - len(top) well-separated values below `below` (default: half
    the smallest of top): evenly spaced down to one step above zero."""
    top = list(top)[:n]
    r = n - len(top)
    if below is None:
        below = 0.5 * abs(top[-1])
    rest = [below * (r - j) / r for j in range(r)]
    return np.array(top + rest, dtype=np.float64)


S = 50.0                                                   # ||M||_2 of the dense cases
_GEO = [S * 0.6 ** k for k in range(8)]                    # 50, 30, 18, 10.8, 6.48, 3.89, 2.33, 1.40


def separated(n, scale=1.0, name="separated"):
    return _mirror(_dense(_fill(_GEO, n), _rng(name, n)).astype(np.float64) * scale)


def pair(n):
    """lambda_1 = lambda_2.  The float32 rounding of M splits the two by about 1e-8 ||M||_2: the solver orthogonalises
    them (they are far inside its cluster tolerance), but inverse iteration alone already resolves such a split, so this
    case runs the cluster branch without depending on it.  The guards of that branch are the exactly degenerate cases:
    rank3, two_blocks, diag_repeats, identity, zero (and octet at n = 8)."""
    return _dense(_fill([S] + _GEO[:7], n), _rng("pair", n))


def octet(n):
    """All kept eigenvalues equal; split by the rounding of M as `pair` is, and like it no guard of the cluster branch
    above n = 8."""
    return _dense(_fill([S] * 8, n), _rng("octet", n))


def straddle(n):
    """lambda_6 .. lambda_10 equal (as many of them as the order has)."""
    return _dense(_fill(_GEO[:5] + [0.05 * S] * 5, n), _rng("straddle", n))


def gaps(n):
    """Adjacent eigenvalues 1e-6, 1e-4 and 1e-2 of lambda_max apart."""
    top = [S, S * (1 - 1e-6), 0.6 * S, S * (0.6 - 1e-4), 0.3 * S, S * (0.3 - 1e-2), 0.15 * S, 0.08 * S]
    return _dense(_fill(top, n), _rng("gaps", n))


def _lattice_walk(n, rng):
    """n points of a walk on the integer lattice, kept inside |x| <= 8: every squared distance is a small integer, so the
    Gram matrix is exact in float32 and exactly of rank 3."""
    P = np.zeros((n, 3))
    for i in range(1, n):
        while True:
            step = rng.integers(-1, 2, size=3)
            q = P[i - 1] + step
            if step.any() and np.abs(q).max() <= 8:
                break
        P[i] = q
    return P


def _gram(D):
    return 0.5 * (D[0:1, :] ** 2 + D[:, 0:1] ** 2 - D ** 2)


def rank3(n):
    P = _lattice_walk(n, _rng("rank3", n))
    D = np.linalg.norm(P[:, None] - P[None], axis=2)
    return _mirror(_gram(D))


def rank3_noise(n):
    rng = _rng("rank3", n)
    P = _lattice_walk(n, rng)
    D = np.linalg.norm(P[:, None] - P[None], axis=2) + np.abs(rng.standard_normal((n, n))) * 0.3
    D = 0.5 * (D + D.T)
    return _mirror(_gram(D))


def negative(n):
    """The negative of a positive-definite matrix: the kept eigenvalues are -1, -1.5, ... -17.1, the rest -25 .. -50."""
    top = [-1.0 * 1.5 ** k for k in range(8)]
    r = max(n - 8, 0)
    rest = [-0.5 * S - 0.5 * S * (j + 1) / r for j in range(r)]
    return _dense(np.array(top[:n] + rest), _rng("negative", n))


def scaled_down(n):
    return separated(n, 1e-12)


def scaled_up(n):
    return separated(n, 1e12)


def zero(n):
    return np.zeros((n, n), dtype=np.float32)


def identity(n, c=1.0):
    return (c * np.eye(n)).astype(np.float32)


def diag_distinct(n):
    return np.diag(_rng("diag_distinct", n).permutation(n) + 1.0).astype(np.float32)


def diag_repeats(n):
    vals = [5, 5, 4, 4, 4, 3, 2, 2] + [0.5 ** (1 + j // 2) for j in range(max(n - 8, 0))]
    return np.diag(_rng("diag_repeats", n).permutation(np.array(vals[:n], dtype=np.float64))).astype(np.float32)


def laplacian(n):
    return (2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)).astype(np.float32)


def laplacian_eigenvalues(n):
    return np.sort(2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1)))


def two_blocks(n):
    """Two identical dense blocks of order n // 2 (and a 1 x 1 block below every kept eigenvalue when n is odd)."""
    m = n // 2
    B = _dense(_fill(_GEO, m), _rng("two_blocks", n)).astype(np.float64)
    M = np.zeros((n, n))
    M[:m, :m] = B
    M[m:2 * m, m:2 * m] = B
    if n % 2:
        M[n - 1, n - 1] = 1e-3 * S
    return _mirror(M)


GENERATORS = {
    "separated": separated, "pair": pair, "octet": octet, "straddle": straddle, "gaps": gaps, "rank3": rank3,
    "rank3_noise": rank3_noise, "negative": negative, "scaled_down": scaled_down, "scaled_up": scaled_up,
    "zero": zero, "identity_1": lambda n: identity(n, 1.0), "identity_1e6": lambda n: identity(n, 1e6),
    "identity_neg1": lambda n: identity(n, -1.0), "diag_distinct": diag_distinct, "diag_repeats": diag_repeats,
    "laplacian": laplacian, "two_blocks": two_blocks,
}


# ---------------------------------------------------------------------------------------------------------------------
# truth and checks

class Truth:
    """float64 LAPACK solution of the float32 matrix as the kernel reads it (upper triangle mirrored)."""

    def __init__(self, M):
        M = np.asarray(M)
        assert M.dtype == np.float32 and M.ndim == 2 and M.shape[0] == M.shape[1] and M.shape[0] >= NEV
        A = M.astype(np.float64)
        self.A = np.triu(A) + np.triu(A, 1).T
        self.n = A.shape[0]
        self.lam_all, self.vec_all = np.linalg.eigh(self.A)           # ascending
        self.lam = self.lam_all[-NEV:]                                 # column k of the output belongs to lam[k]
        self.vec = self.vec_all[:, -NEV:]
        self.norm2 = float(np.abs(self.lam_all).max())

    def columns(self):
        """The reference's answer in float64: clamp, scale, sign rule (largest magnitude positive, first index on ties)."""
        v = self.vec
        sgn = np.sign(v[np.abs(v).argmax(axis=0), np.arange(NEV)])
        sgn[sgn == 0] = 1.0
        return v * sgn * np.sqrt(np.maximum(self.lam, CLAMP))

    def groups(self):
        """Maximal runs of the kept eigenvalues whose neighbours are closer than GAP ||M||_2, as (first column, last
        column, gap to the rest of the spectrum); gap is 0 for a run that reaches across the 8th / 9th boundary."""
        n, lam, thr = self.n, self.lam_all, GAP * self.norm2

        def sep(i):                         # is lam_all[i] separated from lam_all[i - 1]?
            if i <= 0 or i >= n:
                return True
            g = lam[i] - lam[i - 1]
            return g > 0.0 and g >= thr

        def gap_at(i):
            return np.inf if (i <= 0 or i >= n) else lam[i] - lam[i - 1]

        out, first = [], n - NEV
        for i in range(n - NEV + 1, n + 1):
            if sep(i):
                lo_ok = sep(first)
                gap = min(gap_at(first), gap_at(i)) if lo_ok else 0.0
                out.append((first - (n - NEV), i - 1 - (n - NEV), float(gap)))
                first = i
        return out


def truth(M):
    return Truth(M)


def check(M, got, T=None):
    """The invariants of the module docstring on `got` (float32 [n][8]).  Returns {check: (ratio, note)} with ratio =
    largest error / its bound (a check holds when ratio <= 1; 0 where it does not apply); check 1 failing ends it."""
    T = T or Truth(M)
    n, N2 = T.n, T.norm2
    got = np.asarray(got)
    assert got.shape == (n, NEV), got.shape
    res = {}
    bad = ~np.isfinite(got)
    if bad.any():
        i, k = np.argwhere(bad)[0]
        return {1: (np.inf, f"{int(bad.sum())} non-finite, first at [{i}][{k}]")}
    res[1] = (0.0, "")
    G = got.astype(np.float64)
    c = np.maximum(T.lam, CLAMP)
    f64 = n * U64 * N2

    def ratio(err, bound):
        err = np.asarray(err, dtype=np.float64)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err <= 0.0, 0.0, err / bound)            # 0 / 0 holds, x / 0 does not
        return r

    def worst(r, what):
        r = np.atleast_1d(r)
        k = int(np.argmax(r))
        return float(r[k]), f"{what} {k}"

    # 2: column norms
    nn = (G * G).sum(axis=0)
    b2 = MARGIN * (C_NORM * EPS32 * c + f64)
    res[2] = worst(ratio(np.abs(nn - c), b2), "column")

    # 3: orthonormality of the unit columns (a zero column has no direction: it fails 2 and is left out here)
    live = nn > 0.0
    U = np.zeros_like(G)
    U[:, live] = G[:, live] / np.sqrt(nn[live])
    b3 = MARGIN * (C_ORTH * EPS32 + n * U64 / GAP)
    O = U.T @ U - np.diag(live.astype(np.float64))
    r3 = ratio(np.abs(O), b3)
    j, k = np.unravel_index(int(np.argmax(r3)), r3.shape)
    res[3] = (float(r3[j, k]), f"columns {j},{k}")

    # 4: residuals against the true eigenvalues
    b4 = MARGIN * (C_RES * EPS32 * N2 + f64)
    R = T.A @ U - U * T.lam
    rn = np.sqrt((R * R).sum(axis=0))
    res[4] = worst(ratio(rn, b4), "column")

    # 5: invariant subspaces of the separated groups
    r5, note5 = 0.0, ""
    off = n - NEV
    for a, b, gap in T.groups():
        if gap <= 0.0:
            continue
        m = b - a + 1
        Q, _ = np.linalg.qr(U[:, a:b + 1])
        Vt = T.vec_all[:, off + a:off + b + 1]
        err = np.linalg.norm(Q - Vt @ (Vt.T @ Q))                 # ||sin Theta||_F
        rr = np.sqrt(m) * b4 * (1.0 + m * b3)
        delta = gap - rr
        b5 = (rr / delta if delta > 0.0 and np.isfinite(gap) else (0.0 if np.isinf(gap) else np.inf)) + MARGIN * np.sqrt(m) * n * U64
        r = float(ratio(err, b5))
        if r >= r5:
            r5, note5 = r, f"columns {a}..{b}"
    res[5] = (r5, note5)

    # 6: sign rule
    amax = np.abs(got).max(axis=0)
    r6, note6 = 0.0, ""
    for k in range(NEV):
        if amax[k] == 0.0:
            continue
        tol = SIGN_ULPS * float(np.spacing(np.float32(amax[k])))
        near = np.abs(G[:, k]) >= float(amax[k]) - tol
        if not (G[near, k] > 0.0).any():
            r6, note6 = np.inf, f"column {k}"
    res[6] = (r6, note6)

    # 7: direct comparison where every kept eigenvalue stands alone
    grp = T.groups()
    res[7] = (0.0, "n/a")
    if len(grp) == NEV and all(g > 0.0 for _, _, g in grp):
        V = T.vec
        amaxv = np.abs(V).max(axis=0)
        best = np.full(NEV, np.inf)
        cols = np.zeros_like(V)
        for k in range(NEV):
            i0 = int(np.abs(V[:, k]).argmax())
            s0 = 1.0 if V[i0, k] >= 0.0 else -1.0
            # the other sign is as right where a component of the other sign ties within what float32 can tell
            tie = ((np.abs(V[:, k]) >= amaxv[k] * (1.0 - 2 * SIGN_ULPS * EPS32)) & (V[:, k] * s0 < 0.0)).any()
            for s in ((s0, -s0) if tie else (s0,)):
                t = s * V[:, k] * np.sqrt(c[k])
                e = np.linalg.norm(G[:, k] - t)
                if e < best[k]:
                    best[k], cols[:, k] = e, t
        ra = float(ratio(np.abs(G - cols).max(), C_LEGACY * np.abs(cols).max()))
        gk = np.array([g for _, _, g in grp])
        with np.errstate(divide="ignore", invalid="ignore"):
            ang = np.where(np.isinf(gk), 0.0, np.sqrt(2.0) * b4 / np.maximum(gk - b4, 1e-300))   # ||u - v|| <= sqrt(2) sin
        b7 = np.sqrt(nn) * (ang + MARGIN * n * U64) + b2 / np.sqrt(c)       # + | ||g|| - sqrt(c) | <= b2 / sqrt(c)
        rb, nb = worst(ratio(best, b7), "column")
        res[7] = (ra, "whole matrix, 2e-5") if ra >= rb else (rb, nb + ", own scale")
    return res


def failed(res):
    return sorted(k for k, (r, _) in res.items() if not r <= 1.0)


def reference_solution(M, T=None):
    """LAPACK's float64 answer (clamp and sign rule applied) rounded once to float32."""
    T = T or Truth(M)
    return T.columns().astype(np.float32)
