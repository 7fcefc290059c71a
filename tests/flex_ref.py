"""Option "flex" restated in NumPy: the one definition of include/dmpfold_hip.h, evaluated on the host in float64.

    leg(ca, cut_mA)            -> the Gaussian network model of one C-alpha trace (float32 (L, 3)) as a `Leg`
    block(L, cut_mA, m, n)     -> the flex block (48 + 20L floats) the library writes for the two legs, rounded once
    split(block, L)            -> the two legs of a block as raw float32 views
    check(ref, got)            -> {check: (largest error / its bound, note)}; a check holds when the ratio is <= 1

Tolerances, derived as tests/eigh_ref.py derives its own (EPS32 = 2^-24, U64 = 2^-53, every bound MARGIN = 8 times its
rounding bound, no constant taken from a kernel's output).  The library solves M = sigma I - Gamma in float64 - M's entries
are integers below 4096, exact in float32 - and rounds once at the end:

    mode[k][i] = (float)(sgn z_i)          lambda_k = (float)(sigma - mu)          msf_i = (float) sum_k z_ki z_ki / lambda_k

with z, mu and the sum in float64.  ||Gamma||_2 <= sigma and ||Gamma - lambda||_2 <= sigma for 0 <= lambda <= sigma (Gamma is
positive semi-definite and Gershgorin bounds it by twice the largest degree), so sigma stands where eigh_ref has ||M||_2 - and
M = sigma I - Gamma has the same bound.  The float64 solve is taken as backward stable with multiple 1, as there: eigenvalues
and residuals off by n U64 sigma.

  integers   degree, contacts, sigma, components, used: exact.
  lambda     |got - lambda| <= EPS32 |lambda| + n U64 sigma: one float32 rounding of lambda and the solver's error.
  orth       |u_j . u_k - delta_jk|, u the returned mode: u = z + dz with ||dz||_2 <= EPS32 (one rounding per element), so
             2 EPS32 from the two cross terms, and z_j . z_k in float64 is n U64 / GAP (eigh_ref (3), one rounding, not two).
  residual   ||Gamma u - lambda u||_2 <= n U64 sigma + ||Gamma - lambda||_2 ||dz||_2 <= n U64 sigma + 2 EPS32 sigma (eigh_ref (4)
             with one rounding: its constant 4 becomes 2).  lambda is the TRUE k-th eigenvalue; a column rotated inside a
             cluster of true eigenvalues of width w (neighbours closer than GAP sigma, the run taken over the WHOLE spectrum, so
             one that straddles the 8th / 9th eigenvalue counts in full) adds up to w: any unit vector of the cluster's
             invariant subspace is a right answer there, and its residual against a member's eigenvalue is at most w.
  sign       the component of largest magnitude is positive; a component of the other sign may tie within one float32 ulp
             (each of two float64 near-ties is rounded once).
  mode       only where the true eigenvalue stands alone (gaps to both neighbours >= GAP sigma): Davis-Kahan,
             ||u - v||_2 <= sqrt(2) b_res / (gap - b_res) for the NumPy vector v of the same sign, plus | ||u|| - 1 | <= b_orth and
             NumPy's own n U64.
  msf        only where every non-zero mode of the eight stands alone (the 9th eigenvalue counts as a neighbour): one float32
             rounding of a float64 sum whose terms carry the eigenvalue's and the vector's FLOAT64 errors - the library sums
             the float64 z, not the rounded modes -
               |d msf_i| <= EPS32 msf_i + sum_k ( 2 |z_ki| (n U64 sigma / gap_k) / lambda_k + z_ki^2 (n U64 sigma) / lambda_k^2 ).
  msf_self   always (it holds for any basis): msf_i against sum_k u_ki^2 / l_k recomputed in float64 from the RETURNED float32
             modes u and eigenvalues l over the modes the block calls non-zero: each term carries two roundings of u and one
             of l, the sum one more - 4 EPS32 msf_i - plus the float64 terms above without the gap (the vector's own float64
             error does not enter: the same vector is on both sides), z^2 (n U64 sigma) / lambda^2.

No GPU, no library."""
import numpy as np

EPS32 = 2.0 ** -24
U64 = 2.0 ** -53
MARGIN = 8.0
GAP = 1e-3                 # eigh_ref's: "separated" = a gap of at least GAP * sigma
NEV = 8
ZERO = 1e-7                # a mode is a zero mode iff lambda <= ZERO (include/dmpfold_hip.h derives the number)
HEADER, LEG = 16, 16


def contact_table(ca, cut_mA=7300):
    """bool (L, L): i != j and d^2 < c c, c = cut_mA / 1000.0, d^2 in float64 from the float32 coordinates as
    (dx*dx + dy*dy) + dz*dz - the expression of domains_ref.contact_table; a NaN coordinate makes no contact."""
    x = np.asarray(ca, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    c = cut_mA / 1000.0
    d = x[:, None, :] - x[None, :, :]
    with np.errstate(invalid="ignore"):
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = d2 < c * c
    return near & ~np.eye(x.shape[0], dtype=bool)


def cutoff_margin(ca, cut_mA=7300):
    """The smallest | d - c | over all pairs, Angstrom: how far the trace is from a contact that rounding could flip."""
    x = np.asarray(ca, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    iu = np.triu_indices(x.shape[0], 1)
    return float(np.abs(d[iu] - cut_mA / 1000.0).min())


def sign_rule(v):
    """Columns of v with the component of largest magnitude positive, first index on ties."""
    v = np.asarray(v, dtype=np.float64)
    s = np.sign(v[np.abs(v).argmax(axis=0), np.arange(v.shape[1])])
    s[s == 0] = 1.0
    return v * s


class Leg:
    """The float64 answer for one trace.  eigenvalues (8,), modes (8, L) ascending in lambda, msf (L,), and what the checks
    need of the whole spectrum."""

    def __init__(self, ca, cut_mA=7300):
        self.cut_mA = int(cut_mA)
        self.A = contact_table(ca, cut_mA)
        self.L = n = self.A.shape[0]
        assert n >= NEV
        self.degree = self.A.sum(1).astype(np.int64)
        self.contacts = int(self.A.sum()) // 2
        self.sigma = 2 * int(self.degree.max())
        self.gamma = np.diag(self.degree.astype(np.float64)) - self.A.astype(np.float64)
        self.lam_all, self.vec_all = np.linalg.eigh(self.gamma)
        self.eigenvalues = self.lam_all[:NEV].copy()
        self.modes = sign_rule(self.vec_all[:, :NEV]).T.copy()
        self.components = int((self.eigenvalues <= ZERO).sum())
        self.used = NEV - self.components
        live = self.eigenvalues > ZERO
        self.msf = np.zeros(n)
        for k in np.flatnonzero(live):                        # ascending, as the library sums
            self.msf = self.msf + (self.modes[k] * self.modes[k]) / self.eigenvalues[k]
        # clusters of the whole spectrum: runs whose neighbours are closer than GAP sigma
        thr = GAP * max(self.sigma, 1)
        brk = np.flatnonzero(np.diff(self.lam_all) >= thr) + 1
        first = np.r_[0, brk]
        last = np.r_[brk - 1, n - 1]
        self.cluster = np.zeros(n, dtype=np.int64)
        for c, (a, b) in enumerate(zip(first, last)):
            self.cluster[a:b + 1] = c
        self.width = np.array([self.lam_all[last[self.cluster[k]]] - self.lam_all[first[self.cluster[k]]] for k in range(NEV)])
        self.alone = np.array([first[self.cluster[k]] == last[self.cluster[k]] for k in range(NEV)])
        lo = np.r_[np.inf, np.diff(self.lam_all)]             # gap below eigenvalue k
        hi = np.r_[np.diff(self.lam_all), np.inf]             # gap above
        self.gap = np.minimum(lo, hi)[:NEV]
        self.msf_comparable = bool(self.alone[live].all())

    def connected(self):
        return self.components == 1 and self.lam_all[1] > ZERO

    def relative_gap(self):
        """The smallest (lambda_k+1 - lambda_k) / lambda_k+1 over the seven non-zero modes and the eigenvalue behind them."""
        lam = self.lam_all[self.components:NEV + 1]
        return float((np.diff(lam) / lam[1:]).min()) if lam.size > 1 else float("inf")

    def raw(self):
        """The leg as the library writes it: every figure rounded once to float32."""
        hdr = np.zeros(LEG, dtype=np.float32)
        hdr[:4] = [self.contacts, self.sigma, self.components, self.used]
        hdr[8:] = self.eigenvalues.astype(np.float32)
        return {"header": hdr, "degree": self.degree.astype(np.float32), "msf": self.msf.astype(np.float32),
                "modes": self.modes.astype(np.float32)}


def leg(ca, cut_mA=7300):
    return Leg(ca, cut_mA)


def block(L, cut_mA, model, native=None):
    """The flex block of a prediction of length L from the legs of its model and, with a native leg, of its native (`Leg`s or
    raw dicts): float32 (48 + 20L,)."""
    out = np.zeros(HEADER + 2 * LEG + 20 * L, dtype=np.float32)
    out[0], out[1], out[2] = L, cut_mA, 0.0 if native is None else 1.0
    out[HEADER + 2 * LEG + 10 * L:] = np.nan
    for e, p in enumerate((model, native)):
        if p is None:
            continue
        r = p.raw() if isinstance(p, Leg) else p
        out[HEADER + LEG * e:HEADER + LEG * (e + 1)] = r["header"]
        a = out[HEADER + 2 * LEG + 10 * L * e:HEADER + 2 * LEG + 10 * L * (e + 1)].reshape(10, L)
        a[0], a[1], a[2:] = r["degree"], r["msf"], r["modes"]
    return out


def split(blk, L):
    """(header (16,), [leg 0, leg 1]) of a flex block, each leg as the raw dict of `Leg.raw`: views."""
    blk = np.asarray(blk)
    assert blk.shape == (HEADER + 2 * LEG + 20 * L,), blk.shape
    legs = []
    for e in range(2):
        a = blk[HEADER + 2 * LEG + 10 * L * e:HEADER + 2 * LEG + 10 * L * (e + 1)].reshape(10, L)
        legs.append({"header": blk[HEADER + LEG * e:HEADER + LEG * (e + 1)], "degree": a[0], "msf": a[1], "modes": a[2:]})
    return blk[:HEADER], legs


def _ratio(err, bound):
    err = np.asarray(err, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err <= 0.0, 0.0, err / bound)                # 0 / 0 holds, x / 0 does not
    return np.where(np.isnan(err), np.inf, r)


def _worst(r, what):
    r = np.atleast_1d(r)
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), f"{what} {np.unravel_index(k, r.shape)}"


def check(ref, got):
    """The checks of the module docstring on `got` (the raw dict of one leg) against the `Leg` ref."""
    n, sig = ref.L, float(max(ref.sigma, 1))
    res = {}
    hdr = np.asarray(got["header"], dtype=np.float64)
    ints_ok = (np.array_equal(np.asarray(got["degree"], dtype=np.float64), ref.degree.astype(np.float64))
               and list(hdr[:4]) == [ref.contacts, ref.sigma, ref.components, ref.used] and not hdr[4:8].any())
    res["integers"] = (0.0 if ints_ok else np.inf, "" if ints_ok else f"header {list(hdr[:8])}")
    U = np.asarray(got["modes"], dtype=np.float64)
    msf = np.asarray(got["msf"], dtype=np.float64)
    lam_got = hdr[8:16]
    if not (np.isfinite(U).all() and np.isfinite(msf).all() and np.isfinite(lam_got).all()):
        res["finite"] = (np.inf, "a non-finite figure")
        return res
    f64 = n * U64 * sig
    lam = ref.eigenvalues
    res["lambda"] = _worst(_ratio(np.abs(lam_got - lam), MARGIN * (EPS32 * np.abs(lam) + f64)), "eigenvalue")
    b3 = MARGIN * (2.0 * EPS32 + n * U64 / GAP)
    res["orth"] = _worst(_ratio(np.abs(U @ U.T - np.eye(NEV)), b3), "modes")
    b4 = MARGIN * (2.0 * EPS32 * sig + f64)
    R = ref.gamma @ U.T - U.T * lam
    res["residual"] = _worst(_ratio(np.sqrt((R * R).sum(0)), b4 + ref.width), "mode")
    r6, note6 = 0.0, ""
    got32 = np.asarray(got["modes"], dtype=np.float32)
    for k in range(NEV):
        amax = float(np.abs(got32[k]).max())
        near = np.abs(U[k]) >= amax - float(np.spacing(np.float32(amax)))
        if not (U[k][near] > 0.0).any():
            r6, note6 = np.inf, f"mode {k}"
    res["sign"] = (r6, note6)
    r7, note7 = 0.0, "n/a"
    for k in np.flatnonzero(ref.alone):
        if not ref.gap[k] - b4 > 0.0:
            continue
        v = ref.modes[k]
        tie = ((np.abs(v) >= np.abs(v).max() * (1.0 - 2.0 * EPS32)) & (v < 0.0)).any()
        err = min(np.linalg.norm(U[k] - s * v) for s in ((1.0, -1.0) if tie else (1.0,)))
        b7 = np.sqrt(2.0) * b4 / (ref.gap[k] - b4) + b3 + MARGIN * n * U64
        r = float(_ratio(err, b7))
        if r >= r7:
            r7, note7 = r, f"mode {k}"
    res["mode"] = (r7, note7)
    live_ref = lam > ZERO
    if ref.msf_comparable:
        z = ref.modes
        terms = np.zeros(n)
        for k in np.flatnonzero(live_ref):
            terms += 2.0 * np.abs(z[k]) * (f64 / ref.gap[k]) / lam[k] + z[k] * z[k] * f64 / (lam[k] * lam[k])
        res["msf"] = _worst(_ratio(np.abs(msf - ref.msf), MARGIN * (EPS32 * np.abs(ref.msf) + terms)), "residue")
    else:
        res["msf"] = (0.0, "n/a")
    comps = int(hdr[2]) if 0 <= hdr[2] <= NEV else NEV
    again, terms = np.zeros(n), np.zeros(n)
    for k in range(comps, NEV):
        if lam_got[k] > 0.0:
            again += U[k] * U[k] / lam_got[k]
            terms += U[k] * U[k] * f64 / (lam_got[k] * lam_got[k])
    res["msf_self"] = _worst(_ratio(np.abs(msf - again), MARGIN * (4.0 * EPS32 * np.abs(again) + terms)), "residue")
    return res


def failed(res):
    return sorted(k for k, (r, _) in res.items() if not r <= 1.0)


def hinges(mode):
    """The residues i where the mode changes sign between i and i + 1; zero counts as positive."""
    neg = np.asarray(mode) < 0
    return [int(i) for i in np.flatnonzero(neg[1:] != neg[:-1])]


def parse_agreement(mode, sides):
    """The share of residues whose sign in `mode` agrees with the boolean `sides`, the better of the two assignments."""
    same = float(((np.asarray(mode) < 0) == np.asarray(sides, dtype=bool)).mean())
    return max(same, 1.0 - same)
