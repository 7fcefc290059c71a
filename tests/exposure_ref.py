"""Option "exposure" restated in NumPy (include/dmpfold_hip.h has the definition): float64 formed from the float32
coordinates and the float32 sphere points, every operation in the order the header writes it, every count an integer.  The point
table is an argument: tests/test_exposure_cpu.py passes score.exposure_points(), tests/test_gpu_exposure.py the 768 floats the
device holds (dmp_debug_fetch "exposure_points").

`surface_atoms` is the definition over any set of spheres; `exposure` applies it and the two pair counts to a backbone.  The
partners of an atom may be prefiltered by |c_i - c_j| < R_i + R_j + 0.01 (`prefilter`): a point of atom i lies R_i from c_i up
to rounding, so an atom further away than that cannot hold it; the CPU test shows the filtered form equal to the unfiltered one.
"""
import numpy as np

RADII = np.array([3.05, 3.27, 3.16, 2.80, 3.20], dtype=np.float64)      # N, CA, C, O, CB: atom radius + 1.4 A probe
POINTS = 256
MARGIN = 0.01
GLYCINE = 7                                                              # the residue code of G


def _sq(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def surface_atoms(centres, radii, present, points, prefilter=True):
    """Exposed points of every sphere: centres (n, 3) float32, radii (n,) float64 (probe included), present (n,) bool, points
    (256, 3) float32 -> int64 (n,), -1 for an absent sphere (it neither has points nor blocks any)."""
    C = np.asarray(centres, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    R = np.asarray(radii, dtype=np.float64).reshape(-1)
    U = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    present = np.asarray(present, dtype=bool).reshape(-1)
    n = np.full(C.shape[0], -1, dtype=np.int64)
    idx = np.arange(C.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for g in np.nonzero(present)[0]:
            p = C[g][None, :] + R[g] * U                                 # one multiply, then one add, per component
            partners = present & (idx != g)
            if prefilter:
                reach = (R[g] + R) + MARGIN
                partners &= _sq(C - C[g][None, :]) < reach * reach
            cj, rj = C[partners], R[partners]
            buried = (_sq(p[:, None, :] - cj[None, :, :]) < (rj * rj)[None, :]).any(axis=1)
            n[g] = U.shape[0] - int(buried.sum())
    return n


def exposure(coords, first_row, points, prefilter=True):
    """The three measures of a backbone: coords float32 (L, 5, 3) N, CA, C, O, CB, the alignment's first row (codes; a 7 is
    a glycine, whose CB is absent from the surface) -> dict with n (L, 5) int64 (-1 at a glycine's CB), hse_up, hse_down, cn10
    (L,) int64 and the header's counts: atoms, sums (5), buried_atoms."""
    X32 = np.asarray(coords, dtype=np.float32).reshape(-1, 5, 3)
    L = X32.shape[0]
    gly = np.asarray(first_row).reshape(-1)[:L] == GLYCINE
    present = np.ones((L, 5), dtype=bool)
    present[gly, 4] = False
    n = surface_atoms(X32.reshape(-1, 3), np.tile(RADII, L), present.reshape(-1), points, prefilter).reshape(L, 5)
    X = X32.astype(np.float64)
    CA, CB = X[:, 1], X[:, 4]
    off = ~np.eye(L, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        v = CB - CA
        w = CA[None, :, :] - CA[:, None, :]                              # w[i, j] = CA_j - CA_i
        near = (_sq(w) < 169.0) & off
        dot = (v[:, None, 0] * w[..., 0] + v[:, None, 1] * w[..., 1]) + v[:, None, 2] * w[..., 2]
        up = near & (dot > 0.0)
        down = near & ~up
        cn = (_sq(CB[None, :, :] - CB[:, None, :]) < 100.0) & off
    return {"n": n, "hse_up": up.sum(axis=1).astype(np.int64), "hse_down": down.sum(axis=1).astype(np.int64),
            "cn10": cn.sum(axis=1).astype(np.int64), "atoms": int(present.sum()),
            "sums": [int(np.maximum(n[:, a], 0).sum()) for a in range(5)], "buried_atoms": int((n == 0).sum())}


def arrays_of(e):
    """The eight per-residue arrays of one entity as the block holds them: float32 (8, L)."""
    return np.concatenate([e["n"].T, e["hse_up"][None], e["hse_down"][None], e["cn10"][None]]).astype(np.float32)


def header_of(e):
    """The seven header floats of one entity: atoms present, the five sums, atoms with n = 0."""
    return np.asarray([e["atoms"]] + list(e["sums"]) + [e["buried_atoms"]], dtype=np.float32)


def block_of(model, L, native=None):
    """The exposure block (32 + 16L floats) the library writes for the restatement's results."""
    b = np.zeros(32 + 16 * L, dtype=np.float32)
    b[0] = POINTS
    b[1:8] = header_of(model)
    arr = b[32:].reshape(16, L)
    arr[:8] = arrays_of(model)
    arr[8:] = np.nan
    if native is not None:
        b[8] = 1
        b[9:16] = header_of(native)
        arr[8:] = arrays_of(native)
    return b


def area(n):
    """Total accessible area in square Angstrom of counts (L, 5): the host's float64 sum of 4 pi R^2 n / 256."""
    return float((4.0 * np.pi * RADII * RADII * np.maximum(np.asarray(n), 0) / float(POINTS)).sum())
