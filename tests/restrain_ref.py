"""NumPy restatement of the restrained minimiser step (options "restrain_milli" / "restrain_cut_mA" of
include/dmpfold_hip.h), dtype-parametric: float32 restates the kernel's arithmetic up to the order of the partner sum,
float64 is the yardstick.  It shares nothing with the library; tests/test_restrain_cpu.py and tests/test_gpu_restrain.py
use it.  k = 0 or dm = None is the plain step of the reference's minimiser (network.py:106-137)."""
import numpy as np


def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def restraint_mask(dm, cut):
    """(L, L) bool: pairs with |i - j| >= 2 whose map entry lies below the cutoff (NaN: not restrained)."""
    L = dm.shape[0]
    idx = np.arange(L)
    sep = np.abs(idx[:, None] - idx[None, :])
    with np.errstate(invalid="ignore"):
        return (sep >= 2) & (dm < cut)


def restraint_accel(x, dm, k, cut, dtype=np.float64):
    """The restraint term alone: a_j = - sum_i (k e_ij) (x_j - x_i) / dr_ij over the restrained partners i of j."""
    f = dtype
    x = np.asarray(x, dtype=f)
    t = np.asarray(dm, dtype=f)
    dv = x[:, None, :] - x[None, :, :]                      # [j][i] = x_j - x_i
    dr = np.maximum(_norm(dv), f(0.01))
    # the thread that owns j reads dm[i][j]
    mask = restraint_mask(t, f(cut)).T
    e = np.minimum(np.maximum(dr - np.where(mask, t.T, f(0)), f(-3.0)), f(3.0))
    ke = np.where(mask, f(k) * e, f(0))
    return -(ke[..., None] * (dv / dr[..., None])).sum(axis=1, dtype=f)


def steric_accel(x, dtype=np.float64):
    f = dtype
    x = np.asarray(x, dtype=f)
    dv = x[:, None, :] - x[None, :, :]
    d = np.minimum(np.maximum(_norm(dv), f(0.01)), f(10.0))
    viol = np.where(d < f(3.0), f(3.0) - d, f(0))
    return ((f(100.0) * viol)[..., None] * (dv / d[..., None])).sum(axis=1, dtype=f)


def bond_accel(x, dtype=np.float64):
    f = dtype
    x = np.asarray(x, dtype=f)
    a = np.zeros_like(x)
    dv = x[1:] - x[:-1]
    d = np.maximum(_norm(dv), f(0.1))
    cov = (f(100.0) * np.minimum(d - f(3.78), f(3.0)))[:, None] * (dv / d[:, None])
    a[:-1] += cov
    a[1:] -= cov
    return a


def step(x, dm=None, k=0.0, cut=15.0, dtype=np.float64):
    """One step: x (L, 3) -> x + clamp(a, +-100) * 0.001, a = steric + restraint (if k > 0 and a map) + bonds."""
    f = dtype
    x = np.asarray(x, dtype=f)
    a = steric_accel(x, f)
    if dm is not None and k > 0:
        a = a + restraint_accel(x, dm, k, cut, f)
    a = a + bond_accel(x, f)
    return x + np.minimum(np.maximum(a, f(-100.0)), f(100.0)) * f(0.001)


def refine(x, steps, dm=None, k=0.0, cut=15.0, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    for _ in range(int(steps)):
        x = step(x, dm, k, cut, dtype)
    return x


def distances(x):
    """(L, L) float64 distances of a trace."""
    x = np.asarray(x, dtype=np.float64)
    return _norm(x[:, None, :] - x[None, :, :])


def map_rms(dm, x):
    """sqrt(mean over i < j of (dm_ij - |x_i - x_j|)^2), float64: the map_rms of option "emit_distmap"."""
    L = len(x)
    iu = np.triu_indices(L, 1)
    return float(np.sqrt(np.mean((np.asarray(dm, dtype=np.float64)[iu] - distances(x)[iu]) ** 2)))
