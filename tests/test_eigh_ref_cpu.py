"""tests/eigh_ref.py is fair (LAPACK's own float64 solution, rounded to float32, passes every check with 4x to spare on
every generator) and has teeth (each corrupted solution fails the check that is there to catch it).  No GPU."""
import numpy as np
import pytest

import eigh_ref as E

ORDERS = (8, 9, 64, 65, 129)
_TRUTH = {}


def _case(name, n):
    """(M, Truth), computed once per (generator, order) and never modified."""
    if (name, n) not in _TRUTH:
        M = E.GENERATORS[name](n)
        M.setflags(write=False)
        _TRUTH[name, n] = (M, E.truth(M))
    return _TRUTH[name, n]


_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nrounded float64 LAPACK solution: largest error / bound per check (generator, order):")
        for k in sorted(_WORST):
            r, name, n, note = _WORST[k]
            print(f"  check {k}: {r:.4f}  ({name}, n = {n}, {note})")


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("name", sorted(E.GENERATORS))
def test_generators_are_what_they_say(name, n):
    M, T = _case(name, n)
    assert M.dtype == np.float32 and M.shape == (n, n) and np.array_equal(M, M.T)
    assert np.array_equal(M, E.GENERATORS[name](n)), "seeded and deterministic"
    lam = T.lam_all[::-1]                                    # descending
    N2 = T.norm2
    tight = 16 * E.EPS32 * max(N2, 1e-300)                   # what the float32 rounding of M may split
    if name == "pair":
        assert lam[0] - lam[1] <= tight and lam[1] - lam[2] >= E.GAP * N2
    elif name == "octet":
        assert lam[0] - lam[7] <= tight and (n == 8 or lam[7] - lam[8] >= E.GAP * N2)
    elif name == "straddle":
        hi = min(n, 10) - 1
        assert lam[5] - lam[hi] <= tight and lam[4] - lam[5] >= E.GAP * N2
        assert [g for g in T.groups() if g[0] == 0][0][2] == (0.0 if n > 8 else lam[4] - lam[5])
    elif name == "gaps":
        d = (lam[:-1] - lam[1:])[:6] / N2
        assert abs(d[0] - 1e-6) < 5e-7 and abs(d[2] - 1e-4) < 5e-7 and abs(d[4] - 1e-2) < 5e-7
    elif name == "rank3":
        assert lam[2] >= E.GAP * N2 and np.abs(lam[3:]).max() <= n * E.U64 * N2 * 8 < E.CLAMP
        assert np.array_equal(M[0], np.zeros(n, dtype=np.float32))
    elif name in ("negative", "identity_neg1"):
        assert lam[0] < 0.0
    elif name == "scaled_down":
        assert 0.0 < lam[7] and lam[0] < E.CLAMP
    elif name == "scaled_up":
        assert lam[0] > 1e13
    elif name == "zero":
        assert N2 == 0.0
    elif name == "laplacian":
        assert np.abs(T.lam_all - E.laplacian_eigenvalues(n)).max() <= 8 * n * E.U64 * 4.0
    elif name == "two_blocks":
        assert np.abs(lam[0:8:2] - lam[1:8:2]).max() <= 4 * n * E.U64 * N2 and lam[7] - lam[8 % n] != 0.0
    elif name == "diag_repeats":
        assert np.array_equal(lam[:8], [5, 5, 4, 4, 4, 3, 2, 2])
    if name in ("separated", "negative", "scaled_down", "scaled_up", "diag_distinct"):
        g = T.groups()
        assert len(g) == 8 and all(x[2] >= E.GAP * N2 for x in g), "every kept eigenvalue stands alone: check 7 applies"


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("name", sorted(E.GENERATORS))
def test_checks_are_fair_to_the_rounded_float64_solution(name, n):
    M, T = _case(name, n)
    res = E.check(M, E.reference_solution(M, T), T)
    assert sorted(res) == [1, 2, 3, 4, 5, 6, 7]
    for k, (r, note) in res.items():
        if k not in _WORST or r > _WORST[k][0]:
            _WORST[k] = (r, name, n, note)
        assert r <= 0.25, (k, r, note)


def _rotate(g, T, j, k, theta):
    """Rotate the unit eigenvectors behind columns j, k by theta and scale them as before."""
    out = g.astype(np.float64)
    c = np.sqrt(np.maximum(T.lam, E.CLAMP))
    a, b = out[:, j] / c[j], out[:, k] / c[k]
    out[:, j] = (np.cos(theta) * a + np.sin(theta) * b) * c[j]
    out[:, k] = (-np.sin(theta) * a + np.cos(theta) * b) * c[k]
    # keep the sign rule
    for q in (j, k):
        if out[np.abs(out[:, q]).argmax(), q] < 0.0:
            out[:, q] = -out[:, q]
    return out.astype(np.float32)


N_TEETH = 64


def test_teeth_same_vector_twice_fails_orthonormality():
    M, T = _case("pair", N_TEETH)
    g = E.reference_solution(M, T).copy()
    g[:, 6] = g[:, 7]
    f = E.failed(E.check(M, g, T))
    assert 3 in f and set(f) <= {3, 5}, f              # (5: the pair's subspace has lost a dimension)


def test_teeth_zeroed_clamped_column_fails_the_norm():
    M, T = _case("rank3", N_TEETH)
    assert T.lam[0] < E.CLAMP
    g = E.reference_solution(M, T).copy()
    g[:, 0] = 0.0
    assert E.failed(E.check(M, g, T)) == [2]


def test_teeth_the_ninth_eigenvector_fails_the_residual():
    M, T = _case("separated", N_TEETH)
    g = T.columns()
    v9 = T.vec_all[:, -9]
    v9 = v9 * np.sign(v9[np.abs(v9).argmax()])
    g[:, 0] = v9 * np.sqrt(T.lam[0])
    f = E.failed(E.check(M, g.astype(np.float32), T))
    assert 4 in f and 2 not in f and 3 not in f and 6 not in f, f    # (5 and 7 follow from 4: wrong subspace, wrong column)


def test_teeth_negated_column_fails_the_sign_rule():
    M, T = _case("pair", N_TEETH)
    g = E.reference_solution(M, T).copy()
    g[:, 3] = -g[:, 3]
    assert E.failed(E.check(M, g, T)) == [6]
    M, T = _case("separated", N_TEETH)                 # where columns are compared directly, that notices too
    g = E.reference_solution(M, T).copy()
    g[:, 3] = -g[:, 3]
    assert E.failed(E.check(M, g, T)) == [6, 7]


def test_teeth_one_nan_fails_finiteness():
    M, T = _case("separated", N_TEETH)
    g = E.reference_solution(M, T).copy()
    g[17, 2] = np.nan
    assert E.failed(E.check(M, g, T)) == [1]


def test_rotation_inside_the_straddling_cluster_is_legitimate():
    M, T = _case("straddle", N_TEETH)
    g = E.reference_solution(M, T)
    for j, k in ((0, 1), (1, 2), (0, 2)):              # lambda_8, lambda_7, lambda_6: all inside the cluster 6 .. 10
        g = _rotate(g, T, j, k, 0.7)
    res = E.check(M, g, T)
    assert E.failed(res) == [], res
    # and with a vector of the dropped part of the cluster (lambda_9) rotated in
    T9 = T.vec_all[:, -9]
    out = g.astype(np.float64)
    c0 = np.sqrt(T.lam[0])
    out[:, 0] = np.cos(0.7) * out[:, 0] + np.sin(0.7) * T9 * c0
    if out[np.abs(out[:, 0]).argmax(), 0] < 0.0:
        out[:, 0] = -out[:, 0]
    res = E.check(M, out.astype(np.float32), T)
    assert E.failed(res) == [], res


def test_teeth_rotation_across_a_real_gap_fails_the_subspace():
    M, T = _case("gaps", N_TEETH)
    g = E.reference_solution(M, T)
    inside = E.check(M, _rotate(g, T, 6, 7, 0.7), T)    # lambda_1, lambda_2: 1e-6 apart, one subspace
    assert E.failed(inside) == [], inside
    across = E.check(M, _rotate(g, T, 3, 4, 0.7), T)    # lambda_5 | lambda_4: 0.3 ||M|| apart
    f = E.failed(across)
    assert 5 in f and set(f) <= {4, 5}, f              # (4 necessarily: Davis-Kahan bounds 5 by 4)
    # the smallest rotation that check 5 is derived to see
    tiny = E.check(M, _rotate(g, T, 3, 4, 1e-3), T)
    assert 5 in E.failed(tiny)
