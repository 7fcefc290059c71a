"""The float64 references and the inputs of the alignment-depth sweep (tests/depth_ref.py) on the CPU: the oracle's float32
fast_dca and nn.GRU against them at every (L, N) of the sweep, so that what tests/test_gpu_depths.py holds the kernels to
is itself right, and so that the bounds used there (1e-5 of scale for the covariance features, 3e-6 for the float32
vertical GRU) leave the reference several times its own error.

Bounds are the measured worst value x 2.  Measured (float32 oracle against float64, depth_msa rows):
  cov_reg    8.7e-07 of max(1, |ref|max)   at L = 33, N = 769
  inv_cov    1.1e-06                       at L = 33, N = 257
  contacts   6.5e-07                       at L = 33, N = 769
  vertical GRU, last row   4.0e-08 absolute (|h|max = 0.12)   at L = 33, N = 144
The condition number of cov_reg is at most 143 (L = 33, N = 2: two rows of one cluster, num_points = 1 - sqrt(1/2));
from N = 15 on it is below 20.  The hand-written float64 recurrence and nn.GRU(...).double() agree to 5e-17.
"""
import numpy as np
import pytest
import torch

import dmpfold_oracle as O
import depth_ref as DR

DCA_SHAPES = ([(L, N) for L in DR.LENGTHS for N in DR.DEPTHS] + [s for s in DR.PREDICT_SHAPES if s[1] > 1]
              + [(DR.REUSE_LENGTH, N) for N in DR.REUSE_DEPTHS if N > 1])
GRU_SHAPES = ([(L, N) for L in DR.LENGTHS for N in [1] + DR.DEPTHS if N <= DR.GRU_MAX_DEPTH] + DR.GROUP_SHAPES
              + [(DR.REUSE_LENGTH, N) for N in DR.REUSE_DEPTHS])
BOUNDS = {"cov_reg": 1.8e-6, "inv_cov": 2.3e-6, "contacts": 1.3e-6, "gru": 8.1e-8}


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def test_oracle_fast_dca_against_the_float64_formula_over_the_depth_sweep():
    worst = {}
    for L, N in DCA_SHAPES:
        a = DR.depth_msa(L, N, DR.seed_of(L, N))
        w = O.reweight(a)
        cap = {}
        f = O.fast_dca(a, w, capture=cap)
        cov, inv, con = DR.dca(a, w)
        for k, ref in (("cov_reg", cov), ("inv_cov", inv), ("contacts", con)):
            d = _rel(cap[k], ref)
            if d > worst.get(k, (0.0,))[0]:
                worst[k] = (d, L, N)
        assert _rel(f, DR.dca_features(inv, con)) <= BOUNDS["inv_cov"], (L, N)          # the (L, L, 442) layout
    print("oracle fast_dca vs float64 (of scale, at L, N):", worst)
    for k, (d, L, N) in worst.items():
        assert d <= BOUNDS[k], (k, d, L, N)


def test_oracle_vertical_gru_against_the_float64_recurrence_over_the_depth_sweep(oracle_weights):
    W = oracle_weights
    worst = (0.0, 0, 0)
    for L, N in GRU_SHAPES:
        a = DR.depth_msa(L, N, DR.seed_of(L, N))
        ref = O._gru(W, "vgru", W["embed.weight"][torch.from_numpy(a.astype(np.int64))], 22, 512, 2, False, False)[-1]
        d = float((ref.double() - DR.vgru(W, a)).abs().max())
        worst = max(worst, (d, L, N))
    print("oracle nn.GRU vs the float64 recurrence (absolute, at L, N):", worst)
    assert worst[0] <= BOUNDS["gru"], worst


def test_float64_recurrence_is_nn_gru_in_double(oracle_weights):
    W = oracle_weights
    g64 = torch.nn.GRU(22, 512, num_layers=2).double().eval()
    g64.load_state_dict({k[5:]: v.double() for k, v in W.items() if k.startswith("vgru.")})
    for L, N in [(13, 1), (13, 2), (33, 17)]:
        a = DR.depth_msa(L, N, DR.seed_of(L, N))
        with torch.no_grad():
            want = g64(W["embed.weight"][torch.from_numpy(a.astype(np.int64))].double())[0][-1]
        assert float((DR.vgru(W, a) - want).abs().max()) <= 1e-15, (L, N)


@pytest.mark.parametrize("L", DR.LENGTHS + [9, 17, 40])
def test_depth_msa_has_clusters_and_both_gap_codes(L):
    # (at L = 9 two rows that differ in two positions are no neighbours: 7 < 7.2; the sweep has no such shape)
    for N in ([2, 3] if L > 10 else []) + [n for n in DR.DEPTHS if n >= 15][:: 4 if L > 13 else 1] + [769]:
        a = DR.depth_msa(L, N, DR.seed_of(L, N))
        w = O.reweight(a)
        assert w[N - 1] < 1.0, (L, N)                                  # the last row belongs to a cluster
        assert (a == 20).any() and (a == 21).any() and (a[0] < 20).all()
        if N >= 15:
            assert w[0] <= 0.25 and w[N // 2] == w[0] and w[1] <= 0.25, (L, N, w[:4])
            assert L < 10 or w[N - 1] <= 0.25, (L, N, w[N - 1])        # (two near-duplicates agree in L - 2 positions)
            assert len(np.unique(w)) >= 2, (L, N)                      # ... and not every row has the same weight
        # were codes 20 and 21 different classes, row 1 would lose its near-duplicates at L = 13
        if L == 13 and N >= 3:
            b = np.where(a == 21, 22, a)
            assert (b[1] == b[N - 1]).sum() <= 0.8 * L < (np.minimum(a[1], 20) == np.minimum(a[N - 1], 20)).sum()


@pytest.mark.parametrize("L", DR.THRESHOLD_LENGTHS)
def test_threshold_family_sits_on_both_sides_of_the_cutoff(L):
    a, pairs = DR.threshold_msa(L)
    w = O.reweight(a)
    m0 = (4 * L) // 5
    assert np.float32(m0) <= np.float32(L * 0.8) < np.float32(m0 + 1)
    assert (np.float32(m0) == np.float32(L * 0.8)) == (L % 5 == 0)     # equality occurs, and must not count
    for r, s, extra in pairs:
        eq = int((np.minimum(a[r], 20) == np.minimum(a[s], 20)).sum())
        assert eq == m0 + extra
        assert w[r] == w[s] == (0.5 if extra else 1.0), (L, r, s, w[r], w[s])
    assert int((w < 1).sum()) == 4                                     # nothing else is a neighbour of anything
    assert {(r // 64, s // 64) for r, s, _ in pairs} == {(0, 0), (0, 1)}
