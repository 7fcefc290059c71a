"""Float64 references and inputs of the alignment-depth sweep (tests/test_gpu_depths.py), checked on the CPU by
tests/test_depth_ref_cpu.py.

References, written out from the formulas of oracle/dmpfold_oracle.py (fast_dca, gru_manual) in float64:
  dca(aln, w)        -> cov_reg, inv_cov, contacts of fast_dca
  dca_features(...)  -> the same in fast_dca's (L, L, 442) layout
  vgru(W, aln)       -> the last row of the two-layer vertical GRU (time = alignment rows, batch = columns)

Inputs:
  depth_msa(L, N, seed)   synth.synth_msa rows with redundancy, so that the sequence weights are not all 1: exact
                          duplicates of row 0, near-duplicates of row 1, the LAST row always in a cluster; codes 20
                          (unknown) and 21 (gap) both occur and have to compare equal for the clusters to hold
  threshold_msa(L)        130 unrelated rows with four hand-built pairs that agree in exactly floor(0.8 L) positions
                          (not neighbours: the comparison is strict, also where 0.8 L is an integer) and in
                          floor(0.8 L) + 1 positions (neighbours), one of each inside a 64-row tile and one of each
                          across the boundary between two tiles
"""
import numpy as np
import torch

import dmpfold_oracle as O

NS = 21

# ---------------------------------------------------------------------------------------------------- the sweep
# every depth at which a front-end kernel takes another path: the GEMM's K tail (N % 16), its one-level accumulation
# (N <= 256) and first / second flush (257, 512 / 513), the 64-row tiles of the reweighting, the 256-thread loops of the
# covariance's reductions, the vertical GRU's parity (N & 1), its 16-row graphs (N + 1 = 16 / 17, 144 / 145) and
# 128-row chunks (N + 1 = 128 / 129, 256 / 257 / 258)
DEPTHS = [2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 143, 144, 145, 255, 256, 257, 272, 273, 511, 512, 513,
          769]
LENGTHS = [13, 33]        # D = 273: three Gauss-Jordan blocks, one GRU column tile; D = 693: two column tiles (32 + 1)
GRU_MAX_DEPTH = 257
GROUP_SHAPES = [(33, 127), (33, 128), (9, 129), (40, 1), (17, 2), (13, 16)]          # (L, N)
PREDICT_SHAPES = [(17, 2), (17, 3), (17, 17), (17, 129), (40, 127), (40, 128), (40, 255), (40, 257)]
REUSE_DEEP = (40, 300)
REUSE_LENGTH, REUSE_DEPTHS = 33, [1, 2, 17, 65, 129]


def seed_of(L, N):
    return 5000 + 1000 * L + N



# ---------------------------------------------------------------------------------------------------- references
def dca(alnmat, w, penalty=4.5):
    """predict.py:41-61 in float64, from the float32 weights `w`: (cov_reg (D, D), inv_cov (D, D), contacts (L, L))."""
    a = np.minimum(np.asarray(alnmat), 20).astype(np.int64)
    n, L = a.shape
    D = L * NS
    w = torch.as_tensor(np.asarray(w, dtype=np.float64))
    x = torch.zeros(n, D, dtype=torch.float64)
    x[torch.arange(n)[:, None], torch.arange(L)[None, :] * NS + torch.from_numpy(a)] = 1.0
    neff = w.sum()
    num_points = neff - torch.sqrt(w.mean())
    mean = (x * w[:, None]).sum(dim=0, keepdim=True) / num_points
    xc = (x - mean) * torch.sqrt(w)[:, None]
    cov_reg = xc.t() @ xc / num_points + torch.eye(D, dtype=torch.float64) * (penalty / torch.sqrt(neff))
    inv_cov = torch.linalg.inv(cov_reg)
    blocks = inv_cov.view(L, NS, L, NS)
    off = 1.0 - torch.eye(L, dtype=torch.float64)
    norms = torch.sqrt((blocks[:, :-1, :, :-1] ** 2).sum(dim=(1, 3))) * off
    apc = norms.sum(dim=0, keepdim=True) * norms.sum(dim=1, keepdim=True) / norms.sum()
    return cov_reg, inv_cov, (norms - apc) * off


def dca_features(inv_cov, contacts):
    """fast_dca's return value: channel 21a+b of pair (i, j) is inv_cov[21i+a, 21j+b], channel 441 the contacts."""
    L = contacts.shape[0]
    return torch.cat((inv_cov.view(L, NS, L, NS).transpose(1, 2).reshape(L, L, NS * NS), contacts[:, :, None]), dim=2)


def vgru(W, alnmat):
    """The vertical GRU (network.py:223-224: embedding, two layers, hidden 512, h0 = 0) over the rows of the alignment
    in float64; the state of the second layer after the last row, (L, 512).
        r = s(W_ir x + b_ir + W_hr h + b_hr);  z likewise
        n = tanh(W_in x + b_in + r * (W_hn h + b_hn));  h' = (1 - z) n + z h"""
    idx = torch.from_numpy(np.asarray(alnmat).astype(np.int64))
    inp = W["embed.weight"].double()[idx]                       # (N, L, 22)
    for layer in range(2):
        wih, whh = W[f"vgru.weight_ih_l{layer}"].double(), W[f"vgru.weight_hh_l{layer}"].double()
        bih, bhh = W[f"vgru.bias_ih_l{layer}"].double(), W[f"vgru.bias_hh_l{layer}"].double()
        H = whh.shape[1]
        gi_all = inp @ wih.t() + bih
        h = torch.zeros(inp.shape[1], H, dtype=torch.float64)
        out = torch.empty(inp.shape[0], inp.shape[1], H, dtype=torch.float64)
        for t in range(inp.shape[0]):
            gi, gh = gi_all[t], h @ whh.t() + bhh
            r = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (1.0 - z) * n + z * h
            out[t] = h
        inp = out
    return inp[-1]


# ---------------------------------------------------------------------------------------------------- inputs
def _other(code, k):
    """a standard residue different from `code` (and from class 20)"""
    return np.uint8((min(int(code), 20) + 1 + k % 19) % 20) if code < 20 else np.uint8(k % 20)


def depth_msa(L, N, seed):
    """(N, L) uint8 codes.  Row 0 is synth_msa's query (standard residues only).
      N = 1   the query alone
      N = 2   row 1 = row 0 with code 20 at position 3 and code 21 at position 4 (L - 2 of L agree)
      N = 3   row 1 carries codes 20 / 21, row 2 is a near-duplicate of row 1
      N >= 4  rows 2, N // 2, N - 2 are exact duplicates of row 0; rows 3, 2 N // 3, N - 1 are near-duplicates of row 1
    Row 1 has code 20 at position 3 and code 21 at position 4; its near-duplicates have them the other way round and
    one more position changed to another residue (L - 1 of L agree, L - 2 between two of them - if 20 and 21 did not
    compare equal it would be L - 3 and L - 4, below 0.8 L at L = 13).  L >= 9."""
    from dmpfold2_amd import synth
    a = np.array(O.encode_aln(synth.synth_msa(L, N, seed)))
    assert L >= 9 and a.shape == (N, L)
    if N == 1:
        return a
    if N == 2:
        a[1] = a[0]
    a[1, 3], a[1, 4] = 20, 21
    if N >= 4:
        for n in sorted({2, N // 2, N - 2}):
            a[n] = a[0]
    for k, n in enumerate(sorted({3, 2 * N // 3, N - 1}) if N >= 4 else ([2] if N == 3 else [])):
        a[n] = a[1]
        a[n, 3], a[n, 4] = 21, 20
        p = (5 + k) % L
        a[n, p] = _other(a[1, p], k)
    assert (a == 20).any() and (a == 21).any() and (a[0] < 20).all()
    return a


THRESHOLD_LENGTHS = [5, 8, 9, 10, 13, 15, 16, 17, 20]
THRESHOLD_ROWS = 130
# (row, row, agreeing positions beyond floor(0.8 L)): two pairs inside the first 64-row tile, two across rows 63 | 64
THRESHOLD_PAIRS = [(10, 11, 0), (20, 21, 1), (63, 64, 0), (62, 65, 1)]


def threshold_msa(L, seed=0):
    """(130, L) codes: rows uniform over the 20 residues (unrelated: about L / 20 agreements), except the pairs of
    THRESHOLD_PAIRS, which agree in exactly floor(0.8 L) + extra positions; the first agreeing position holds code 20 in
    one row and 21 in the other.  Returns (codes, pairs)."""
    rng = np.random.Generator(np.random.Philox(key=0xDE97 + 131 * L + seed))
    a = rng.integers(0, 20, size=(THRESHOLD_ROWS, L)).astype(np.uint8)
    m0 = (4 * L) // 5
    for k, (r, s, extra) in enumerate(THRESHOLD_PAIRS):
        agree = m0 + extra
        order = rng.permutation(L)
        a[s] = a[r]
        a[r, order[0]], a[s, order[0]] = (20, 21) if k % 2 == 0 else (21, 20)
        for p in order[agree:]:
            a[s, p] = _other(a[r, p], int(p) + k)
        assert int((np.minimum(a[r], 20) == np.minimum(a[s], 20)).sum()) == agree
    return a, THRESHOLD_PAIRS
