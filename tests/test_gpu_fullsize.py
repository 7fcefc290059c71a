"""HIP path at BASELINE.json's full sizes.

The oracle does not finish in seconds at these sizes, so the checks are (a) the oracle on the
stages it can still do, (b) independent implementations of single stages (PyTorch-ROCm operators
on the same GPU: integer counting, F.conv2d, nn.GRU - checkers only, never the product path),
(c) size-independent properties: A A^-1 = I, truncation at 3000 rows, run-to-run determinism,
scheduler == single engine.

  configs[1]  L=200, N=1000, 10 + 100        oracle-checked prefix (2 recycling iterations, m = 0)
  metric      L=300, N=2000, 10 + 100        stage checks + determinism + scheduler equality
  configs[2]  L=500, N=5000 (-> 3000), 30+200   truncation property, finite outputs
  configs[4]  L=1000, N=2000, 100 + 1000     runs within the context capacity, finite outputs
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ca_rmsd

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure)


def _msa(L, N, seed):
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import encode_aln
    return encode_aln(synth.synth_msa(L, N, seed=seed))


@pytest.fixture(scope="module")
def ns(synth_sd):
    """One context of the north-star capacity, shared by the stage checks."""
    from abi import Stages
    st = Stages(synth_sd, max_L=300, max_N=2000)
    yield st
    st.eng.sync_check()
    st.eng.close()


@pytest.fixture(scope="module")
def ns_msa():
    return _msa(300, 2000, 4242)


def test_ns_msa_weights_bit_exact(ns, ns_msa):
    """reweight at N=2000, L=300 against an integer count done with torch on the GPU."""
    w = ns.msa_weights(ns_msa).cpu().numpy()
    m = torch.from_numpy(np.minimum(ns_msa, 20)).cuda()
    counts = torch.zeros(m.shape[0], dtype=torch.int64, device="cuda")
    thr = np.float32(m.shape[1] * 0.8)
    for lo in range(0, m.shape[0], 250):
        same = (m[lo:lo + 250, None, :] == m[None, :, :]).sum(-1).to(torch.float32)
        counts[lo:lo + 250] = (same > float(thr)).sum(-1)
    ref = (1.0 / counts.to(torch.float32)).cpu().numpy()
    assert np.array_equal(w, ref)


def test_ns_covariance_inverse_identity(ns, ns_msa):
    """fast_dca at D = 6300: covariance against the oracle's formula evaluated with torch on the
    GPU, and cov @ inverse = I."""
    w = ns.msa_weights(ns_msa)
    cov = ns.cov_build(ns_msa, w)
    N, L = ns_msa.shape
    x = F.one_hot(torch.from_numpy(np.minimum(ns_msa, 20).astype(np.int64)).cuda(), 21).float().reshape(N, 21 * L)
    S = w.sum()
    num = S - torch.sqrt(w.mean())
    mean = (x * w[:, None]).sum(0, keepdim=True) / num
    xc = (x - mean) * torch.sqrt(w)[:, None]
    ref = (xc.double().t() @ xc.double() / num.double()).float()
    ref += torch.eye(21 * L, device="cuda") * (4.5 / torch.sqrt(S))
    assert float((cov - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    inv = ns.spd_inverse(cov)
    resid = (cov.double() @ inv.double() - torch.eye(21 * L, device="cuda", dtype=torch.float64)).abs().max()
    assert float(resid) < 5e-4
    assert float((inv - inv.t()).abs().max()) <= 1e-4 * float(inv.abs().max())


def _gru_recurrence(ns_msa, synth_sd, dtype):
    """The vertical GRU (network.py:189; ATen gru_cell: h' = (h - n) z + n) written out with torch matmuls in `dtype` on
    the GPU: the last row's hidden state of the second layer, (300, 512)."""
    W = {k: torch.from_numpy(np.array(v)).cuda().to(dtype) for k, v in synth_sd.items() if k.startswith(("vgru.", "embed."))}
    codes = torch.from_numpy(ns_msa.astype(np.int64)).cuda()
    h = [torch.zeros(ns_msa.shape[1], 512, dtype=dtype, device="cuda") for _ in range(2)]
    for t in range(ns_msa.shape[0]):
        x = W["embed.weight"][codes[t]]
        for l in range(2):
            gi = x @ W[f"vgru.weight_ih_l{l}"].t() + W[f"vgru.bias_ih_l{l}"]
            gh = h[l] @ W[f"vgru.weight_hh_l{l}"].t() + W[f"vgru.bias_hh_l{l}"]
            r = torch.sigmoid(gi[:, :512] + gh[:, :512])
            z = torch.sigmoid(gi[:, 512:1024] + gh[:, 512:1024])
            n = torch.tanh(gi[:, 1024:] + r * gh[:, 1024:])
            h[l] = (h[l] - n) * z + n
            x = h[l]
    return h[1].double()


@pytest.fixture(scope="module")
def ns_gru_refs(ns_msa, synth_sd):
    """(float64 recurrence, distance of the same recurrence in float32 matmuls from it), once per module."""
    h64 = _gru_recurrence(ns_msa, synth_sd, torch.float64)
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        h32 = _gru_recurrence(ns_msa, synth_sd, torch.float32)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    return h64, float((h32 - h64).abs().max())


@pytest.mark.parametrize("form", [0, 1, 2])
def test_ns_gru_vertical_vs_torch_gru(ns, ns_msa, ns_gru_refs, form):
    """2000 recurrent steps x 300 columns - the headline's depth - against the GRU recurrence in float64 on the GPU, in
    each form of the vertical GRU (option vgru_f32): 0 the split-f16 products, 1 float32 MFMAs (vgru_f32.hip), 2
    full-width operands on the bf16 matrix cores (vgru_x3.hip, the headline).  The float32 forms are held to the
    distance of a float32 evaluation of the same recurrence (torch matmuls, no TF32) from float64."""
    h64, err_f32 = ns_gru_refs
    ns.eng.set_option("vgru_f32", form)
    try:
        assert ns.eng.get_option("vgru_f32") == form
        out = ns.gru_vertical(ns_msa)
        ns.eng.sync_check()
        err = float((out.double() - h64).abs().max())
    finally:
        ns.eng.set_option("vgru_f32", 0)
    print(f"vertical GRU form {form}: max |dev| from float64 {err:.3e} (torch float32 {err_f32:.3e})")
    if form == 0:
        assert err < 2e-5
    else:
        assert err <= 2.0 * err_f32 + 1e-7, (err, err_f32)


@pytest.mark.parametrize("mode", [0, 2])
def test_ns_conv_block_vs_conv2d(ns, synth_sd, mode):
    """One residual-block convolution at L = 300 against F.conv2d + maxout (float64 on the GPU)."""
    ns.eng.set_option("conv_mode", mode)
    try:
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.randn(128, 300, 300, device="cuda", generator=g) * 3.0
        u, st = ns.conv(5, x)
        w = torch.from_numpy(np.array(synth_sd["resnet.5.layer1.lin.weight"])).cuda().double()
        b = torch.from_numpy(np.array(synth_sd["resnet.5.layer1.lin.bias"])).cuda().double()
        ref = torch.empty(128, 300, 300, dtype=torch.float64, device="cuda")
        for lo in range(0, 300, 50):             # rows lo..lo+49: im2col slab (3200 x 15000) in float64
            xp = F.pad(x.double(), (2, 2, 2, 2))[:, lo:lo + 54]
            cols = F.unfold(xp[None], 5)[0]                                   # (128*25, 50*300)
            y = (w.reshape(512, 3200) @ cols + b[:, None]).reshape(128, 4, 50, 300)
            ref[:, lo:lo + 50] = y.max(1)[0]
        scale = float(ref.abs().max())
        assert float((u.double() - ref).abs().max()) <= 1e-5 * scale
        assert float((st[:, 0] - ref.sum((1, 2))).abs().max()) <= 1e-5 * float(ref.abs().sum((1, 2)).max())
    finally:
        ns.eng.set_option("conv_mode", 0)


def test_ns_end_to_end_deterministic_and_scheduler_equal(ns, ns_msa, synth_sd):
    """The north-star prediction twice on one engine, and through the 3-engine scheduler: same bits."""
    from dmpfold2_amd.predict import Pipeline
    # like with like: the scheduler's engines tridiagonalise with one launch per Householder step; the lone engine's
    # cluster launch is the same algorithm with float64 sums associated differently - the same float32 bits on almost
    # every matrix, not on all (round 4: a benchmark target's minimised trace told them apart)
    ns.eng.set_option("tridiag_cluster", 0)
    c1, f1 = ns.eng.predict(ns_msa, None, 10, 100)
    c2, f2 = ns.eng.predict(ns_msa, None, 10, 100)
    ns.eng.sync_check()
    assert torch.equal(c1, c2) and torch.equal(f1, f2)
    assert bool(torch.isfinite(c1).all()) and bool(torch.isfinite(f1).all())
    assert float(f1.min()) >= 0.0 and float(f1.max()) <= 1.0
    dev = torch.device("cuda:0")
    pipe = Pipeline(dev, 300, 2000, synth_sd, streams=3)
    other = _msa(300, 2000, 99)
    d_a, d_b = torch.from_numpy(ns_msa).to(dev), torch.from_numpy(other).to(dev)
    res = pipe.run([d_a, d_b, d_a, d_b, d_a], 10, 100)
    pipe.sync_check()
    cb, fb = ns.eng.predict(other, None, 10, 100)
    ns.eng.sync_check()
    same = [bool(torch.equal(res[i][0], c1 if i % 2 == 0 else cb)) and
            bool(torch.equal(res[i][1], f1 if i % 2 == 0 else fb)) for i in range(5)]
    dev_max = [float((res[i][0] - (c1 if i % 2 == 0 else cb)).abs().max()) for i in range(5)]
    ns.eng.set_option("tridiag_cluster", 1)
    pipe.close()
    assert all(same), (same, dev_max)


def test_config1_L200_N1000_prefix_vs_oracle(synth_sd, oracle_weights):
    """configs[1] (L=200, N=1000): the oracle is affordable for 2 recycling iterations without the
    minimiser; the full 10 + 100 run must then be finite and deterministic."""
    from abi import Stages
    msa = _msa(200, 1000, 11)
    st = Stages(synth_sd, max_L=200, max_N=1000)
    coords, confs = st.eng.predict(msa, None, 2, 0)
    st.eng.sync_check()
    rc, rf = O.predict(msa, oracle_weights, None, 2, 0, "canonical")
    assert ca_rmsd(coords.cpu().numpy()[:, 1], np.asarray(rc)[:, 1]) <= 1e-3
    assert np.abs(confs.cpu().numpy() - np.asarray(rf)).max() < 1e-4
    a = st.eng.predict(msa, None, 10, 100)
    b = st.eng.predict(msa, None, 10, 100)
    st.eng.sync_check()
    assert torch.equal(a[0], b[0]) and bool(torch.isfinite(a[0]).all())
    st.eng.close()


def test_config2_deep_msa_truncated_at_3000_rows(synth_sd, tmp_path, weights_file):
    """configs[2] (L=500, N=5000, 30 + 200): the alignment is cut to its first 3000 rows
    (predict.py:130-132), so the result equals that of the 3000-row alignment."""
    from dmpfold2_amd import aln_to_coords, synth
    rows = synth.synth_msa(500, 5000, seed=5)
    full, cut = tmp_path / "deep.aln", tmp_path / "cut.aln"
    synth.write_aln(str(full), rows)
    synth.write_aln(str(cut), rows[:3000])
    c1, f1 = aln_to_coords(str(full), device="cuda:0", iterations=30, minsteps=200, weights_file=weights_file)
    c2, f2 = aln_to_coords(str(cut), device="cuda:0", iterations=30, minsteps=200, weights_file=weights_file)
    assert c1.shape == (500, 5, 3) and f1.shape == (500,)
    assert torch.equal(c1, c2) and torch.equal(f1, f2)
    assert bool(torch.isfinite(c1).all()) and bool(torch.isfinite(f1).all())


def test_config4_L1000_long_recycling(synth_sd):
    """configs[4] (L=1000, N=2000, 100 iterations + 1000 minimiser steps) on one context."""
    from dmpfold2_amd.predict import Engine
    eng = Engine("cuda:0", 1000, 2000)
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()})
    assert eng.device_bytes < 16e9
    msa = _msa(1000, 2000, 3)
    coords, confs = eng.predict(msa, None, 100, 1000)
    eng.sync_check()
    assert coords.shape == (1000, 5, 3)
    assert bool(torch.isfinite(coords).all()) and bool(torch.isfinite(confs).all())
    eng.close()


def test_embedding_is_folded_into_the_input_weights(synth_sd, oracle_weights):
    """embed.weight is part of the state_dict (network.py:188 freezes it to the identity): a
    different matrix must still give the reference's x = embed[code] semantics."""
    from abi import Stages
    rng = np.random.default_rng(3)
    sd = dict(synth_sd)
    sd["embed.weight"] = (np.eye(22) + 0.3 * rng.standard_normal((22, 22))).astype(np.float32)
    ow = dict(oracle_weights)
    ow["embed.weight"] = torch.from_numpy(sd["embed.weight"])
    msa = _msa(40, 60, 8)
    st = Stages(sd, max_L=64, max_N=64)
    out = st.gru_vertical(msa).cpu().numpy()
    idx = torch.from_numpy(msa.astype(np.int64))
    v = O._gru(ow, "vgru", ow["embed.weight"][idx], 22, 512, 2, False, False)[-1].numpy()
    assert np.abs(out - v).max() < 1e-5
    st.eng.close()


def test_eigensolver_at_the_largest_order(synth_sd):
    """max_L = DMP_MAX_L = 2048.  The eigensolver's kernels are instantiated per range of the order: up to 384 the
    inverse iteration's vectors AND LU factors live in LDS (157 KB at 384), up to 1280 the vectors (112 640 bytes), above
    that the vectors are in global memory (all need the dynamic-LDS opt-in set at context creation); the Householder
    step holds 5 x 256 rows per thread block up to 1280 and 8 x 256 above.  Both sides of every boundary.  A
    distance-geometry Gram matrix of a 3-D random walk plus noise against the float64 solution."""
    from abi import Stages
    st = Stages(synth_sd, max_L=2048, max_N=4)
    try:
        rng = np.random.default_rng(17)
        for L in (2048, 1537, 1281, 1280, 1000, 640, 513, 385, 384, 300):
            P = np.cumsum(rng.standard_normal((L, 3)) * 2.2, axis=0)
            D = np.linalg.norm(P[:, None] - P[None], axis=2) + np.abs(rng.standard_normal((L, L))) * 0.3
            D = 0.5 * (D + D.T)
            M = (0.5 * (D[0:1, :] ** 2 + D[:, 0:1] ** 2 - D ** 2)).astype(np.float32)
            got = st.eigh_top8(st.to(M)).cpu().numpy().astype(np.float64)
            st.eng.sync_check()
            Mu = np.triu(M.astype(np.float64)) + np.triu(M.astype(np.float64), 1).T      # upper triangle is used
            lam, vec = np.linalg.eigh(Mu)
            vec = vec[:, -8:] * np.sign(vec[np.abs(vec[:, -8:]).argmax(axis=0), np.arange(L - 8, L)])
            truth = vec * np.sqrt(np.maximum(lam[-8:], 1e-8))
            assert np.abs(got - truth).max() <= 2e-5 * np.abs(truth).max(), L
    finally:
        st.eng.close()


def test_cluster_tridiagonalisation_is_bitwise_the_per_step_launches(synth_sd):
    """Orders up to 640 run every Householder step in ONE launch on a cluster of 32 workgroups of one XCD (rows in LDS,
    products and pivot row handed over per step as granules; option tridiag_cluster, default 1).  It repeats the
    per-step launches operation for operation except for the association of the float64 partial sums: on these
    full-rank (noisy) distance matrices the float32 MDS coordinates are the same bits.  (On rank-deficient Gram
    matrices the near-null columns of the eight can differ in their last bits: tools/eigh_variants_bits.py.)  Orders
    below, at and above the cluster size, partial last row slots, the largest order."""
    from abi import Stages
    st = Stages(synth_sd, max_L=640, max_N=4)
    try:
        rng = np.random.default_rng(23)
        for L in (8, 31, 32, 33, 82, 255, 300, 513, 640):
            P = np.cumsum(rng.standard_normal((L, 3)) * 2.2, axis=0)
            D = np.linalg.norm(P[:, None] - P[None], axis=2) + np.abs(rng.standard_normal((L, L))) * 0.3
            D = 0.5 * (D + D.T)
            M = st.to((0.5 * (D[0:1, :] ** 2 + D[:, 0:1] ** 2 - D ** 2)).astype(np.float32))
            outs = []
            for mode in (0, 1, 1):
                st.eng.set_option("tridiag_cluster", mode)
                outs.append(st.eigh_top8(M).clone())
                st.eng.sync_check()
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2]), L
    finally:
        st.eng.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("name", ["synth_L200_N1000_n10_m0", "synth_L500_N5000_n1_m0", "synth_L1000_N2000_n0_m0"])
def test_baseline_config_sizes_vs_reference(synth_sd, name, precision):
    """The single-target configurations of BASELINE.json at their own sizes against outputs of the reference
    itself (tests/golden/make_goldens.py; minimiser off - it is chaotic on random weights): configs[1]
    L=200, N=1000, 10 iterations; configs[2] L=500, N=5000 (cut to 3000 rows), 1 iteration; configs[4]
    L=1000, N=2000, first pass.  The alignments are regenerated from their seeds (SHA-256 in the fixture).
    A fixture that has not been generated yet is skipped."""
    import hashlib
    import os
    from conftest import GOLDEN, load_golden
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, encode_aln
    if not os.path.exists(os.path.join(GOLDEN, name + ".npz")):
        pytest.skip("fixture not generated: " + name)
    g = load_golden(name)
    L = g["coords"].shape[0]
    alnmat = encode_aln(synth.synth_msa(L, int(g["msa_rows"]), int(g["msa_seed"])))
    assert hashlib.sha256(alnmat.tobytes()).hexdigest() == bytes(g["alnmat_sha256"]).decode()
    n = int(g["iterations"])
    eng = Engine("cuda:0", L, alnmat.shape[0])
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()})
    eng.set_option("precision", precision)
    try:
        coords, confs = eng.predict(alnmat, None, n, 0)
        eng.sync_check()
        P = n + 1
        ca_pass = eng.fetch("ca_pass", P * L * 3).cpu().numpy().reshape(P, L, 3)
        # floors of the reference itself: thread-count noise per pass, and how far its float32 LAPACK
        # eigenvectors are from the exact ones of its own Gram matrix (1.8e-3 A at L=1000, where two of the
        # top eight eigenvalues are 3e-4 apart; the HIP solver works in float64)
        eig = float(g["noise_eig_ca_rmsd"]) if "noise_eig_ca_rmsd" in g else 0.0
        floor = np.maximum(g["noise_ca_pass"], eig)
        dev = np.array([ca_rmsd(ca_pass[p], g["ca_pass"][p]) for p in range(P)])
        assert (dev <= np.maximum(1e-3, 3.0 * floor)).all(), (dev, floor)
        means = eng.fetch("conf_means", P).cpu().numpy()
        assert np.abs(means - g["conf_mean_pass"]).max() < 1e-3
        final = ca_rmsd(coords.cpu().numpy()[:, 1], g["coords"][:, 1])
        dconf = float(np.abs(confs.cpu().numpy() - g["confs"]).max())
        print(name, "precision", precision, "per-pass CA-RMSD", dev, "final", final, "max|dconf|", dconf)
        if name == "synth_L1000_N2000_n0_m0":
            # the documented ill-conditioned case (two of the top eight MDS eigenvalues 3e-4 apart: the reference's
            # float32 LAPACK eigenvectors are 1.8e-3 A from the exact ones of its own matrix); the well-separated
            # L=1000 fixture below holds the plain tolerance
            assert final <= max(1e-3, 3.0 * max(float(g["noise_ca_rmsd"]), eig))
        else:
            assert final <= 1e-3                       # the output of aln_to_coords: plain north-star tolerance
        # confidences: the plain tolerance where the reference's OWN thread-count spread allows it - on the L = 200
        # fixture (eleven passes) its 8- and 4-thread runs are 8.0e-5 apart, and the float32-MFMA setting lands 1.5e-4
        # from the 8-thread run (round 6: the test used to run in the fast mode only, which lands below 1e-4)
        assert dconf < max(1e-4, 3.0 * float(g["noise_conf"])), (dconf, float(g["noise_conf"]))
    finally:
        eng.close()


def test_config4_L1000_well_separated_spectrum_vs_reference(synth_sd):
    """configs[4] (L=1000, N=2000) on a fixture whose top MDS eigenvalues are well separated in BOTH passes
    (alignment seed 0 chosen by tools/screen_eig_gaps.py: smallest relative gap 7.3e-3, the seed-3 fixture has
    3.4e-4; profiles/r03_eig_gap_screen_L1000.txt), two trunk passes through the reference itself.  PLAIN
    north-star tolerances: CA-RMSD <= 1e-3 A per pass and final, |dconf| < 1e-4 - no eigensolver-floor term
    (the ill-conditioned seed-3 case stays in test_baseline_config_sizes_vs_reference as the documented
    subspace-rotation case).  Both the default and the exact-f32 convolution."""
    import hashlib
    from conftest import load_golden
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, encode_aln
    g = load_golden("synth_L1000_N2000_n1_m0_sep")
    L = 1000
    alnmat = encode_aln(synth.synth_msa(L, int(g["msa_rows"]), int(g["msa_seed"])))
    assert hashlib.sha256(alnmat.tobytes()).hexdigest() == bytes(g["alnmat_sha256"]).decode()
    eng = Engine("cuda:0", L, alnmat.shape[0])
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()})
    try:
        for mode in (0, 1, 2):
            eng.set_option("precision", mode)
            coords, confs = eng.predict(alnmat, None, 1, 0)
            eng.sync_check()
            ca_pass = eng.fetch("ca_pass", 2 * L * 3).cpu().numpy().reshape(2, L, 3)
            dev = np.array([ca_rmsd(ca_pass[p], g["ca_pass"][p]) for p in range(2)])
            print("L=1000 well-separated, precision", mode, "per-pass CA-RMSD", dev)
            assert (dev <= 1e-3).all(), (mode, dev)
            means = eng.fetch("conf_means", 2).cpu().numpy()
            assert np.abs(means - g["conf_mean_pass"]).max() < 1e-4
            assert ca_rmsd(coords.cpu().numpy()[:, 1], g["coords"][:, 1]) <= 1e-3
            assert np.abs(confs.cpu().numpy() - g["confs"]).max() < 1e-4
    finally:
        eng.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("name,L", [("deep_L500_N5000_n30_m0", 500), ("deep_L1000_N2000_n10_m0", 1000)])
def test_deep_recycling_at_the_large_configurations_vs_reference(synth_sd, name, L, precision):
    """the recycling loop (network.py:264-306) at DEPTH at the large configurations, through the
    reference itself - configs[2] (L=500, 5000 rows cut to 3000) at 31 trunk passes and configs[4] (L=1000, the
    well-separated seed 0) at 11 - every pass's trace and confidence mean.  One reference run takes most of an hour
    in the build container (make_goldens.py: reference at 8 threads + one oracle run at 4 threads for the per-pass
    floors).  The final structure at the plain tolerance where the fixture's own floor allows it, every pass at
    max(1e-3, 4 x that pass's floor) (recycling is expansive over its early passes, test_gpu_headline._check_passes)."""
    import hashlib
    import os
    from conftest import GOLDEN, load_golden
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, encode_aln
    if not os.path.exists(os.path.join(GOLDEN, name + ".npz")):
        pytest.skip("fixture not generated: " + name)
    g = load_golden(name)
    n = int(g["iterations"])
    P = n + 1
    alnmat = encode_aln(synth.synth_msa(L, int(g["msa_rows"]), int(g["msa_seed"])))
    assert hashlib.sha256(alnmat.tobytes()).hexdigest() == bytes(g["alnmat_sha256"]).decode()
    eng = Engine("cuda:0", L, alnmat.shape[0])
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()})
    eng.set_option("precision", precision)
    try:
        coords, confs = eng.predict(alnmat, None, n, 0)
        eng.sync_check()
        ca_pass = eng.fetch("ca_pass", P * L * 3).cpu().numpy().reshape(P, L, 3)
        dev = np.array([ca_rmsd(ca_pass[p], g["ca_pass"][p]) for p in range(P)])
        floor = np.asarray(g["noise_ca_pass"])
        means = eng.fetch("conf_means", P).cpu().numpy()
        final = ca_rmsd(coords.cpu().numpy()[:, 1], g["coords"][:, 1])
        dconf = float(np.abs(confs.cpu().numpy() - g["confs"]).max())
        print(name, "precision", precision, "per-pass CA-RMSD", np.array2string(dev, precision=2), "floors", np.array2string(floor, precision=2),
              "final", final, "max|dconf|", dconf, "max|dmean|", float(np.abs(means - g["conf_mean_pass"]).max()))
        assert (dev <= np.maximum(1e-3, 4.0 * floor)).all(), (dev, floor)
        assert np.abs(means - g["conf_mean_pass"]).max() < 1e-3
        assert final <= max(1e-3, 3.0 * float(g["noise_ca_rmsd"]))
        assert dconf < max(1e-4, 3.0 * float(g["noise_conf"]))
    finally:
        eng.close()


def test_above_the_former_length_limit_vs_reference(synth_sd):
    """L = 1344 > 1280 (the round-2 DMP_MAX_L): one trunk pass through the reference itself on an alignment whose top
    MDS eigenvalues are well separated (seed 4 of tools/screen_eig_gaps.py --L 1344 --N 1000: smallest relative gap
    among the top nine 3.0e-3; tests/golden/make_goldens.py).  Every kernel runs with 37 % more rows / columns than
    any other reference-pinned case: D = 28 224 in the covariance inverse (3.2 GB per matrix), the eigensolver's
    large-order instantiations (tridiag_step_kernel<8>, tri_eig_kernel<2>, backtransform_kernel<32, 1>).  PLAIN
    tolerances; default and exact-f32 convolution."""
    import hashlib
    import os
    from conftest import GOLDEN, load_golden
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, encode_aln
    name = "synth_L1344_N1000_n0_m0_sep"
    if not os.path.exists(os.path.join(GOLDEN, name + ".npz")):
        pytest.skip("fixture not generated: " + name)
    g = load_golden(name)
    L = 1344
    alnmat = encode_aln(synth.synth_msa(L, int(g["msa_rows"]), int(g["msa_seed"])))
    assert hashlib.sha256(alnmat.tobytes()).hexdigest() == bytes(g["alnmat_sha256"]).decode()
    eng = Engine("cuda:0", L, alnmat.shape[0])
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()})
    try:
        for mode in (0, 1, 2):
            eng.set_option("precision", mode)
            coords, confs = eng.predict(alnmat, None, 0, 0)
            eng.sync_check()
            ca = eng.fetch("ca_pass", L * 3).cpu().numpy().reshape(L, 3)
            dev = ca_rmsd(ca, g["ca_pass"][0])
            means = eng.fetch("conf_means", 1).cpu().numpy()
            final = ca_rmsd(coords.cpu().numpy()[:, 1], g["coords"][:, 1])
            dconf = float(np.abs(confs.cpu().numpy() - g["confs"]).max())
            print("L=1344, precision", mode, "CA-RMSD pass 0", dev, "final", final, "max|dconf|", dconf)
            assert dev <= 1e-3 and final <= 1e-3, (mode, dev, final)
            assert np.abs(means - g["conf_mean_pass"]).max() < 1e-4
            assert dconf < 1e-4
    finally:
        eng.close()


def test_largest_length_end_to_end(synth_sd, oracle_weights):
    """L = DMP_MAX_L = 2048 (D = 43 008 in the covariance inverse: 7.4 GB per matrix, (21 L)^2 and 442 L^2 just below
    2^31 elements).  What the CPU oracle can afford at this length is checked against it - sequence weights bit-exact,
    covariance samples, the vertical GRU - the inverse against the identity on sampled rows, and a whole prediction
    (2 trunk passes, 10 minimiser steps) for finite, normalised outputs and the exact symmetry of the Gram matrix."""
    from abi import Stages
    from dmpfold2_amd import predict
    L, N = predict.MAX_L, 96
    msa = _msa(L, N, 31)
    st = Stages(synth_sd, max_L=L, max_N=N)
    try:
        w = st.msa_weights(msa)
        assert np.array_equal(w.cpu().numpy(), np.asarray(O.reweight(msa)))
        cov = st.cov_build(msa, w)
        # sampled entries of the oracle's cov_reg (predict.py:44-52 / oracle fast_dca) without its D x D matrices
        D = 21 * L
        wt = torch.from_numpy(np.asarray(O.reweight(msa)))
        x = F.one_hot(torch.from_numpy(np.minimum(msa, 20).astype(np.int64)), 21).float().reshape(N, D)
        neff = wt.sum()
        num_points = neff - torch.sqrt(wt.mean())
        mean = (x * wt[:, None]).sum(dim=0, keepdim=True) / num_points
        xc = (x - mean) * torch.sqrt(wt[:, None])
        g = torch.Generator().manual_seed(3)
        idx = torch.randint(0, D, (4096, 2), generator=g)
        idx[:64, 1] = idx[:64, 0]                                          # some diagonal entries (the ridge)
        want = (xc[:, idx[:, 0]] * xc[:, idx[:, 1]]).sum(dim=0) / num_points \
            + (idx[:, 0] == idx[:, 1]).float() * 4.5 / torch.sqrt(neff)
        got = cov[idx[:, 0].cuda(), idx[:, 1].cuda()].cpu()
        assert (got - want).abs().max() <= 1e-5 * max(1.0, float(want.abs().max()))
        inv = st.spd_inverse(cov)
        rows = torch.tensor([0, 1, 777, 21 * 1280 + 5, D // 2, D - 2, D - 1], device="cuda")
        prod = (cov[rows] @ inv).double()                  # float32 products of 43 008 terms: 5e-5 is their rounding
        eye = torch.zeros_like(prod)
        eye[torch.arange(len(rows)), rows] = 1.0
        assert (prod - eye).abs().max() < 5e-4              # the bound of the D = 6300 identity test (measured here: 2e-4)
        del cov, inv, prod, eye
        v = st.gru_vertical(msa).cpu().numpy()
        idxm = torch.from_numpy(msa.astype(np.int64))
        vr = O._gru(oracle_weights, "vgru", oracle_weights["embed.weight"][idxm], 22, 512, 2, False, False)[-1].numpy()
        assert np.abs(v - vr).max() < 1e-5
        for form in (1, 2):                                # the float32 / three-piece bf16 forms at the largest length (64 tiles, 8 per XCD)
            st.eng.set_option("vgru_f32", form)
            v32 = st.gru_vertical(msa).cpu().numpy()
            st.eng.set_option("vgru_f32", -1)
            assert np.abs(v32 - vr).max() < 3e-6, form
        coords, confs = st.eng.predict(msa, None, 1, 10)
        st.eng.sync_check()
        c, f = coords.cpu().numpy(), confs.cpu().numpy()
        assert np.isfinite(c).all() and np.isfinite(f).all() and (f > 0).all() and (f < 1).all()
        gram = st.eng.fetch("gram", L * L).cpu().numpy().reshape(L, L)
        assert np.array_equal(gram, gram.T)
    finally:
        st.eng.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("name,L", [("fitns2_L300_N2000_n10_m100", 300), ("fit_L500_N5000_n30_m200", 500),
                                    ("fit_L1000_N2000_n3_m1000", 1000)])
def test_minimiser_on_at_the_configured_sizes_vs_reference(name, L, precision):
    """the minimiser ON, through the reference itself (network.py:106-137, 257-258, 308-309), at
    - the metric's configuration a SECOND time (fitns2_*: L=300 N=2000 10+100 with another alignment seed, another weight
      seed and another regression target than fitns_*: the headline parity is no longer one sample),
    - BASELINE configs[2] IN FULL (L=500, 5000 rows cut to 3000, 30 iterations + 200 steps),
    - BASELINE configs[4] at reduced depth (L=1000, 3 iterations + 1000 steps),
    on weight sets of the stability design of fitns_* (coord_fc fitted to a protein-like trace of the target's length,
    the coordinate GRU's MDS columns x 0.02; tests/golden/make_goldens.py).  In all three arithmetic settings: final
    structure max(1e-3, 3 x the reference's own thread-count floor) A, confidences 1e-4 (or 3 x their floor), every pass's
    trace max(1e-3, 4 x that pass's floor), bonds of the refined trace near 3.8 A."""
    import hashlib
    import os
    import sys
    from conftest import GOLDEN, load_golden
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import Engine, encode_aln
    if not os.path.exists(os.path.join(GOLDEN, name + ".npz")):
        pytest.skip("fixture not generated: " + name)
    g = load_golden(name)
    n, m = int(g["iterations"]), int(g["minsteps"])
    sd = synth.headline_fixture_weights(g["coord_fc"], float(g["coord_gru_mds_scale"]), seed=int(g["weights_seed"]))
    assert synth.weights_checksum(sd) == bytes(g["weights_sha256"]).decode()
    alnmat = encode_aln(synth.synth_msa(L, int(g["msa_rows"]), int(g["msa_seed"])))
    assert hashlib.sha256(alnmat.tobytes()).hexdigest() == bytes(g["alnmat_sha256"]).decode()
    eng = Engine("cuda:0", L, alnmat.shape[0])
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    eng.set_option("precision", precision)
    try:
        coords, confs = eng.predict(alnmat, None, n, m)
        eng.sync_check()
        coords, confs = coords.cpu().numpy(), confs.cpu().numpy()
        P = n + 1
        ca_pass = eng.fetch("ca_pass", P * L * 3).cpu().numpy().reshape(P, L, 3)
        dev = np.array([ca_rmsd(ca_pass[p], g["ca_pass"][p]) for p in range(P)])
        floor = np.asarray(g["noise_ca_pass"])
        means = eng.fetch("conf_means", P).cpu().numpy()
        final = ca_rmsd(coords[:, 1], g["coords"][:, 1])
        dconf = float(np.abs(confs - g["confs"]).max())
        print(name, "precision", precision, "per-pass CA-RMSD", np.array2string(dev, precision=2), "floors",
              np.array2string(floor, precision=2), "final", final, "floor", float(g["noise_ca_rmsd"]), "max|dconf|", dconf,
              file=sys.stderr)
        # (pass 0: the fixture's trace is the coordinate head's output, the engine records it after the first refinement)
        assert (dev[1:] <= np.maximum(1e-3, 4.0 * floor)[1:]).all(), (dev, floor)
        assert np.abs(means - g["conf_mean_pass"]).max() < 1e-3
        assert final <= max(1e-3, 3.0 * float(g["noise_ca_rmsd"])), (final, float(g["noise_ca_rmsd"]))
        assert dconf < max(1e-4, 3.0 * float(g["noise_conf"]))
        bonds = np.linalg.norm(coords[1:, 1] - coords[:-1, 1], axis=1)
        assert 3.6 < bonds.min() and bonds.max() < 4.0          # the minimiser ran in its regular regime
    finally:
        eng.close()
