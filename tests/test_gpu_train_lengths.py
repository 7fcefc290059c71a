"""The training slice's backward kernels (dmpfold2_amd/csrc/train.hip) against a float64 reference at the lengths where
they branch - the backward counterpart of tests/test_gpu_lengths.py.

  conv5x5_maxout_kernel<true>, conv5x5_dgrad_kernel   16 x 16 pixel tiles: a one-pixel edge tile at L = 17, 33, 65, 129, 257;
                                                      the grid is rounded up to 8 (2 live workgroups of 8 up to L = 16)
  conv5x5_wgrad_kernel                                8 x 16 pixel tiles (ragged rows when L % 8, columns when L % 16) split
                                                      over 12 workgroups: fewer than 12 tiles up to L = 32
  bwd_bias_kernel                                     L^2 pixels in 16 chunks by integer division
  tb_stats / tb_channel_sums / stem_in_sums           cdiv(L^2, 4096) chunks: 1 -> 2 at 64 / 65, 2 -> 3 at 90 / 91, 4 -> 5 at
                                                      128 / 129; a last chunk shorter than a workgroup
  stem_bwd's three gemm_f32 calls                     K tails L % 16 and L^2 % 16; the 64-tile form up to L = 127, the 128-tile
                                                      form from 128; two-level accumulation once K = L exceeds 256 (L = 257)

The reference is tests/train_ref.py: the oracle's block_finish / stem / head in float64 under autograd with the maxout a
gather at the winners the KERNEL's forward saved, so every gradient comparison is between smooth functions and no decision
has to be excluded; the winners themselves are checked against the float64 convolution (every decision that differs from
the float64 argmax must have a float64 margin within twice the convolution's error bound).  Inputs come from Philox keys
derived from L (philox_plane of tests/test_gpu_train.py); case L uses block 1 + L % 16, so consecutive cases also switch the
cached flipped weight pack.  The u fed to the norm half and the stem's inputs have per-channel means and spreads.  Every
output is NaN- (winners: 0xFF-) poisoned with a guard tail (tests/abi.py), checked with sync_check() after every case.

Tolerances: every gradient within 1e-4 of the reference tensor's scale (close_full / close_sample of
tests/test_gpu_train.py); the maxout output within 1e-5 max(1, max |u|) ("conv vs float64 conv2d" of
tests/test_gpu_lengths.py); winner margins within 2e-5 max(1, max |z|).

With -s the module prints the largest error per check across the sweep next to its tolerance.  Measured on the MI355X
(155 cases in 13 s), the worst ratio error / tolerance per check and the length it occurred at:
  conv_winners    u 0.301 (L=127; the bound is 1e-5 absolute here, max |u| < 1), margin 0.031 (L=80); 17 decisions of the
                  whole sweep differ from the float64 argmax, at most 6 in one case (L=257)
  conv_bwd        dx 0.032 (L=63), dw 0.009 (L=257), db 0.001; with random winners dx 0.034 (L=127), dw 0.009, db 0.001
  norm_bwd        du 0.003, dgamma 0.002, dbeta 0.001, dfc0 0.009, dfc2 0.008, dsse_w 0.004, dsse_b 0.101 (L=129)
  head_bwd        dx 0.001, dw < 0.001, db < 0.001
  whole block     out 0.036 (L=257), du 0.010, dx 0.032 (L=129), dw 0.009, db 0.015, dgamma 0.025, dbeta 0.005, dfc0 0.066
                  (L=97), dfc2 0.024, dsse_w 0.044, dsse_b 0.485 (L=127)
  stem            u 0.117 (L=257), margin 0.017; dw outer 0.005, covariance 0.013, contacts 0.017, distance 0.029 (all
                  L=257), db 0.037 (L=257), dgamma 0.011, dbeta < 0.001, dmat1d 0.002; 4 decisions differ, at most 2 (L=257)
  single sequence db 0.006, dgamma 0.004, dw outer 0.002, dw distance 0.005, dmat1d 0.002; columns 512 .. 953 exactly 0
One check comes within a factor of 3 of its bound: the whole block's dsse_b at L = 127 (0.485).  d sSE bias is ONE number,
the sum over the L^2 pixels of d(a)_p, so "the tensor's scale" is that sum itself, and the terms cancel: at L = 127 (block
16) sum |d(a)| = 20558 and the sum is 3.24, a cancellation of 6350.  The kernel adds the float32 d(a)_p in float64, so its
error is that of the terms: 1.6e-4 absolute = 7.6e-9 of sum |d(a)|, far below one float32 rounding per term (each d(a)_p is
a 128-term float32 dot product, and in the whole block it is evaluated at the kernel's float32 u).  Float32 PyTorch
autograd on the CPU, on the same inputs and winners, deviates MORE on this number: 7.0e-5 of the sum (0.70 of the bound).
The per-half check (norm_bwd dsse_b, the float64 u given) stays at 0.101.
"""
import numpy as np
import pytest
import torch

import train_ref as TR
from test_gpu_train import philox_plane

pytestmark = pytest.mark.gpu

LENGTHS_128 = [8, 9, 15, 16, 17, 24, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 90, 91, 96, 97, 127, 128]
LENGTHS_272 = [129, 257]
STEM_LENGTHS = [8, 9, 15, 16, 17, 33, 63, 64, 65, 96, 127, 128, 129, 257]
ENTRIES = ["conv_winners", "conv_bwd", "norm_bwd", "head_bwd", "whole_block"]
REUSE_LENGTHS = [9, 17, 33, 65, 97]
SINGLE_SEQUENCE_LENGTHS = [17, 33]
TOL = 1e-4                            # of the reference tensor's scale: every gradient
REF = "cuda"                          # where the float64 arithmetic runs (train_ref.py: no float64 conv2d is needed there)

# d_dparams of the norm half and of the head (include/dmpfold_hip.h)
NORM_GROUPS = {"dgamma": (0, 128), "dbeta": (128, 256), "dfc0": (256, 1280), "dfc2": (1280, 2304), "dsse_w": (2304, 2432),
               "dsse_b": (2432, 2433)}
HEAD_GROUPS = {"dw": (0, 256), "db": (256, 258)}
STEM_DW_GROUPS = {"dw outer": (0, 512), "dw covariance": (512, 953), "dw contacts": (953, 954), "dw distance": (954, 955)}


# ------------------------------------------------------------------------------------------------ worst errors
WORST = {}          # check -> (error / tolerance, error, tolerance, L)
FLIPS = {}          # check -> (decisions that differ from the float64 argmax, summed over the sweep; the most in one case, its L)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest error per check across the backward length sweep (error, tolerance, at L):")
        for k in sorted(WORST):
            r, e, t, L = WORST[k]
            print(f"  {k:34s} {e:.3e}  tol {t:.1e}  ({r:5.3f} of it)  L={L}")
        for k, (n, most, L) in sorted(FLIPS.items()):
            print(f"  {k}: {n} decisions differ from the float64 argmax over the sweep, at most {most} in one case (L={L})")
    _BLOCK.clear()                     # the last length's float64 graph


def _check(name, err, tol, L):
    err = float(err)
    r = err / tol if np.isfinite(err) else float("inf")
    if name not in WORST or not r <= WORST[name][0]:
        WORST[name] = (r, err, tol, L)
    assert err <= tol, f"{name}: max error {err:.3e} > tolerance {tol:.1e} at L = {L}"


def _close(name, got, ref, L, rel=TOL, floor=0.0):
    """max |got - ref| <= rel x max(floor, max |ref|); NaN (an unwritten element) propagates and fails"""
    ref = ref.detach().to(got.device).double().reshape(got.shape)
    _check(name, (got.double() - ref).abs().max(), rel * max(floor, float(ref.abs().max()), 1e-30), L)


def _groups(prefix, got, ref, groups, L):
    for k, (lo, hi) in groups.items():
        _close(f"{prefix} {k}", got[lo:hi], ref[lo:hi], L)


def _flips(name, n, L):
    tot, most, at = FLIPS.get(name, (0, 0, L))
    FLIPS[name] = (tot + n, max(most, n), L if n > most else at)


# ------------------------------------------------------------------------------------------------ contexts, inputs
@pytest.fixture(scope="module")
def t128(synth_sd):
    from abi import Stages
    st = Stages(synth_sd, max_L=128, max_N=8)
    yield st
    st.eng.set_option("precision", 0)
    st.eng.sync_check()
    st.eng.close()


@pytest.fixture(scope="module")
def t272(synth_sd):
    from abi import Stages
    st = Stages(synth_sd, max_L=272, max_N=8)
    yield st
    st.eng.set_option("precision", 0)
    st.eng.sync_check()
    st.eng.close()


def _block_of(L):
    return 1 + L % 16


def _per_channel(key, n, lo, hi, mean):
    """per-channel spreads lo .. hi (ascending) and Philox means in (-mean, mean)"""
    return (np.linspace(lo, hi, n, dtype=np.float32), philox_plane(key, (n,), mean))


def _block_inputs(L):
    k = 1000 * L
    spread, mean = _per_channel(k + 5, 128, 0.5, 2.0, 3.0)
    return {"x": philox_plane(k + 1, (128, L, L), 2.0), "du": philox_plane(k + 2, (128, L, L), 1.0),
            "rnd": np.random.Generator(np.random.Philox(key=k + 3)).integers(0, 4, size=(128, L, L), dtype=np.uint8),
            "u": philox_plane(k + 4, (128, L, L), 1.0) * spread[:, None, None] + mean[:, None, None],
            "dout": philox_plane(k + 6, (128, L, L), 1.0), "hx": philox_plane(k + 7, (128, L, L), 2.0),
            "hg": philox_plane(k + 8, (2, L, L), 1.0)}


def _stem_inputs(L, features=True, salt=0):
    k = 1000 * L + 100 * salt
    ms, mm = _per_channel(k + 15, 512, 0.3, 1.0, 0.3)
    fs, fm = _per_channel(k + 16, 442, 0.2, 1.0, 0.2)
    f2d = philox_plane(k + 12, (442, L, L), 0.5) * fs[:, None, None] + fm[:, None, None]
    return {"mat1d": philox_plane(k + 11, (512, L), 1.0) * ms[:, None] + mm[:, None],
            "f2d": f2d if features else np.zeros_like(f2d), "dmap": np.abs(philox_plane(k + 13, (L, L), 10.0)),
            "dy": philox_plane(k + 14, (128, L, L), 1.0)}


_BLOCK = {}


def _block_ref(L, W):
    """the inputs of length L and the float64 convolution of its block with the graph kept: one length at a time"""
    if L not in _BLOCK:
        _BLOCK.clear()
        I = _block_inputs(L)
        _BLOCK[L] = (I, TR.Block(W, _block_of(L), I["x"], REF))
    return _BLOCK[L]


# ------------------------------------------------------------------------------------------------ the five checks
def _winner_checks(name, z, pool, u, idx, L):
    zmax = max(1.0, float(z.abs().max()))
    _close(f"{name} u", u, TR.select(z, pool, None), L, rel=1e-5, floor=1.0)
    assert int(idx.max()) <= pool - 1, f"{name}: a winner byte above {pool - 1} at L = {L}"
    margin, differ = TR.winner_margin(z, pool, idx)
    _flips(name, differ, L)
    print(f"{name} L={L}: {differ} of {idx.numel()} decisions differ from the float64 argmax, largest float64 margin "
          f"{margin / zmax:.1e} of scale")
    _check(f"{name} margin", margin, 2e-5 * zmax, L)


def _conv_winners(S, W, L):
    I, R = _block_ref(L, W)
    blk, x = _block_of(L), S.to(I["x"])
    u, idx = S.conv_winners(blk, x)
    _winner_checks("conv_winners", R.z.detach(), 4, u, idx, L)
    S.eng.set_option("precision", 1)
    u1, _ = S.conv(blk, x)
    S.eng.sync_check()
    assert torch.equal(u, u1), f"conv_winners and the float32 convolution differ at L = {L}"


def _conv_bwd(S, W, L):
    I, R = _block_ref(L, W)
    blk, x, du = _block_of(L), S.to(I["x"]), S.to(I["du"])
    _, idx = S.conv_winners(blk, x)
    own = S.conv_bwd(blk, x, du, idx)
    for k, got, ref in zip(("dx", "dw", "db"), own, R.conv_bwd(I["du"], idx)):
        _close(f"conv_bwd {k}", got, ref, L)
    rnd = S.to(I["rnd"], torch.uint8)
    for k, got, ref in zip(("dx", "dw", "db"), S.conv_bwd(blk, x, du, rnd), R.conv_bwd(I["du"], rnd)):
        _close(f"conv_bwd random winners {k}", got, ref, L)
    again = S.conv_bwd(blk, x, du, None)
    S.eng.sync_check()
    for k, p, q in zip(("dx", "dw", "db"), own, again):
        assert torch.equal(p, q), f"conv_bwd {k}: idx = NULL and idx = the forward's winners differ at L = {L}"
    # the routed gradient keeps its mass: the four bias gradients of a quadruple sum to that of its maxout channel
    db = own[2]
    assert float((db.view(128, 4).sum(1) - du.double().sum((1, 2)).float()).abs().max()) <= 1e-3 * float(du.abs().sum((1, 2)).max())


def _norm_bwd(S, W, L):
    I, _ = _block_ref(L, W)
    blk = _block_of(L)
    du, dp = S.norm_bwd(blk, S.to(I["u"]), S.to(I["dout"]))
    rdu, rdp = TR.norm_bwd(W, blk, I["u"], I["dout"], REF)
    _close("norm_bwd du", du, rdu, L)
    _groups("norm_bwd", dp, rdp, NORM_GROUPS, L)


def _head_bwd(S, W, L):
    I, _ = _block_ref(L, W)
    dx, dp = S.head_bwd(S.to(I["hx"]), S.to(I["hg"]))
    rdx, rdp = TR.head_bwd(W, I["hx"], I["hg"], REF)
    _close("head_bwd dx", dx, rdx, L)
    _groups("head_bwd", dp, rdp, HEAD_GROUPS, L)


def _whole_block(S, W, L):
    I, R = _block_ref(L, W)
    blk, x, dout = _block_of(L), S.to(I["x"]), S.to(I["dout"])
    S.eng.set_option("precision", 1)                         # the forward's second half in float32 as well
    u, idx = S.conv_winners(blk, x)
    _, stats = S.conv(blk, x)
    out = S.norm(blk, u, stats, x)
    du, dp = S.norm_bwd(blk, u, dout)
    dx, dw, db = S.conv_bwd(blk, x, du, idx)
    r = R.whole(I["dout"], idx)
    for k, got in (("out", out), ("du", du), ("dx", dx + dout), ("dw", dw), ("db", db)):
        _close(f"whole block {k}", got, r[k], L)
    _groups("whole block", dp, r["dparams"], NORM_GROUPS, L)


CHECKS = {"conv_winners": _conv_winners, "conv_bwd": _conv_bwd, "norm_bwd": _norm_bwd, "head_bwd": _head_bwd,
          "whole_block": _whole_block}


def _cases():
    return [pytest.param(L, e, id=f"L{L}-{e}") for L in LENGTHS_128 + LENGTHS_272 for e in ENTRIES]


@pytest.mark.parametrize("L,entry", _cases())
def test_backward_entry_vs_float64_at_length(request, oracle_weights, L, entry):
    S = request.getfixturevalue("t128" if L <= 128 else "t272")
    try:
        CHECKS[entry](S, oracle_weights, L)
        S.eng.sync_check()
    finally:
        S.check_guards()
        S.eng.set_option("precision", 0)


# ------------------------------------------------------------------------------------------------ the stem
def _stem_forward(S, I, features=True):
    """stem_static -> stem_winners on the inputs I: -> (mat1d, dmap, dy on the device, u, idx)"""
    mat1d, dmap, dy = S.to(I["mat1d"]), S.to(I["dmap"]), S.to(I["dy"])
    if features:
        inv, contacts = TR.f2d_as_inverse(torch.from_numpy(I["f2d"]))
        z0 = S.stem_static(mat1d, S.to(inv), S.to(contacts))
    else:
        z0 = S.stem_static(mat1d, None, None)
    u, idx = S.stem_winners(z0, dmap)
    return mat1d, dmap, dy, u, idx


def _stem_compare(name, I, W, u, idx, dw, dp, dm, L, groups):
    r = TR.stem_bwd(W, I["mat1d"], I["f2d"], I["dmap"], I["dy"], idx, REF)
    _winner_checks(f"{name}_winners", r["z"], 3, u, idx, L)
    for k, (lo, hi) in groups.items():
        _close(f"{name}_bwd {k}", dw[:, lo:hi], r["dw"][:, lo:hi], L)
    _close(f"{name}_bwd db", dp[:384], r["db"], L)
    _close(f"{name}_bwd dgamma", dp[384:512], r["dgamma"], L)
    _close(f"{name}_bwd dbeta", dp[512:640], r["dbeta"], L)
    _close(f"{name}_bwd dmat1d", dm, r["dmat1d"], L)


@pytest.mark.parametrize("L", STEM_LENGTHS)
def test_stem_backward_vs_float64_at_length(request, oracle_weights, L):
    S = request.getfixturevalue("t128" if L <= 128 else "t272")
    try:
        I = _stem_inputs(L)
        mat1d, dmap, dy, u, idx = _stem_forward(S, I)
        dw, dp, dm = S.stem_bwd(u, idx, dy, mat1d, dmap)
        S.eng.sync_check()
        _stem_compare("stem", I, oracle_weights, u, idx, dw, dp, dm, L, STEM_DW_GROUPS)
    finally:
        S.check_guards()


def test_first_maximal_channel_wins_an_exact_tie(t128):
    """The winner of a triple with equal maxima is its FIRST maximal channel (torch.max; the header's contract for the
    saved winners).  dmap = 0, so the caller's z0 is the compared value itself: triples (a, a, a), (a, b, b) and (b, a, b)
    with b > a give winners 0, 1, 0 at every pixel of an L = 17 target, and u is the maximum bit for bit."""
    S, L = t128, 17
    a = philox_plane(1717, (L, L), 4.0)
    b = a + np.float32(1.0)
    assert (b > a).all()
    pattern = [(a, a, a), (a, b, b), (b, a, b)]
    z0 = np.stack([pattern[g % 3][q] for g in range(128) for q in range(3)])
    try:
        u, idx = S.stem_winners(S.to(z0), S.to(np.zeros((L, L), np.float32)))
        S.eng.sync_check()
        want_idx = torch.tensor([0, 1, 0], dtype=torch.uint8).repeat(43)[:128, None, None].expand(128, L, L)
        want_u = torch.from_numpy(np.stack([a if g % 3 == 0 else b for g in range(128)]))
        assert torch.equal(idx.cpu(), want_idx)
        assert torch.equal(u.cpu(), want_u)
    finally:
        S.check_guards()


# ------------------------------------------------------------------------------------------------ reused context
def _run_backward(S, L):
    """Every backward entry point on inputs of length L, in the order conv_bwd(block a), stem_bwd, conv_bwd(block a): the
    stem overwrites the flipped weight pack, which the second conv_bwd must rebuild."""
    I, T = _block_inputs(L), _stem_inputs(L)
    blk, x, du = _block_of(L), S.to(I["x"]), S.to(I["du"])
    out = {}
    out["conv_winners u"], out["conv_winners idx"] = S.conv_winners(blk, x)
    out["norm_bwd du"], out["norm_bwd dparams"] = S.norm_bwd(blk, S.to(I["u"]), S.to(I["dout"]))
    out["head_bwd dx"], out["head_bwd dparams"] = S.head_bwd(S.to(I["hx"]), S.to(I["hg"]))
    first = S.conv_bwd(blk, x, du, None)
    mat1d, dmap, dy, u, idx = _stem_forward(S, T)
    out["stem u"], out["stem idx"] = u, idx
    out["stem_bwd dw"], out["stem_bwd dparams"], out["stem_bwd dmat1d"] = S.stem_bwd(u, idx, dy, mat1d, dmap)
    second = S.conv_bwd(blk, x, du, None)
    S.eng.sync_check()
    for k, p, q in zip(("dx", "dw", "db"), first, second):
        assert torch.equal(p, q), f"conv_bwd {k} differs after stem_bwd used the workspace at L = {L}"
        out[f"conv_bwd {k}"] = p
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("L", REUSE_LENGTHS)
def test_backward_on_a_reused_context_gives_a_fresh_contexts_bits(synth_sd, t128, L):
    """The backward form of test_exact_capacity_and_reused_context_give_the_same_bits: a context that has just run every
    backward entry point at L = 128, run at L, against a fresh context of capacity exactly L.  The one workspace is carved
    for the capacity and reused by every smaller target and by both the blocks and the stem."""
    from abi import Stages
    shared = t128
    fresh = Stages(synth_sd, max_L=L, max_N=8)
    try:
        _run_backward(shared, 128)
        got = _run_backward(shared, L)
        want = _run_backward(fresh, L)
        for k in want:
            assert torch.equal(got[k], want[k]), f"{k} differs between a reused max_L = 128 context and a fresh max_L = {L} context"
            if want[k].dtype.is_floating_point:
                assert bool(torch.isfinite(want[k]).all()), k
    finally:
        shared.check_guards()
        fresh.check_guards()
        fresh.eng.close()


# ------------------------------------------------------------------------------------------------ single-sequence targets
NO_COV = {k: v for k, v in STEM_DW_GROUPS.items() if k in ("dw outer", "dw distance")}


def _single_sequence(S, W, L):
    I = _stem_inputs(L, features=False, salt=1)
    mat1d, dmap, dy, u, idx = _stem_forward(S, I, features=False)
    dw, dp, dm = S.stem_bwd(u, idx, dy, mat1d, dmap)
    S.eng.sync_check()
    cov = dw[:, 512:954]
    assert int(torch.count_nonzero(cov)) == 0 and not bool(torch.isnan(cov).any()), \
        f"{int(torch.count_nonzero(cov))} of the {cov.numel()} covariance / contact columns of dw are not 0 at L = {L}"
    _stem_compare("single-sequence stem", I, W, u, idx, dw, dp, dm, L, NO_COV)


@pytest.mark.parametrize("L", SINGLE_SEQUENCE_LENGTHS)
def test_single_sequence_stem_gradient_after_a_target_with_features(oracle_weights, t128, L):
    """dmp_stem_static without features (d_inv = d_contacts = NULL) does not write the context's covariance planes, so they
    still hold the previous target's: the covariance and contact columns of the weight gradient are exactly 0
    nevertheless, and everything else is the float64 reference's gradient at a zero f2d."""
    S = t128
    try:
        _stem_forward(S, _stem_inputs(L))                  # another target of the same length, with features
        _single_sequence(S, oracle_weights, L)
    finally:
        S.check_guards()


@pytest.mark.parametrize("L", SINGLE_SEQUENCE_LENGTHS)
def test_single_sequence_stem_gradient_on_a_fresh_context(synth_sd, oracle_weights, L):
    """... and on a context whose planes were never written (the allocation is not cleared)."""
    from abi import Stages
    S = Stages(synth_sd, max_L=L, max_N=8)
    try:
        _single_sequence(S, oracle_weights, L)
    finally:
        S.check_guards()
        S.eng.close()


def test_stem_bwd_refuses_a_length_stem_static_did_not_run(synth_sd, t128):
    """dmp_stem_bwd reads the planes dmp_stem_static left on the context: for another length (or before any
    dmp_stem_static) it returns the argument error with nothing enqueued - the poisoned outputs stay untouched - and the
    context goes on working."""
    from abi import Stages
    from dmpfold2_amd import _lib

    def refused(S, L):
        I = _stem_inputs(L)
        u, idx = S.to(philox_plane(7, (128, L, L), 1.0)), S.to(np.zeros((128, L, L), np.uint8), torch.uint8)
        outs = S.f32(384, 955), S.f32(640), S.f32(512, L)
        with pytest.raises(_lib.DmpError, match="dmp_stem_static"):
            S.call("dmp_stem_bwd", u, idx, S.to(I["dy"]), S.to(I["mat1d"]), S.to(I["dmap"]), L, *outs)
        S.eng.sync_check()
        assert all(bool(torch.isnan(o).all()) for o in outs)

    S = t128
    fresh = Stages(synth_sd, max_L=33, max_N=8)
    try:
        refused(fresh, 33)                                   # no dmp_stem_static yet
        I = _stem_inputs(17)
        mat1d, dmap, dy, u, idx = _stem_forward(S, I)
        refused(S, 33)
        dw, _, _ = S.stem_bwd(u, idx, dy, mat1d, dmap)       # the target dmp_stem_static ran for is still served
        S.eng.sync_check()
        assert bool(torch.isfinite(dw).all())
    finally:
        S.check_guards()
        fresh.check_guards()
        fresh.eng.close()
