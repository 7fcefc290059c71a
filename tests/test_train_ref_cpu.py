"""The float64 reference of the training slice's backward (tests/train_ref.py) against the reference project's recorded
autograd, on the CPU: what tests/test_gpu_train_lengths.py holds the kernels to must itself be right."""
import numpy as np
import torch

import dmpfold_oracle as O
import train_ref as TR
from conftest import load_golden
from test_gpu_train import philox_plane


def _dev(got, want):
    """max |got - want| in units of the recorded tensor's scale"""
    got = got.detach().double().reshape(-1)
    want = torch.as_tensor(np.asarray(want)).double().reshape(-1)
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _dev_sample(got, g, name):
    return _dev(got.detach().reshape(-1)[torch.from_numpy(g[name + ".idx"])], g[name + ".val"])


def test_block_reference_reproduces_the_recorded_autograd_of_block_3(oracle_weights):
    """bwd_block3_full_L24 (the reference project's float32 autograd through ResNet_Block 3) with the float64 argmax
    imposed as winners: every tensor of the fixture within 1e-5 of its scale.  Measured: the largest deviation is
    8.3e-07 (dsse_w; then dfc0 8.1e-07, dgamma 6.2e-07; u 4.4e-07, du 2.9e-07, dx 2.1e-07, dw 4.1e-07, db 4.0e-07); the
    smallest winner margin at this input is 3.9e-06 of the scale of z, above the float32 convolution's error, so no
    decision flips."""
    g = load_golden("bwd_block3_full_L24")
    B = TR.Block(oracle_weights, int(g["block"]), g["x"])
    r = B.whole(g["dout"], B.winners())
    dp = r["dparams"]
    dev = {"u": _dev(r["u"], g["u"]), "du": _dev(r["du"], g["du"]), "dx": _dev(r["dx"], g["dx"]),
           "db": _dev(r["db"], g["db"]), "dw": _dev_sample(r["dw"], g, "dw"),
           "dgamma": _dev(dp[0:128], g["dgamma"]), "dbeta": _dev(dp[128:256], g["dbeta"]),
           "dfc0": _dev(dp[256:1280], g["dfc0"]), "dfc2": _dev(dp[1280:2304], g["dfc2"]),
           "dsse_w": _dev(dp[2304:2432], g["dsse_w"]), "dsse_b": _dev(dp[2432:2433], g["dsse_b"])}
    q = B.z.detach().view(128, 4, 24, 24).topk(2, dim=1).values
    margin = float((q[:, 0] - q[:, 1]).min()) / float(B.z.detach().abs().max())
    print("bwd_block3_full_L24 vs the float64 reference, of scale: " + ", ".join(f"{k} {v:.1e}" for k, v in dev.items())
          + f"; smallest winner margin {margin:.1e} of scale")
    for k, v in dev.items():
        assert v <= 1e-5, (k, v)
    # the convolution half alone and the norm half alone are the whole block's pieces
    dx, dw, db = B.conv_bwd(r["du"], B.winners())
    assert _dev(dx + torch.from_numpy(g["dout"]).double(), g["dx"]) <= 1e-5 and _dev(db, g["db"]) <= 1e-5
    assert _dev_sample(dw, g, "dw") <= 1e-5
    du, dp2 = TR.norm_bwd(oracle_weights, int(g["block"]), g["u"], g["dout"])
    assert _dev(du, g["du"]) <= 1e-5 and _dev(dp2[2304:2432], g["dsse_w"]) <= 1e-5 and _dev(dp2[0:128], g["dgamma"]) <= 1e-5


def test_stem_reference_reproduces_the_recorded_autograd_of_the_stem(oracle_weights):
    """bwd_stem_L96 (the reference project's float32 autograd through resnet[0]) with the float64 argmax as winners and
    the fixture's near-tie decisions substituted (substitute_near_ties of tests/test_gpu_train.py): within that
    fixture's bound, 1e-4 of each tensor's scale.  Measured: the largest deviation is 2.0e-06 (db; then dw_dist 1.7e-06,
    dgamma 6.9e-07, dw_contacts 6.5e-07, dw_outer 6.0e-07, dw 4.3e-07; u, y, du and dmat1d at most 2.1e-07); none of the
    254 listed near-tie winners differs from the float64 argmax."""
    g = load_golden("bwd_stem_L96")
    L = int(g["L"])
    mat1d = philox_plane(g["mat1d_key"], (512, L), 1.0)
    f2d = philox_plane(g["f2d_key"], (442, L, L), float(g["f2d_scale"]))
    dmap = np.abs(philox_plane(g["dmap_key"], (L, L), float(g["dmap_scale"])))
    dy = philox_plane(g["g_key"], (128, L, L), 1.0)
    with torch.no_grad():
        W0 = oracle_weights["resnet.0.lin.weight"].double().reshape(384, 955)
        inp = TR.stem_input(torch.from_numpy(mat1d).double(), torch.from_numpy(f2d).double(), torch.from_numpy(dmap).double())[0]
        z = (W0 @ inp.reshape(955, -1) + oracle_weights["resnet.0.lin.bias"].double()[:, None]).reshape(384, L, L)
        win = TR.argmax_winners(z, 3)
        flat = win.view(-1)
        at = torch.from_numpy(g["tie.at"])
        differ = int((flat[at] != torch.from_numpy(g["tie.win"])).sum())
        flat[at] = torch.from_numpy(g["tie.win"])
    r = TR.stem_bwd(oracle_weights, mat1d, f2d, dmap, dy, win)
    dev = {"u": _dev_sample(r["u"], g, "u"), "y": _dev_sample(r["y"], g, "y"), "du": _dev_sample(r["du"], g, "du"),
           "dw": _dev_sample(r["dw"], g, "dw"), "dw_outer": _dev_sample(r["dw"][:, :512].contiguous(), g, "dw_outer"),
           "dw_dist": _dev(r["dw"][:, 954], g["dw_dist"]), "dw_contacts": _dev(r["dw"][:, 953], g["dw_contacts"]),
           "dmat1d": _dev_sample(r["dmat1d"], g, "dmat1d"), "db": _dev(r["db"], g["db"]),
           "dgamma": _dev(r["dgamma"], g["dgamma"]), "dbeta": _dev(r["dbeta"], g["dbeta"])}
    print(f"bwd_stem_L96 vs the float64 reference ({len(at)} near-ties listed, {differ} differ from the float64 argmax), "
          "of scale: " + ", ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= 1e-4, (k, v)


def test_imposed_argmax_is_autograd_through_torch_max(oracle_weights):
    """Imposing the reference's own argmax gives, bit for bit, the gradients of autograd through torch.max on the same
    float64 graph (L = 9): the gather is the maxout, not an approximation of it."""
    L = 9
    x = philox_plane(901, (128, L, L), 2.0)
    dout = philox_plane(902, (128, L, L), 1.0)
    B = TR.Block(oracle_weights, 3, x)
    a, b = B.whole(dout, B.winners()), B.whole(dout, None)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    mat1d, f2d = philox_plane(903, (512, L), 1.0), philox_plane(904, (442, L, L), 0.5)
    dmap = np.abs(philox_plane(905, (L, L), 10.0))
    b = TR.stem_bwd(oracle_weights, mat1d, f2d, dmap, dout, None)
    a = TR.stem_bwd(oracle_weights, mat1d, f2d, dmap, dout, TR.argmax_winners(b["z"], 3))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # ... and the stem reference without imposed winners IS the oracle's stem
    W64 = {k: v.double() for k, v in oracle_weights.items() if k.startswith("resnet.0.")}
    t = lambda v: torch.from_numpy(v).double()
    assert torch.equal(b["y"], O.stem(W64, TR.stem_input(t(mat1d), t(f2d), t(dmap)))[0])


def test_the_gpu_form_of_the_convolution_is_conv2d(oracle_weights):
    """The reference's 5x5 convolution on a GPU is unfold + matmul in slabs of rows; on the CPU it is F.conv2d.  The two
    agree to float64 rounding, forwards and in all three gradients, with more than one slab and a ragged last one."""
    L = 19
    x = torch.from_numpy(philox_plane(911, (128, L, L), 2.0)).double().requires_grad_(True)
    w = oracle_weights["resnet.5.layer1.lin.weight"].double().requires_grad_(True)
    b = oracle_weights["resnet.5.layer1.lin.bias"].double().requires_grad_(True)
    dz = torch.from_numpy(philox_plane(912, (512, L, L), 1.0)).double()
    old, TR.SLAB_PIXELS = TR.SLAB_PIXELS, 5 * L
    try:
        za = TR.conv5x5_unfold(x, w, b)
    finally:
        TR.SLAB_PIXELS = old
    zb = TR.conv5x5(x, w, b)
    ga, gb = torch.autograd.grad(za, (x, w, b), dz), torch.autograd.grad(zb, (x, w, b), dz)
    for p, q in zip((za,) + ga, (zb,) + gb):
        assert float((p - q).detach().abs().max()) <= 1e-12 * float(q.detach().abs().max())
