"""Every per-length stage kernel against the CPU oracle at the lengths where the kernels branch, in all three precisions.

The benchmark and most parity tests run one length (L = 82 or 300); the kernels choose their tiles, grids and
workgroup counts by L:
  5x5 convolution         8 x 16 pixel tiles up to L = 80, 16 x 16 above; a partial band below the last full band
                          (L % 16 in 1 .. 15); a single tile below L = 16
  InstanceNorm + scSE     cdiv(L, 64) workgroups (64 / 65, 128 / 129)
  head, Gram, stem        cdiv(L, 256) workgroups (256 / 257), cdiv(L * L, 64) for the stem's static part
  minimiser               one workgroup with min(8, 1024 / L) partial slices below L = 32, a 16-workgroup cluster
                          with ceil(L / 16) residues per workgroup from L = 32 on
  Gauss-Jordan inverse    D = 21 L: a ragged last 128-row block at every length
Every check feeds the stage the ORACLE's input for it (the oracle's capture of one prediction, N = 48, one recycling
iteration, no refinement), at the tolerances of tests/test_gpu_parity.py, and every output is a NaN-poisoned buffer with
a guard tail (tests/abi.py), checked after each test: an element left unwritten or a write past the end fails.

The second half runs a prediction and two stages on a context that has just run a length-128 target and compares them,
bit for bit, with a fresh context created with exactly the capacity of the target.

With -s, the module prints the largest error per check across the sweep next to its tolerance.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure)

N_ROWS = 48
LENGTHS_128 = [8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 47, 48, 63, 64, 65, 79, 80, 81, 95, 96, 97, 127, 128]
LENGTHS_272 = [129, 255, 256, 257]
PRECISIONS = [0, 1, 2]
STAGES = ["features", "gru_vertical", "gru_bidir", "stem", "block1", "block2", "block16", "head", "eigh", "coords",
          "refine", "backbone", "end_to_end"]
ONE_ROW_LENGTHS = [8, 33]                      # one-row alignments: the zero-DCA path end to end
CAPACITY_LENGTHS = [8, 15, 17, 33, 65, 81, 97, 128]
DIAG_CLAMPED = np.float32(np.sqrt(np.float64(np.float32(1e-8))))     # pair distance of a residue to itself, clamp 1


def _cases():
    out = []
    for L in LENGTHS_128 + LENGTHS_272:
        for p in PRECISIONS:
            for s in STAGES + (["end_to_end_one_row"] if L in ONE_ROW_LENGTHS else []):
                out.append(pytest.param(L, p, s, id=f"L{L}-p{p}-{s}"))
    return out


# ------------------------------------------------------------------------------------------------ worst errors
WORST = {}          # check -> (error / tolerance, error, tolerance, L, precision)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest error per check across the length sweep (error, tolerance, at L, precision):")
        for k in sorted(WORST):
            r, e, t, L, p = WORST[k]
            print(f"  {k:34s} {e:.3e}  tol {t:.1e}  ({r:5.3f} of it)  L={L} p={p}")


def _check(name, err, tol, L, p):
    err = float(err)
    r = err / tol if np.isfinite(err) else float("inf")
    if name not in WORST or not r <= WORST[name][0]:
        WORST[name] = (r, err, tol, L, p)
    assert err <= tol, f"{name}: max error {err:.3e} > tolerance {tol:.1e} at L = {L}, precision {p}"


def _maxdiff(got, ref):
    got = got.detach().cpu().double() if isinstance(got, torch.Tensor) else torch.as_tensor(np.asarray(got)).double()
    ref = ref.detach().cpu().double() if isinstance(ref, torch.Tensor) else torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max())          # NaN (an unwritten element) propagates and fails every bound


def _scale(ref, rel):
    return rel * max(1.0, float(torch.as_tensor(ref).abs().max()))


# ------------------------------------------------------------------------------------------------ inputs and oracle
def _msa(L, N, seed):
    from dmpfold2_amd import synth
    return O.encode_aln(synth.synth_msa(L, N, seed))


def _spread_chain(L, seed):
    """A random chain of 3.8 A steps that does not come back closer than 2.5 A to itself (a few pairs inside the
    minimiser's 3 A repulsion range), centred on the origin."""
    rng = np.random.default_rng(seed)
    P = np.zeros((L, 3))
    for i in range(1, L):
        for _ in range(1000):
            s = rng.standard_normal(3)
            q = P[i - 1] + s * (3.8 / np.linalg.norm(s))
            if i < 2 or np.linalg.norm(P[:i - 1] - q, axis=1).min() >= 2.5:
                break
        P[i] = q
    return (P - P.mean(axis=0)).astype(np.float32)


class Ref:
    """Oracle tensors of one length, computed when first needed and shared by the three precisions."""

    def __init__(self, L, W):
        self.L, self.W = L, W
        self.aln = _msa(L, N_ROWS, 1000 + L)
        self.cap = {}
        torch.set_num_threads(max(1, torch.get_num_threads()))
        self.coords, self.conf = O.predict(self.aln, W, None, 1, 0, "canonical", self.cap)
        self._memo = {}

    def get(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def resinp(self, dmap):
        L, c = self.L, self.cap
        m = c["mat1d"]
        pair = (m.unsqueeze(1) * m.unsqueeze(2)).unsqueeze(0)
        inv = c["inv_cov"].view(L, 21, L, 21).transpose(1, 2).reshape(L, L, 441)
        f2d = torch.cat((inv, c["contacts"][:, :, None]), dim=2).permute(2, 0, 1).unsqueeze(0)
        return torch.cat((pair, f2d, dmap.view(1, 1, L, L)), dim=1)

    def chain(self):
        return self.get("chain", lambda: _spread_chain(self.L, 2000 + self.L))


_REF = {}


def _ref(L, oracle_weights):
    if L not in _REF:
        _REF.clear()                               # the sweep runs length by length: keep one length's tensors
        _REF[L] = Ref(L, oracle_weights)
    return _REF[L]


def _conv_f64(W, block, x):
    """Block `block`'s 5x5 convolution + maxout of x (128, L, L) in float64 on the GPU (im2col slabs of 32 rows)."""
    L = x.shape[-1]
    w = W[f"resnet.{block}.layer1.lin.weight"].cuda().double().reshape(512, 3200)
    b = W[f"resnet.{block}.layer1.lin.bias"].cuda().double()
    xp = F.pad(x.cuda().double(), (2, 2, 2, 2))
    out = torch.empty(128, L, L, dtype=torch.float64, device="cuda")
    for lo in range(0, L, 32):
        hi = min(L, lo + 32)
        cols = F.unfold(xp[None, :, lo:hi + 4], 5)[0]                       # (3200, (hi - lo) * L)
        y = (w @ cols + b[:, None]).reshape(128, 4, hi - lo, L)
        out[:, lo:hi] = y.max(1)[0]
    return out.cpu()


def _near_degenerate(M):
    """True if two of the eigenvalues that the MDS embedding uses (the top 8, and the 9th beside the 8th) lie within
    float32 rounding of each other: their eigenvectors are then not defined to float32 resolution."""
    lam = torch.linalg.eigvalsh(M.double())
    top = lam[-9:] if lam.numel() > 8 else lam
    gaps = (top[1:] - top[:-1]).abs()
    return bool(gaps.min() < 64 * 2.0 ** -24 * float(lam.abs().max()))


# ------------------------------------------------------------------------------------------------ contexts
@pytest.fixture(scope="module")
def ctx128(synth_sd):
    from abi import Stages
    st = Stages(synth_sd, max_L=128, max_N=64)
    yield st
    st.eng.set_option("precision", 0)
    st.eng.sync_check()
    st.eng.close()


@pytest.fixture(scope="module")
def ctx272(synth_sd):
    from abi import Stages
    st = Stages(synth_sd, max_L=272, max_N=64)
    yield st
    st.eng.set_option("precision", 0)
    st.eng.sync_check()
    st.eng.close()


# ------------------------------------------------------------------------------------------------ stage checks
def _features(S, R, L, p):
    c = R.cap
    w = S.msa_weights(R.aln).cpu().numpy()
    assert np.array_equal(w, c["w"].numpy()), f"msa_weights differ at L = {L}"
    ref = c["cov_reg"]
    cov = S.cov_build(R.aln, S.to(c["w"].numpy()))
    _check("cov_build", _maxdiff(cov, ref), _scale(ref, 1e-5), L, p)
    iref = c["inv_cov"]
    inv = S.spd_inverse(S.to(ref.numpy()))
    _check("spd_inverse", _maxdiff(inv, iref), _scale(iref, 1e-5), L, p)
    cref = c["contacts"]
    con = S.dca_contacts(S.to(iref.numpy()), L)
    _check("dca_contacts", _maxdiff(con, cref), _scale(cref, 1e-5), L, p)
    # fast_dca's return value: channel 21a+b of pair (i, j) is inv_cov[21i+a, 21j+b], channel 441 the contacts
    fref = torch.cat((iref.view(L, 21, L, 21).transpose(1, 2).reshape(L, L, 441), cref[:, :, None]), dim=2)
    f = S.dca_features(R.aln)
    _check("dca_features", _maxdiff(f, fref), _scale(fref, 1e-5), L, p)


def _gru_vertical(S, R, L, p):
    W = R.W
    ref = R.get("vgru", lambda: O._gru(W, "vgru", W["embed.weight"][torch.from_numpy(R.aln.astype(np.int64))],
                                       22, 512, 2, False, False)[-1])
    # the float32 forms (1, 2) at the bound of test_float32_vertical_gru_is_the_references_arithmetic
    _check(f"gru_vertical p{p}", _maxdiff(S.gru_vertical(R.aln), ref), 1e-5 if p == 0 else 3e-6, L, p)


def _gru_bidir(S, R, L, p):
    W, c = R.W, R.cap
    vin = R.get("vgru", lambda: O._gru(W, "vgru", W["embed.weight"][torch.from_numpy(R.aln.astype(np.int64))],
                                       22, 512, 2, False, False)[-1])
    ref = O._gru(W, "hgru", vin.unsqueeze(1), 512, 256, 2, True, False)[:, 0]
    got = S.gru_bidir(0, S.to(vin.numpy()))
    _check("gru_bidir(0) horizontal", _maxdiff(got, ref), 1e-5, L, p)
    _check("gru_bidir(0) = mat1d", _maxdiff(got.t(), c["mat1d"]), 1e-5, L, p)
    emb = torch.cat((c["mat1d"].t(), c["p0.mds"]), dim=1)
    ref = O._gru(W, "coord_gru", emb.unsqueeze(0), 520, 256, 3, True, True)[0]
    _check("gru_bidir(1) coordinate", _maxdiff(S.gru_bidir(1, S.to(emb.numpy())), ref), 1e-5, L, p)


def _z0(S, R):
    c = R.cap
    return S.stem_static(S.to(c["mat1d"].numpy()), S.to(c["inv_cov"].numpy()), S.to(c["contacts"].numpy()))


def _stem(S, R, L, p):
    z0 = _z0(S, R)
    dmap = torch.zeros(L, L) - 1
    ref = R.cap["p0.stem"][0]                                   # the oracle's stem at the seed distance map -1
    _check("stem, dmap -1", _maxdiff(S.stem_update(z0, S.to(dmap.numpy())), ref), _scale(ref, 1e-4), L, p)
    dmap2 = O.pair_distances(torch.from_numpy(R.chain()))
    ref2 = R.get("stem2", lambda: O.stem(R.W, R.resinp(dmap2))[0])
    _check("stem, chain dmap", _maxdiff(S.stem_update(z0, S.to(dmap2.numpy())), ref2), _scale(ref2, 1e-4), L, p)


def _block(block):
    def run(S, R, L, p):
        W, c = R.W, R.cap
        x = c["p0.stem"] if block == 1 else c["p0.block1"]

        def refs():
            u = O.block_conv(W, block, x)
            s = torch.stack((u[0].double().sum(dim=(1, 2)), (u[0].double() ** 2).sum(dim=(1, 2))), 1)
            return u, s, O.block_finish(W, block, u, x)[0], _conv_f64(W, block, x[0])
        u_ref, s_ref, out_ref, truth = R.get(f"block{block}", refs)
        xd = S.to(x[0].numpy())
        u, stats = S.conv(block, xd)
        _check("conv", _maxdiff(u, u_ref[0]), _scale(u_ref, 1e-5), L, p)
        _check("conv statistics", _maxdiff(stats, s_ref), 1e-5 * float(s_ref.abs().max()), L, p)
        _check("conv vs float64 conv2d", _maxdiff(u, truth), 1e-5 * max(1.0, float(truth.abs().max())), L, p)
        out = S.norm(block, S.to(u_ref[0].numpy()), S.to(s_ref.numpy(), torch.float64), xd)
        _check("norm on the oracle's u", _maxdiff(out, out_ref), _scale(out_ref, 1e-5), L, p)
        out = S.norm(block, u, stats, xd)
        _check("norm on the kernel's u", _maxdiff(out, out_ref), _scale(out_ref, 1e-4), L, p)
    return run


def _head(S, R, L, p):
    c = R.cap
    conf, M = S.head_gram(S.to(c["p0.block16"][0].numpy()))
    _check("head_gram conf", _maxdiff(conf, c["p0.conf"]), 1e-4, L, p)
    _check("head_gram M", _maxdiff(M, c["p0.M"]), _scale(c["p0.M"], 1e-5), L, p)
    M = M.cpu()
    assert torch.equal(M, M.t()), f"head_gram: M is not exactly symmetric at L = {L}"
    tconf, tM = S.trunk_pass(_z0(S, R), S.to((torch.zeros(L, L) - 1).numpy()))
    _check("trunk_pass conf", _maxdiff(tconf, c["p0.conf"]), 1e-4, L, p)
    _check("trunk_pass M", _maxdiff(tM, c["p0.M"]), _scale(c["p0.M"], 1e-4), L, p)


def _eigh(S, R, L, p):
    M = R.cap["p0.M"]
    got = S.eigh_top8(S.to(M.numpy()))
    lam, vec = torch.linalg.eigh(M.double(), UPLO="U")
    truth = (O.canonical_signs(vec) * lam.clamp(min=1e-8).sqrt())[:, -8:]
    _check("eigh_top8 vs float64", _maxdiff(got, truth), _scale(truth, 2e-5), L, p)
    if _near_degenerate(M):
        # two used eigenvalues within float32 rounding of each other: the float32 LAPACK solve of the oracle does not
        # resolve their eigenvectors, so this length is held to the float64 truth alone
        print(f"L = {L}: near-degenerate top-8 spectrum, eigh_top8 compared with the float64 truth only")
        return
    ref = O.mds_top8(M.unsqueeze(0), "canonical")[0]
    _check("eigh_top8 vs oracle", _maxdiff(got, ref), _scale(ref, 5e-4), L, p)


def _pair_distance_check(name, got, ref, L, p):
    """< 1e-5 for every distance below 128 A; from 128 A on, where float32 values lie 1.5e-5 apart and a one-ulp
    difference in a library sqrt (the oracle's CPU sqrt rounds the diagonal one ulp high on some hosts) already
    exceeds 1e-5, within one float32 ulp of the oracle's distance."""
    got, ref = got.cpu().double(), ref.double()
    near = ref < 128.0
    _check(name, float((got - ref)[near].abs().max()), 1e-5, L, p)
    if not near.all():
        ulp = torch.from_numpy(np.spacing(ref[~near].float().numpy()).astype(np.float64))
        far = float(((got - ref)[~near].abs() / ulp).max())
        _check(name + " >= 128 A (ulp)", far, 1.0, L, p)


def _coords(S, R, L, p):
    c = R.cap
    got = S.coords_from_mds(S.to(c["mat1d"].numpy()), S.to(c["p0.mds"].numpy()))
    _check("coords_from_mds", _maxdiff(got, c["p0.ca"]), 1e-4, L, p)
    for ca in (c["p0.ca"], torch.from_numpy(R.chain())):
        ref = O.pair_distances(ca)
        d1 = S.pair_distances(S.to(ca.numpy()), 1)
        _pair_distance_check("pair_distances clamp 1", d1, ref, L, p)
        # the diagonal is sqrt(1e-8f) correctly rounded (0x38d1b717); PyTorch's vectorised CPU sqrt returns one ulp
        # above it on some hosts, so the bits are compared with the IEEE value rather than with the oracle's
        dg = torch.diagonal(d1.cpu()).numpy()
        assert (dg == DIAG_CLAMPED).all(), f"pair_distances diagonal at L = {L}: {dg[:4].view(np.uint32)}"
        d0 = S.pair_distances(S.to(ca.numpy()), 0)
        _pair_distance_check("pair_distances clamp 0", d0 - torch.diag(torch.diagonal(d0)),
                             ref - torch.diag(torch.diagonal(ref)), L, p)
        assert not torch.diagonal(d0).cpu().any(), f"pair_distances clamp 0: nonzero diagonal at L = {L}"


def _refine(S, R, L, p):
    # below L = 32 the single-workgroup minimiser, from 32 on the 16-workgroup cluster
    ca = R.chain()
    for steps, tol in ((1, 1e-5), (10, 1e-5), (100, 1e-4)):
        ref = R.get(f"refine{steps}", lambda: O.refine_coords(torch.from_numpy(ca), steps))
        _check(f"refine {steps} steps", _maxdiff(S.refine(S.to(ca), steps), ref), tol, L, p)


def _backbone(S, R, L, p):
    ca = R.chain()
    logit = R.cap["p0.conf"]
    ref = O.ca_to_backbone(torch.from_numpy(ca).unsqueeze(0)).view(L, 5, 3)
    coords, conf = S.backbone(S.to(ca), S.to(logit.numpy()))
    _check("backbone coordinates", _maxdiff(coords, ref), 1e-4, L, p)
    _check("backbone conf", _maxdiff(conf, torch.sigmoid(logit)), 1e-6, L, p)


def _end_to_end_against(S, aln, coords_ref, conf_ref, pass_means, L, p, tag):
    coords, confs = S.eng.predict(aln, None, 1, 0)
    S.eng.sync_check()
    means = S.eng.fetch("conf_means", 2)
    d = coords.cpu()[:, 1].double() - coords_ref[:, 1].double()
    _check(f"{tag} CA-RMSD", float((d ** 2).sum(-1).mean().sqrt()), 1e-3, L, p)
    _check(f"{tag} conf", _maxdiff(confs, conf_ref), 1e-4, L, p)
    _check(f"{tag} per-pass conf_means", _maxdiff(means, pass_means), 1e-3, L, p)


def _end_to_end(S, R, L, p):
    c = R.cap
    means = torch.stack((c["p0.conf"].mean(), c["p1.conf"].mean()))
    _end_to_end_against(S, R.aln, R.coords, R.conf, means, L, p, "end to end")


def _end_to_end_one_row(S, R, L, p):
    def run():
        cap = {}
        aln = np.ascontiguousarray(R.aln[:1])
        coords, conf = O.predict(aln, R.W, None, 1, 0, "canonical", cap)
        return aln, coords, conf, torch.stack((cap["p0.conf"].mean(), cap["p1.conf"].mean()))
    aln, coords, conf, means = R.get("one_row", run)
    _end_to_end_against(S, aln, coords, conf, means, L, p, "end to end N = 1")


CHECKS = {"features": _features, "gru_vertical": _gru_vertical, "gru_bidir": _gru_bidir, "stem": _stem,
          "block1": _block(1), "block2": _block(2), "block16": _block(16), "head": _head, "eigh": _eigh,
          "coords": _coords, "refine": _refine, "backbone": _backbone, "end_to_end": _end_to_end,
          "end_to_end_one_row": _end_to_end_one_row}


@pytest.mark.parametrize("L,precision,stage", _cases())
def test_stage_vs_oracle_at_length(request, oracle_weights, L, precision, stage):
    S = request.getfixturevalue("ctx128" if L <= 128 else "ctx272")
    R = _ref(L, oracle_weights)
    S.eng.set_option("precision", precision)
    try:
        CHECKS[stage](S, R, L, precision)
        S.eng.sync_check()
    finally:
        S.check_guards()
        S.eng.set_option("precision", 0)


# ------------------------------------------------------------------------------------------------ capacity and reuse
def _run_target(S, aln, seed):
    """A prediction with refinement, a block convolution and the stem on inputs of the target's length."""
    L = aln.shape[1]
    rng = np.random.default_rng(seed)
    coords, confs = S.eng.predict(aln, None, 1, 5)
    x = S.to(rng.standard_normal((128, L, L)).astype(np.float32))
    u, stats = S.conv(2, x)
    mat1d = S.to((rng.standard_normal((512, L)) * 0.2).astype(np.float32))
    inv = S.to((rng.standard_normal((21 * L, 21 * L)) * 0.1).astype(np.float32))
    contacts = S.to((rng.standard_normal((L, L)) * 0.1).astype(np.float32))
    z0 = S.stem_static(mat1d, inv, contacts)
    dmap = S.to(O.pair_distances(torch.from_numpy(_spread_chain(L, seed))).numpy())
    x1 = S.stem_update(z0, dmap)
    S.eng.sync_check()
    return {"coords": coords.clone(), "confs": confs.clone(), "conv": u.clone(), "conv statistics": stats.clone(),
            "stem_static": z0.clone(), "stem_update": x1.clone()}


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("L", CAPACITY_LENGTHS)
def test_exact_capacity_and_reused_context_give_the_same_bits(synth_sd, ctx128, L, precision):
    """A context that has just run a length-128 target, run at L, against a fresh context of capacity exactly (L, N):
    the same bits.  Workspaces are sized by the capacity and reused for every smaller target; a kernel that reads a
    stale element of a larger earlier target, or whose work split depends on the capacity, fails here."""
    from abi import Stages
    aln = _msa(L, N_ROWS, 3000 + L)
    shared = ctx128
    shared.eng.set_option("precision", precision)
    fresh = Stages(synth_sd, max_L=L, max_N=N_ROWS)
    fresh.eng.set_option("precision", precision)
    try:
        _run_target(shared, _msa(128, N_ROWS, 3128), 128)           # leaves the workspaces full of a larger target
        got = _run_target(shared, aln, L)
        want = _run_target(fresh, aln, L)
        for k in want:
            assert torch.equal(got[k], want[k]), f"{k} differs between a reused max_L = 128 context and a fresh " \
                                                 f"max_L = {L} context at L = {L}, precision {precision}"
        assert np.isfinite(want["coords"].cpu().numpy()).all()
    finally:
        shared.check_guards()
        fresh.check_guards()
        shared.eng.set_option("precision", 0)
        fresh.eng.close()
