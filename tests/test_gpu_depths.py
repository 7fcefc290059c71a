"""The front-end kernels against float64 references and the CPU oracle at the alignment depths where they branch, in all
three precisions.

The length sweep (tests/test_gpu_lengths.py) fixes the depth at N = 48; the front end chooses its tiles, loops, chunks
and units by N:
  reweighting (msa.hip)       64 x 64 row-pair tiles, cdiv(N, 64)^2 workgroups, rows past N padded with patterns that must
                              never match, a row's neighbours summed over tiles by atomicAdd, reciprocals in blocks of 256
  covariance (dca.hip)        256-thread strided loops over N (weight sum, column means), grid.y = N (centering)
  covariance product (gemm)   K = N: a K tail at N % 16 != 0, one accumulation level up to K = 256, a flush into a second
                              accumulator every 256 k above; every tile (dmp_cov_build) or the lower ones (dmp_dca_features)
  vertical GRU (vgru*.hip)    N is the time axis: layer 1 one row behind over rows 0 .. N, the result in the state buffer of
                              parity N & 1; the launch-per-row form in graphs of 128 rows, then of 16 with idle nodes past
                              N + 1
  front-end units (api.hip)   with vgru_persistent = 0, cdiv(N + 1, 128) GRU units alternating with the inverse's units
DEPTHS (tests/depth_ref.py) holds the depths on both sides of each of these, L = 13 (D = 273: three Gauss-Jordan blocks, the
last ragged; one GRU column tile) and L = 33 (two column tiles, the second with one column) the lengths.  Rows are
depth_ref.depth_msa's: synthetic rows with clusters of duplicates (the last row always in one), codes 20 and 21 both present.

Checks, every output a NaN-poisoned buffer with a guard tail (tests/abi.py) checked after each test:
  msa_weights      bit-equal to the oracle's reweight at every depth, at 3000 rows (47 x 47 tiles, the last of 56 rows) and on
                   the threshold family (pairs agreeing in exactly floor(0.8 L) and floor(0.8 L) + 1 positions, inside a tile
                   and across two)
  cov_build        the full product against the float64 cov_reg at 1e-5 of scale, fed the oracle's weights; exactly symmetric
  dca_features     lower tiles, inverse, contacts against the float64 inv_cov / contacts in the (L, L, 442) layout at 1e-5 of
                   scale; all zeros at N = 1
  gru_vertical     both forms (vgru_persistent 1 / 0) against the oracle's nn.GRU up to N = 257: 1e-5 in precision 0, 3e-6 in
                   precisions 1 and 2, which are also no further from the float64 recurrence than twice the oracle's own
                   distance + 1e-7; the two forms bit-equal in precisions 1 and 2, within 5e-6 in precision 0; no fault bit
  gru group        six alignments whose depths straddle a parity and a chunk boundary through one chain on one context: each
                   member bit-equal to the same alignment alone
  predictions      Engine.predict (one iteration, no refinement) against the oracle at the length sweep's end-to-end bounds,
                   with the engine's own w, inv_cov and contacts: L = 17 at the smallest depths, L = 40 (D = 840: two inverse
                   units) at N + 1 = 128, 129, 256, 258 (one, two, two, three GRU units) with and without the persistent form
  reuse            a shallow alignment on a context that has just run a deep one, bit for bit a fresh context of exactly the
                   shallow capacity

With -s, the module prints the largest error per check across the sweep next to its tolerance.  Measured on an MI355X
(375 cases, 22 s of wall time for the module, the CPU references included; no case's call above 0.8 s), error / tolerance and
where the largest occurred:
  cov_build vs float64                 7.5e-07 / 1.0e-05 = 0.08   L = 33, N = 257 (the first depth with a flush)
  dca_features couplings vs float64    4.2e-06 / 3.2e-05 = 0.13   L = 13, N = 256
  dca_features contacts vs float64     1.1e-06 / 1.0e-05 = 0.11   L = 33, N = 2 (cov_reg's condition number 143, else < 20)
  gru_vertical p0 vs oracle            1.4e-07 / 1.0e-05 = 0.014  L = 33, N = 257, per-row (persistent: 1.3e-07 at N = 17)
  gru_vertical p0 persistent / per-row 1.3e-07 / 5.0e-06 = 0.027  L = 33, N = 256
  gru_vertical p1, p2 vs oracle        3.0e-08 / 3.0e-06 = 0.010  L = 33, N = 16 (p1), L = 13, N = 31 (p2), both forms
  gru_vertical p1, p2 vs float64       2.4e-08 / 1.4e-07 = 0.18   L = 13, N = 145 (p1), N = 16 (p2), both forms
  group members                        as the same alignments alone (bit-equal); vs float64 at most 0.16 of the bound
  prediction inv_cov vs float64        4.3e-06 / 3.5e-05 = 0.12   L = 40, N = 257, persistent
  prediction contacts vs float64       7.6e-07 / 1.0e-05 = 0.08   L = 17, N = 2
  prediction conf                      1.9e-05 / 1.0e-04 = 0.19   L = 40, N = 255, precision 1, persistent
  prediction per-pass conf_means       2.5e-06 / 1.0e-03 = 0.003  L = 40, N = 255
  prediction CA-RMSD                   3.4e-04 / 1.0e-03 = 0.34   L = 40, N = 255, precision 0 per-row; precision 1: 3.4e-04
                                                                  at the same shape, precision 2: 2.3e-04 at N = 128
One check is within 3x of its bound, the CA-RMSD of the L = 40 predictions.  It is not an effect of the depth: at that
shape the engine's sequence weights are the oracle's bits and its inverse covariance is within 0.12 of the 1e-5 bound, the
exact-float32 precision 1 gives the same 3.4e-04 as the split-f16 precision 0, and __graft_entry__.smoke(), the same
length at N = 64, gives 2.7e-04: it is the float32 rounding of two trunk passes, the eigen-decomposition and the
coordinate GRU (coordinates of tens of Angstrom), the distance the end-to-end bound was set for.

What the sweep sees, from one run on scratch builds of the library with memory-safe defects (no address, bound or store
guard changed):
  gemm_kernel with nk = K / 16 (the K tail dropped)       the feature checks fail at every depth with N % 16 != 0 and pass
                                                          at 16, 32, 64, 128, 144, 256, 272, 512; every prediction fails
                                                          (the coordinate GRU's input projection has K = 520), and
                                                          the N = 2 reuse case (a zero product: NaN contacts)
  gemm_kernel without the flush's accumulate              the feature checks fail from N = 257 on (257, 272, 273, 511, 512,
                                                          513, 769) and nowhere below; every prediction fails (the
                                                          bidirectional GRUs' projections have K = 512 and 520)
  msa_count_kernel with >= for >                          the threshold family fails at L = 5, 10, 15, 20; so do the L = 40
                                                          predictions (0.8 x 40 is an integer, and synthetic rows do agree
                                                          in exactly 32 positions); nothing at L = 9, 13, 17, 33
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure)
import depth_ref as DR              # noqa: E402

PRECISIONS = [0, 1, 2]
FORMS = {1: "persistent", 0: "per-row"}


# ------------------------------------------------------------------------------------------------ worst errors
WORST = {}          # check -> (error / tolerance, error, tolerance, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest error per check across the depth sweep (error, tolerance, where):")
        for k in sorted(WORST):
            r, e, t, where = WORST[k]
            print(f"  {k:40s} {e:.3e}  tol {t:.1e}  ({r:5.3f} of it)  {where}")


def _check(name, err, tol, where):
    err = float(err)
    r = err / tol if np.isfinite(err) else float("inf")
    if name not in WORST or not r <= WORST[name][0]:
        WORST[name] = (r, err, tol, where)
    assert err <= tol, f"{name}: max error {err:.3e} > tolerance {tol:.1e} at {where}"


def _maxdiff(got, ref):
    got = got.detach().cpu().double() if isinstance(got, torch.Tensor) else torch.as_tensor(np.asarray(got)).double()
    ref = ref.detach().cpu().double() if isinstance(ref, torch.Tensor) else torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max())          # NaN (an unwritten element) propagates and fails every bound


def _scale(ref, rel):
    return rel * max(1.0, float(torch.as_tensor(ref).abs().max()))


def _where(L, N, p, form=None):
    return f"L={L} N={N} p={p}" + (f" {FORMS[form]}" if form is not None else "")


# ------------------------------------------------------------------------------------------------ references
class Ref:
    """The references of one (L, N), computed when first needed and shared by the precisions and forms."""

    def __init__(self, L, N, W):
        self.L, self.N, self.W = L, N, W
        self.aln = DR.depth_msa(L, N, DR.seed_of(L, N))
        self.w = O.reweight(self.aln)
        self._memo = {}

    def get(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def dca(self):
        """float64 (cov_reg, inv_cov, contacts) from the oracle's weights"""
        return self.get("dca", lambda: DR.dca(self.aln, self.w))

    def gru(self):
        """(the oracle's float32 nn.GRU, the float64 recurrence): the last row, (L, 512)"""
        def run():
            x = self.W["embed.weight"][torch.from_numpy(self.aln.astype(np.int64))]
            return O._gru(self.W, "vgru", x, 22, 512, 2, False, False)[-1], DR.vgru(self.W, self.aln)
        return self.get("gru", run)

    def prediction(self):
        def run():
            cap = {}
            coords, conf = O.predict(self.aln, self.W, None, 1, 0, "canonical", cap)
            return coords, conf, torch.stack((cap["p0.conf"].mean(), cap["p1.conf"].mean())), cap["w"].numpy()
        return self.get("prediction", run)


_REF = {}


def _ref(L, N, W):
    if (L, N) not in _REF:
        if len(_REF) >= 8:
            _REF.clear()                           # the sweeps run shape by shape: keep a few shapes' tensors
        _REF[(L, N)] = Ref(L, N, W)
    return _REF[(L, N)]


# ------------------------------------------------------------------------------------------------ context
@pytest.fixture(scope="module")
def ctx(synth_sd):
    from abi import Stages
    st = Stages(synth_sd, max_L=40, max_N=3000)
    assert st.eng.get_option("vgru_persistent") == 1          # a 256-CU device has the persistent form
    yield st
    st.eng.set_option("precision", 0)
    st.eng.sync_check()
    st.eng.close()


class _at:
    """The context in one precision for one test; afterwards the guard tails, precision 0, the persistent form, no fault."""

    def __init__(self, S, precision):
        self.S, self.p = S, precision

    def __enter__(self):
        self.S.eng.set_option("precision", self.p)
        return self.S

    def __exit__(self, *exc):
        self.S.check_guards()
        self.S.eng.set_option("precision", 0)
        self.S.eng.set_option("vgru_persistent", 1)
        if exc[0] is None:
            self.S.eng.sync_check()
        return False


def _form(S, persistent):
    S.eng.set_option("vgru_persistent", persistent)
    assert S.eng.get_option("vgru_persistent") == persistent


# ------------------------------------------------------------------------------------------------ stage checks
def _features(S, R, p):
    L, N, wh = R.L, R.N, _where(R.L, R.N, p)
    w = S.msa_weights(R.aln).cpu().numpy()
    assert np.array_equal(w, R.w), f"msa_weights differ from the oracle's at {wh}: rows {np.nonzero(w != R.w)[0][:8]}"
    if N == 1:
        assert not S.dca_features(R.aln).cpu().numpy().any(), f"dca_features of one row is not zero at {wh}"
        return
    cov64, inv64, con64 = R.dca()
    cov = S.cov_build(R.aln, S.to(R.w))
    _check("cov_build vs float64", _maxdiff(cov, cov64), _scale(cov64, 1e-5), wh)
    cov = cov.cpu()
    assert torch.equal(cov, cov.t()), f"cov_build: the full product is not exactly symmetric at {wh}"
    f = S.dca_features(R.aln).cpu()
    assert f.shape == (L, L, 442)
    # fast_dca's return value: channel 21a+b of pair (i, j) is inv_cov[21i+a, 21j+b], channel 441 the contacts
    fref = DR.dca_features(inv64, con64)
    _check("dca_features couplings vs float64", _maxdiff(f[:, :, :441], fref[:, :, :441]), _scale(inv64, 1e-5), wh)
    _check("dca_features contacts vs float64", _maxdiff(f[:, :, 441], con64), _scale(con64, 1e-5), wh)
    _check("dca_features vs float64", _maxdiff(f, fref), _scale(fref, 1e-5), wh)


def _gru_bounds(tag, got, ref, ref64, p, wh):
    """the bounds of tests/test_gpu_parity.py: 1e-5 for the split-f16 form; the float32 forms 3e-6 and no further from
    float64 than twice the reference's own float32 run + 1e-7"""
    _check(f"gru_vertical p{p} {tag} vs oracle", _maxdiff(got, ref), 1e-5 if p == 0 else 3e-6, wh)
    if p:
        _check(f"gru_vertical p{p} {tag} vs float64", _maxdiff(got, ref64), 2.0 * _maxdiff(ref, ref64) + 1e-7, wh)


def _gru_forms_agree(a, b, p, wh):
    if p:
        assert torch.equal(a, b), f"gru_vertical: the persistent and the launch-per-row form differ at {wh}"
    else:
        _check("gru_vertical p0 persistent vs per-row", _maxdiff(a, b), 5e-6, wh)


def _gru(S, R, p):
    ref, ref64 = R.gru()
    out = {}
    for persistent in (1, 0):
        _form(S, persistent)
        out[persistent] = S.gru_vertical(R.aln)
        assert S.eng.sync_faults() == 0, _where(R.L, R.N, p, persistent)
        _gru_bounds(FORMS[persistent], out[persistent], ref, ref64, p, _where(R.L, R.N, p, persistent))
    _gru_forms_agree(out[1], out[0], p, _where(R.L, R.N, p))


CHECKS = {"features": _features, "gru_vertical": _gru}


def _stage_cases():
    out = []
    for L in DR.LENGTHS:
        for N in [1] + DR.DEPTHS:
            for p in PRECISIONS:
                for s in ["features"] + (["gru_vertical"] if N <= DR.GRU_MAX_DEPTH else []):
                    out.append(pytest.param(L, N, p, s, id=f"L{L}-N{N}-p{p}-{s}"))
    return out


@pytest.mark.parametrize("L,N,precision,stage", _stage_cases())
def test_stage_vs_reference_at_depth(ctx, oracle_weights, L, N, precision, stage):
    R = _ref(L, N, oracle_weights)
    with _at(ctx, precision) as S:
        CHECKS[stage](S, R, precision)


# ------------------------------------------------------------------------------------------------ reweighting
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("L", DR.THRESHOLD_LENGTHS)
def test_msa_weights_on_the_threshold(ctx, L, precision):
    """Pairs of rows that agree in exactly floor(0.8 L) positions are no neighbours (count > float32(0.8 L) is strict,
    also at L % 5 == 0 where the two are equal), pairs that agree in one more are; inside one 64-row tile and across
    rows 63 | 64; at L % 4 != 0 the packed words carry pad bytes."""
    a, pairs = DR.threshold_msa(L)
    ref = O.reweight(a)
    with _at(ctx, precision) as S:
        w = S.msa_weights(a).cpu().numpy()
    for r, s, extra in pairs:
        want = np.float32(0.5 if extra else 1.0)
        assert ref[r] == ref[s] == want
        assert w[r] == w[s] == want, f"rows {r}, {s} agree in floor(0.8 L) + {extra} of L = {L}: weights {w[r]}, {w[s]}"
    assert np.array_equal(w, ref), f"msa_weights differ at L = {L}: rows {np.nonzero(w != ref)[0][:8]}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_msa_weights_at_3000_rows(ctx, precision):
    """47 x 47 tiles, the last with 56 rows; the reciprocals in 12 blocks, the last with 184 rows."""
    a = DR.depth_msa(9, 3000, DR.seed_of(9, 3000))
    ref = O.reweight(a)
    assert ref[-1] < 1 and len(np.unique(ref)) > 8
    with _at(ctx, precision) as S:
        w = S.msa_weights(a).cpu().numpy()
    assert np.array_equal(w, ref), f"msa_weights differ at N = 3000: rows {np.nonzero(w != ref)[0][:8]}"


# ------------------------------------------------------------------------------------------------ one chain, six depths
@pytest.mark.parametrize("persistent", [1, 0])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_grouped_vertical_gru_members_at_mixed_depths(ctx, oracle_weights, precision, persistent):
    """dmp_gru_vertical_group on one context with depths 127, 128, 129, 1, 2, 16: members end at either parity, before and
    after the first 128-row chunk, and idle for most of the chain.  Each member is bit-equal to the same alignment alone
    and inside the oracle's bounds."""
    refs = [_ref(L, N, oracle_weights) for L, N in DR.GROUP_SHAPES]
    with _at(ctx, precision) as S:
        _form(S, persistent)
        grouped = S.gru_vertical_group([R.aln for R in refs])
        assert S.eng.sync_faults() == 0
        for R, g in zip(refs, grouped):
            wh = _where(R.L, R.N, precision, persistent)
            alone = S.gru_vertical(R.aln)
            assert torch.equal(g, alone), f"gru_vertical_group: a member differs from the alignment alone at {wh}"
            _gru_bounds("group member", g, *R.gru(), precision, wh)
        assert S.eng.sync_faults() == 0


# ------------------------------------------------------------------------------------------------ predictions
def _prediction_cases():
    out = []
    for L, N in DR.PREDICT_SHAPES:
        for p in PRECISIONS:
            for persistent in ([1] if L == 17 else [1, 0]):
                out.append(pytest.param(L, N, p, persistent, id=f"L{L}-N{N}-p{p}-{FORMS[persistent]}"))
    return out


@pytest.mark.parametrize("L,N,precision,persistent", _prediction_cases())
def test_prediction_at_depth(ctx, oracle_weights, L, N, precision, persistent):
    """Engine.predict through the front-end units.  With vgru_persistent = 0 the covariance features run on the side stream
    and their units (at L = 40: two, of six and one Gauss-Jordan block) alternate with the GRU's cdiv(N + 1, 128)."""
    R = _ref(L, N, oracle_weights)
    coords_ref, conf_ref, means_ref, w_ref = R.prediction()
    cov64, inv64, con64 = R.dca()
    wh = _where(L, N, precision, persistent)
    with _at(ctx, precision) as S:
        _form(S, persistent)
        coords, confs = S.eng.predict(R.aln, None, 1, 0)
        S.eng.sync_check()
        d = coords.cpu()[:, 1].double() - coords_ref[:, 1].double()
        _check(f"prediction p{precision} CA-RMSD", float((d ** 2).sum(-1).mean().sqrt()), 1e-3, wh)
        _check(f"prediction p{precision} conf", _maxdiff(confs, conf_ref), 1e-4, wh)
        _check("prediction per-pass conf_means", _maxdiff(S.eng.fetch("conf_means", 2), means_ref), 1e-3, wh)
        w = S.eng.fetch("w", N).cpu().numpy()
        assert np.array_equal(w, w_ref) and np.array_equal(w, R.w), f"the engine's sequence weights differ at {wh}"
        inv = S.eng.fetch("inv_cov", (21 * L) ** 2).view(21 * L, 21 * L)
        _check("prediction inv_cov vs float64", _maxdiff(inv, inv64), _scale(inv64, 1e-5), wh)
        con = S.eng.fetch("contacts", L * L).view(L, L)
        _check("prediction contacts vs float64", _maxdiff(con, con64), _scale(con64, 1e-5), wh)


# ------------------------------------------------------------------------------------------------ shallow after deep
def _run_alignment(S, aln):
    """Every front-end stage and a prediction on one alignment: the outputs to compare bit for bit."""
    N, L = aln.shape
    out = {"msa_weights": S.msa_weights(aln).clone()}
    if N > 1:                                                     # (one row has no covariance: num_points = 0)
        out["cov_build"] = S.cov_build(aln, out["msa_weights"]).clone()
    out["dca_features"] = S.dca_features(aln).clone()
    for persistent in (1, 0):
        _form(S, persistent)
        out[f"gru_vertical {FORMS[persistent]}"] = S.gru_vertical(aln).clone()
        coords, confs = S.eng.predict(aln, None, 1, 0)
        out[f"coords {FORMS[persistent]}"], out[f"confs {FORMS[persistent]}"] = coords.clone(), confs.clone()
        out[f"w {FORMS[persistent]}"] = S.eng.fetch("w", N).clone()
        if N > 1:
            out[f"inv_cov {FORMS[persistent]}"] = S.eng.fetch("inv_cov", (21 * L) ** 2).clone()
            out[f"contacts {FORMS[persistent]}"] = S.eng.fetch("contacts", L * L).clone()
    _form(S, 1)
    S.eng.sync_check()
    return out


@pytest.fixture(scope="module")
def ctx_deep(synth_sd):
    from abi import Stages
    st = Stages(synth_sd, max_L=DR.REUSE_DEEP[0], max_N=DR.REUSE_DEEP[1])
    yield st
    st.eng.set_option("precision", 0)
    st.eng.sync_check()
    st.eng.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", DR.REUSE_DEPTHS)
def test_shallow_alignment_after_a_deep_one_gives_the_same_bits(synth_sd, ctx_deep, N, precision):
    """A context that has just run the L = 40, N = 300 target, run at L = 33 and N rows, against a fresh context of capacity
    exactly (33, N): the same bits.  The workspaces are sized by the capacity and reused: a kernel that reads a stale row
    of the centred alignment, of the packed words or of the neighbour counts, a stale GRU state tile, or that indexes a
    buffer sized from max_N past N, fails here."""
    from abi import Stages
    L = DR.REUSE_LENGTH
    deep = DR.depth_msa(*DR.REUSE_DEEP, DR.seed_of(*DR.REUSE_DEEP))
    aln = DR.depth_msa(L, N, DR.seed_of(L, N))
    fresh = Stages(synth_sd, max_L=L, max_N=N)
    fresh.eng.set_option("precision", precision)
    try:
        with _at(ctx_deep, precision) as shared:
            _run_alignment(shared, deep)                          # leaves the workspaces full of a deeper, longer target
            got = _run_alignment(shared, aln)
            want = _run_alignment(fresh, aln)
            assert got.keys() == want.keys()
            for k in want:
                assert torch.equal(got[k], want[k]), f"{k} differs between a context that has just run L = 40, N = 300 " \
                                                     f"and a fresh max_N = {N} context at N = {N}, precision {precision}"
            assert np.isfinite(want["coords persistent"].cpu().numpy()).all()
    finally:
        fresh.check_guards()
        fresh.eng.close()
