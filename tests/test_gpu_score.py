"""A prediction scored against a native structure on the GPU (option "score_native"; include/dmpfold_hip.h).

Every number is compared with the float64 yardstick of tests/test_score_cpu.py, fed the float32 model trace the GPU
returned and the same native: integer-derived outputs exactly, the others within one float32 ulp (the bounds and why:
compare_with_yardstick).  The largest differences seen are printed; profiles/score.txt keeps them.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_rows
from test_score_cpu import _rotation, _tool, compare_with_yardstick, yardstick

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: encode_aln)

from dmpfold2_amd import score as S  # noqa: E402

GUARD = 4096
PRECISIONS = [0, 1, 2]
LENGTHS = [8, 31, 32, 33, 63, 64, 65, 255, 256, 257]


def _tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


@pytest.fixture(scope="module")
def eng(synth_sd):
    """One engine (seed-0 weights, precision 2) for the single-engine tests."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 300, 64)
    e.set_weights(_tensors(synth_sd))
    e.set_option("precision", 2)
    yield e
    e.close()


def _one_row(L):
    from dmpfold2_amd import synth
    return np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L)))


def _random_walk(L, seed, step=3.8, clash=3.0):
    """A self-avoiding walk of fixed step length: a step that comes within `clash` of an earlier point is drawn again."""
    rng = np.random.default_rng(seed)
    pts = [np.zeros(3)]
    while len(pts) < L:
        for _ in range(200):
            v = rng.normal(size=3)
            p = pts[-1] + step * v / np.linalg.norm(v)
            if len(pts) < 2 or np.linalg.norm(np.asarray(pts[:-1]) - p, axis=1).min() > clash:
                break
        pts.append(p)
    return np.asarray(pts, dtype=np.float32)


def _moved(model, seed, shift=(11.0, -7.0, 5.0)):
    R = _rotation(seed)
    return R, np.asarray(shift), (model.astype(np.float64) @ R.T + np.asarray(shift)).astype(np.float32)


def _perturbed_copy(model, seed):
    """The model rigidly moved, about 30 % of its residues displaced by 3-20 A, every seventh row absent."""
    rng = np.random.default_rng(seed)
    _, _, nat = _moved(model, seed)
    L = len(model)
    pick = rng.random(L) < 0.3
    v = rng.normal(size=(L, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    nat = nat + (pick[:, None] * v * rng.uniform(3.0, 20.0, size=(L, 1))).astype(np.float32)
    nat[::7] = np.nan
    return nat.astype(np.float32)


def _scored(eng, aln, native, iterations=0, minsteps=0, **kw):
    """(coords, confs, scores dict) of a prediction with `native`; the option is off again afterwards."""
    out = eng.predict(aln, None, iterations, minsteps, native=native, **kw)
    eng.sync_check()
    assert eng.get_option("score_native") == 0
    return out, eng.scores


def _check(eng_scores, coords, native, lnorm, tag):
    want, margin = yardstick(coords[:, 1].cpu().numpy(), native, lnorm)
    seen = compare_with_yardstick(eng_scores, want, margin, tag)
    print(tag, "margin %.2e A, largest differences in float32 ulps:" % margin, seen, file=sys.stderr)
    return want


# ------------------------------------------------------------------------------------------------ 1. real geometry
@pytest.mark.parametrize("precision", PRECISIONS)
def test_real_geometry_against_3fgx(synth_sd, precision):
    """The benchmark's minimiser setting on weights whose first trace approximates 3FGX chain A, scored against that
    chain: every output against the yardstick, tm not below the tool's reduced search, and the structure bit for bit
    the one of the run without the option.  (On the parent commit the option is unknown: the call raises.)"""
    from dmpfold2_amd.predict import Engine
    g = load_golden("fit3fgx_L96_N50_n0_m100")
    sd = dict(synth_sd)
    sd["coord_fc.weight"] = g["coord_fc"]
    native = load_golden("kat_refine_backbone")["ca_in"].astype(np.float32)
    e = Engine("cuda:0", 96, 64)
    try:
        e.set_weights(_tensors(sd))
        e.set_option("precision", precision)
        plain = e.predict(g["alnmat"], None, 0, 100)
        e.sync_check()
        assert e.scores is None and e.score_block is None
        (coords, confs), sc = _scored(e, g["alnmat"], (native, 96.0), 0, 100)
        assert torch.equal(coords, plain[0]) and torch.equal(confs, plain[1]) and tuple(confs.shape) == (96,)
        assert sc["n_pairs"] == 96 and sc["lnorm"] == 96.0 and np.array_equal(sc["native"], native)
        _check(sc, coords, native, 96.0, f"3fgx p{precision}")
        ca = coords[:, 1].cpu().numpy().astype(np.float64)
        reduced = _tool().tm_score(ca, native.astype(np.float64), 96.0)
        print(f"3fgx p{precision}: tm {sc['tm']:.6f} (tool's reduced search {reduced:.6f}) rmsd {sc['rmsd']:.4f} "
              f"gdt_ts {sc['gdt_ts']:.4f} lddt {sc['lddt']:.4f}", file=sys.stderr)
        assert sc["tm"] >= np.float32(reduced) - np.spacing(np.float32(reduced))
        assert sc["tm"] > 0.5                                      # the fitted trace really resembles the chain
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. length sweep
_TRACES = {}


def _trace(eng, L):
    """The plain prediction of the one-row alignment of length L, made once: (aln, coords, confs)."""
    if L not in _TRACES:
        aln = _one_row(L)
        coords, confs = eng.predict(aln, None, 0, 0)
        eng.sync_check()
        _TRACES[L] = (aln, coords.clone(), confs.clone())
    return _TRACES[L]


@pytest.mark.parametrize("kind", ["perturbed_copy", "random_walk"])
@pytest.mark.parametrize("L", LENGTHS)
def test_length_sweep(eng, L, kind):
    aln, coords0, confs0 = _trace(eng, L)
    model = coords0[:, 1].cpu().numpy()
    native = _perturbed_copy(model, 100 + L) if kind == "perturbed_copy" else _random_walk(L, 200 + L)
    (coords, confs), sc = _scored(eng, aln, native)
    assert torch.equal(coords, coords0) and torch.equal(confs, confs0)
    want = _check(sc, coords, native, 0.0, f"sweep L={L} {kind}")
    assert sc["lnorm"] == 0.0 and sc["n_pairs"] == want["n_pairs"] == int((~np.isnan(native[:, 0])).sum())
    assert np.array_equal(np.isnan(sc["deviation"]), np.isnan(native[:, 0]))


# ------------------------------------------------------------------------------------------------ 3. rigid copies
def _rigid_properties(sc, n, R, t):
    assert sc["n_pairs"] == n
    assert sc["tm"] >= 1.0 - 1e-6 and sc["rmsd"] <= 1e-4 and sc["lddt"] == 1.0
    assert sc["counts"] == [n] * 5 and sc["gdt_ts"] == 1.0 and sc["gdt_ha"] == 1.0
    assert np.abs(sc["R"] - R).max() <= 1e-5 and np.abs(sc["t"] - t).max() <= 1e-5
    assert float(sc["deviation"].max()) <= 1e-3 and bool((sc["lddt_res"] == 1.0).all())


def test_rigid_copy_L64(eng):
    aln, coords0, _ = _trace(eng, 64)
    model = coords0[:, 1].cpu().numpy()
    R, t, native = _moved(model, 7)
    (coords, _), sc = _scored(eng, aln, native)
    assert torch.equal(coords, coords0)
    _rigid_properties(sc, 64, R, t)
    _check(sc, coords, native, 0.0, "rigid L=64")


def test_rigid_copy_L2048(synth_sd):
    """The only place the LDS and seed-record capacities are reached: 8262 seeds, 6 x 2048 floats and 2048 flags of LDS.
    No yardstick here (it would take minutes), the properties of a rigid copy instead."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 2048, 1)
    try:
        e.set_weights(_tensors(synth_sd))
        e.set_option("precision", 2)
        aln = _one_row(2048)
        coords0, _ = e.predict(aln, None, 0, 0)
        e.sync_check()
        model = coords0[:, 1].cpu().numpy()
        R, t, native = _moved(model, 9)
        (coords, _), sc = _scored(e, aln, native)
        assert torch.equal(coords, coords0)
        print("rigid L=2048: tm", sc["tm"], "rmsd", sc["rmsd"], "max|coordinate|", float(np.abs(model).max()),
              "max|R - R0|", float(np.abs(sc["R"] - R).max()), "max|t - t0|", float(np.abs(sc["t"] - t).max()), file=sys.stderr)
        assert sc["n_pairs"] == 2048 and sc["tm"] >= 1.0 - 1e-6 and sc["rmsd"] <= 1e-4 and sc["lddt"] == 1.0
        assert sc["counts"] == [2048] * 5
        assert np.abs(sc["R"] - R).max() <= 1e-5 and np.abs(sc["t"] - t).max() <= 1e-5
        assert not np.isnan(sc["deviation"]).any() and bool((sc["lddt_res"] == 1.0).all())
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. edges
def _out_slots(block, L):
    return block[3 * L + 1:]


def test_too_few_pairs_and_lnorm_zero(eng):
    L = 33
    aln, coords0, confs0 = _trace(eng, L)
    walk = _random_walk(L, 5)
    for keep in (0, 2):
        native = np.full((L, 3), np.nan, dtype=np.float32)
        native[4:4 + keep] = walk[4:4 + keep]
        (coords, confs), sc = _scored(eng, aln, native)
        assert torch.equal(coords, coords0) and torch.equal(confs, confs0)
        blk = eng.score_block.cpu().numpy()
        assert blk[3 * L + 1] == float(keep) and sc["n_pairs"] == keep
        assert np.isnan(_out_slots(blk, L)[1:]).all()
        assert np.array_equal(blk[:3 * L].reshape(L, 3), native, equal_nan=True) and blk[3 * L] == 0.0
    native = walk.copy()
    native[::5] = np.nan
    n = int((~np.isnan(native[:, 0])).sum())
    _, sc0 = _scored(eng, aln, native)
    blk0 = eng.score_block.cpu().numpy().copy()
    _, scn = _scored(eng, aln, (native, float(n)))
    blkn = eng.score_block.cpu().numpy()
    assert sc0["n_pairs"] == n and np.array_equal(_out_slots(blk0, L), _out_slots(blkn, L), equal_nan=True)
    assert blk0[3 * L] == 0.0 and blkn[3 * L] == float(n)


def test_option_values(eng):
    from dmpfold2_amd import _lib
    for bad in (2, -1):
        with pytest.raises(_lib.DmpError):
            eng.set_option("score_native", bad)
    assert eng.get_option("score_native") == 0
    eng.set_option("score_native", 1)
    assert eng.get_option("score_native") == 1
    eng.set_option("score_native", 0)


def test_raw_buffer_is_exactly_the_block(eng):
    """dmp_predict into a poisoned buffer: L + 5L + 24 floats used, the guard behind them intact, the inputs untouched;
    with the option on and no native given through Python the block reads as 'no row present'."""
    L = 31
    aln, coords0, confs0 = _trace(eng, L)
    native = _random_walk(L, 3)
    n_out = S.conf_floats(L, False, True)
    d_msa = torch.from_numpy(aln).to(eng.device)
    coords = torch.full((15 * L + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    buf = torch.full((n_out + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    buf[L:n_out] = torch.from_numpy(S.pack_native(native, 0.0, L)).to(eng.device)
    eng.set_option("score_native", 1)
    try:
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 0, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
        assert rc == 0, eng.lib.dmp_last_error()
        eng.sync_check()
        assert bool(torch.isnan(buf[n_out:]).all()) and bool(torch.isnan(coords[15 * L:]).all())
        assert torch.equal(buf[:L], confs0) and torch.equal(coords[:15 * L].view(L, 5, 3), coords0)
        sc = S.unpack_scores(buf[L:n_out], L)
        assert np.array_equal(sc["native"], native) and sc["n_pairs"] == L
        _check(sc, coords0, native, 0.0, "raw L=31")
        out = eng.predict(aln, None, 0, 0)                         # the option set by hand, no native
        eng.sync_check()
        assert len(out) == 2 and tuple(out[1].shape) == (L,) and eng.scores["n_pairs"] == 0 and np.isnan(eng.scores["tm"])
    finally:
        eng.set_option("score_native", 0)


# ------------------------------------------------------------------------------------------------ 5. with the other options
def test_with_distmap_and_convergence_stop(eng):
    """Offsets with "emit_distmap" on as well; the map and the structure are those of the runs without scoring; under
    "recycle_tol_mA" the scores are those of the plain run that ends with the pass the stop came at."""
    L = 65
    aln = _one_row(L)
    native = _random_walk(L, 21)
    native[::9] = np.nan
    c0, f0, dm0, info0 = eng.predict(aln, None, 2, 0, distmap=True)
    eng.sync_check()
    c0, f0, dm0, info0 = c0.clone(), f0.clone(), dm0.clone(), info0.clone()
    (c1, f1, dm1, info1), sc1 = _scored(eng, aln, native, 2, 0, distmap=True)
    assert eng.get_option("emit_distmap") == 0
    for a, b in ((c0, c1), (f0, f1), (dm0, dm1), (info0, info1)):
        assert torch.equal(a, b)
    assert f1.untyped_storage().nbytes() >= 4 * S.conf_floats(L, True, True)
    assert eng.score_block.data_ptr() == f1.data_ptr() + 4 * (S.score_offset(L, True) - 0)
    _check(sc1, c1, native, 0.0, "with distmap L=65")
    (c2, f2), sc2 = _scored(eng, aln, native, 2, 0)
    blk2 = eng.score_block.cpu().numpy().copy()
    assert torch.equal(c2, c0) and np.array_equal(S.unpack_scores(blk2, L)["deviation"], sc1["deviation"], equal_nan=True)
    assert sc2["tm"] == sc1["tm"] and sc2["counts"] == sc1["counts"]
    # a tolerance so wide that the first comparison stops the recycling: passes 0 and 1 run
    (c3, f3), sc3 = _scored(eng, aln, native, 6, 0, converge=1e3)
    blk3 = eng.score_block.cpu().numpy().copy()
    assert eng.passes_run == 2 and eng.get_option("recycle_tol_mA") == 0
    (c4, f4), sc4 = _scored(eng, aln, native, 1, 0)
    assert torch.equal(c3, c4) and torch.equal(f3, f4)
    assert np.array_equal(blk3, eng.score_block.cpu().numpy(), equal_nan=True)


# ------------------------------------------------------------------------------------------------ 6. pipeline
@pytest.mark.parametrize("streams", [2, 4])
def test_pipeline(synth_sd, streams):
    """Six targets of mixed length, each with a native of its own: every ticket's score block is bit for bit the lone
    context's; a target submitted without a native reads 'no row present'; with the option off `result` has its old shape."""
    from dmpfold2_amd.predict import Engine, Pipeline
    lengths = [40, 24, 64, 33, 40, 57]
    alns = [_one_row(L) for L in lengths]
    natives = []
    for k, L in enumerate(lengths):
        nat = _random_walk(L, 300 + k)
        nat[k::6] = np.nan
        natives.append((nat, float(L + k)))
    dev = torch.device("cuda:0")
    sdt = _tensors(synth_sd)
    single = Engine(dev, 64, 1)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 64, 1, sdt, streams=streams, precision=2)
    try:
        refs = []
        for aln, nat in zip(alns, natives):
            c, f = single.predict(aln, None, 1, 0, native=nat)
            single.sync_check()
            refs.append((c.clone(), f.clone(), single.score_block.clone()))
        assert all(e.get_option("score_native") == 0 for e in pipe.engines)
        t = pipe.submit(torch.from_numpy(alns[0]).to(dev), 1, 0, native=natives[0])          # ignored: the option is off
        pipe.drain()
        pipe.sync_check()
        old = pipe.result(t)
        assert len(old) == 2 and torch.equal(old[0], refs[0][0]) and torch.equal(old[1], refs[0][1])
        pipe.set_score(True)
        assert all(e.get_option("score_native") == 1 for e in pipe.engines)
        tickets = [pipe.submit(torch.from_numpy(a).to(dev), 1, 0, native=n) for a, n in zip(alns, natives)]
        res = pipe.collect(tickets)
        for t, ref, L in zip(tickets, refs, lengths):
            assert not isinstance(res[t], Exception), res[t]
            coords, confs, block = res[t]
            assert tuple(confs.shape) == (L,) and tuple(block.shape) == (5 * L + 24,)
            assert torch.equal(coords, ref[0]) and torch.equal(confs, ref[1])
            assert np.array_equal(block.cpu().numpy(), ref[2].cpu().numpy(), equal_nan=True), L
        t = pipe.submit(torch.from_numpy(alns[1]).to(dev), 1, 0)
        pipe.drain()
        pipe.sync_check()
        coords, confs, block = pipe.result(t)
        sc = S.unpack_scores(block, lengths[1])
        assert sc["n_pairs"] == 0 and np.isnan(sc["tm"]) and torch.equal(coords, refs[1][0])
        pipe.set_score(False)
        out = pipe.run([torch.from_numpy(alns[2]).to(dev)], 1, 0)
        pipe.sync_check()
        assert len(out[0]) == 2 and torch.equal(out[0][0], refs[2][0])
    finally:
        pipe.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 6b. all three options
@pytest.fixture(scope="module")
def single_and_pipe(synth_sd):
    """A lone engine with "tridiag_cluster" 0, as the scheduler's engines, and a two-stream pipeline with the three options on."""
    from dmpfold2_amd.predict import Engine, Pipeline
    dev, sdt = torch.device("cuda:0"), _tensors(synth_sd)
    single = Engine(dev, 96, 16)
    single.set_weights(sdt)
    single.set_option("precision", 2)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, 96, 16, sdt, streams=2, precision=2, converge=BOUNDARY_TOL, distmap=True, score=True)
    yield single, pipe
    pipe.close()
    single.close()


BOUNDARY_TOL = 1e-3         # Angstrom: "recycle_tol_mA" = 1


def _bits(x):
    return (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("L", [8, 63, 64, 96])
def test_all_three_options_at_workgroup_boundaries(single_and_pipe, L):
    """N = 16, -n 2 -m 0 with "recycle_tol_mA", "emit_distmap" and "score_native" on, the native the model's own trace moved
    rigidly.  L = 8: the network's minimum, fewer rows than threads; 63 / 64: one and two workgroups in the reductions of
    recycle_delta and emit_distmap; 96: three, an odd count of partial sums.  The engine's result, the raw buffer of a
    dmp_predict call and the pipeline's result agree bit for bit in every part (NaN slots included); the guard behind
    conf_floats(L, True, True) floats stays; map_rms and pass_delta[1:] agree with their float64 restatements at the
    bounds of test_gpu_distmap.py (1e-6 relative) and test_gpu_recycle_converge.py (1e-5 relative)."""
    from dmpfold2_amd import synth
    from test_recycle_converge_cpu import recycle_deltas
    single, pipe = single_and_pipe
    aln = np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 16, 2000 + L)))
    plain, _ = single.predict(aln, None, 2, 0)
    single.sync_check()
    R, t, native = _moved(plain[:, 1].cpu().numpy(), 30 + L)
    coords, confs, dm, info = single.predict(aln, None, 2, 0, converge=BOUNDARY_TOL, distmap=True, native=native)
    single.sync_check()
    assert [single.get_option(k) for k in ("recycle_tol_mA", "emit_distmap", "score_native")] == [0, 0, 0]
    block, sc, P = single.score_block, single.scores, single.passes_run
    assert sc["n_pairs"] == L and info[1].item() == float(P) and 2 <= P <= 3
    # the float64 restatements
    ca = coords[:, 1].cpu().numpy().astype(np.float64)
    d = ca[:, None, :] - ca[None, :, :]
    iu = np.triu_indices(L, 1)
    e = dm.cpu().numpy().astype(np.float64)[iu] - np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[iu]
    want_rms = float(np.sqrt((e * e).mean()))
    delta = single.fetch("pass_delta", P).cpu().numpy()
    own = recycle_deltas(single.fetch("ca_pass", P * L * 3).cpu().numpy().reshape(P, L, 3))
    print("L", L, "passes", P, "map_rms", float(info[2]), "restated", want_rms, "pass_delta", delta, "restated", own, file=sys.stderr)
    assert abs(float(info[2]) - want_rms) <= 1e-6 * want_rms
    assert delta.shape == (P,) and np.isinf(delta[0]) and (np.abs(delta[1:] - own[1:]) <= 1e-5 * own[1:]).all(), (delta, own)
    # the raw call into a poisoned buffer: the same bits, nothing behind the layout's end
    n_out = S.conf_floats(L, True, True)
    d_msa = torch.from_numpy(aln).to(single.device)
    raw_c = torch.full((15 * L + GUARD,), float("nan"), dtype=torch.float32, device=single.device)
    buf = torch.full((n_out + GUARD,), float("nan"), dtype=torch.float32, device=single.device)
    buf[S.score_offset(L, True):n_out] = torch.from_numpy(S.pack_native(native, 0.0, L)).to(single.device)
    for k, v in (("recycle_tol_mA", 1), ("emit_distmap", 1), ("score_native", 1)):
        single.set_option(k, v)
    try:
        rc = single.lib.dmp_predict(single.ctx, d_msa.data_ptr(), 16, L, None, 0, 2, 0, raw_c.data_ptr(), buf.data_ptr(), single.stream())
        assert rc == 0, single.lib.dmp_last_error()
        single.sync_check()
    finally:
        for k in ("recycle_tol_mA", "emit_distmap", "score_native"):
            single.set_option(k, 0)
    assert bool(torch.isnan(buf[n_out:]).all()) and bool(torch.isnan(raw_c[15 * L:]).all()), "a guard float was written"
    whole = np.concatenate([_bits(x) for x in (confs, dm, info, block)])
    assert whole.size == n_out and np.array_equal(_bits(buf[:n_out]), whole) and np.array_equal(_bits(raw_c[:15 * L]), _bits(coords))
    # the pipeline
    ticket = pipe.submit(d_msa, 2, 0, native=native)
    res = pipe.collect([ticket])[ticket]
    assert not isinstance(res, Exception), res
    assert len(res) == 5 and [tuple(x.shape) for x in res] == [(L, 5, 3), (L,), (L, L), (3,), (5 * L + 24,)]
    for name, a, b in zip(("coords", "confs", "distmap", "info", "score block"), res, (coords, confs, dm, info, block)):
        assert np.array_equal(_bits(a), _bits(b)), (L, name)


# ------------------------------------------------------------------------------------------------ 7. software-latched fault
def test_latched_fault_gives_nan_in_every_out_slot(eng):
    """A residue code of 22 raises the device-side flag DMP_FAULT_BAD_CODE (a software flag, not a GPU fault): every out
    slot of the score block is NaN, the native and lnorm are as the caller wrote them, the guard stays."""
    from dmpfold2_amd.predict import FAULT_BAD_CODE
    L = 33
    aln = _one_row(L).copy()
    aln[0, 5] = 22
    native = _random_walk(L, 8)
    native[3] = np.nan
    n_out = S.conf_floats(L, False, True)
    inputs = S.pack_native(native, 40.0, L)[:3 * L + 1]
    eng.set_option("score_native", 1)
    try:
        d_msa = torch.from_numpy(aln).to(eng.device)
        coords = torch.zeros((L, 5, 3), dtype=torch.float32, device=eng.device)
        buf = torch.zeros((n_out + GUARD,), dtype=torch.float32, device=eng.device)
        buf[n_out:] = 7.0
        buf[L:L + 3 * L + 1] = torch.from_numpy(inputs).to(eng.device)
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, L, None, 0, 1, 0, coords.data_ptr(), buf.data_ptr(), eng.stream())
        assert rc == 0
        assert eng.sync_faults() == FAULT_BAD_CODE
        h = buf.cpu().numpy()
        assert bool(torch.isnan(coords).all()) and np.isnan(h[:L]).all()
        assert np.array_equal(h[L:L + 3 * L + 1], inputs, equal_nan=True), "the inputs were touched"
        assert np.isnan(h[L + 3 * L + 1:n_out]).all()
        assert (h[n_out:] == 7.0).all(), "the NaN fill went past the score block"
    finally:
        eng.set_option("score_native", 0)
    (c, f), sc = _scored(eng, _one_row(L), native)                  # the next prediction on the engine is whole again
    _check(sc, c, native, 0.0, "after a fault L=33")


# ------------------------------------------------------------------------------------------------ 8. front ends
def _write_pdb(path, seq, ca, chain="A"):
    three = dict(zip(S.AA1, S.AA3))
    with open(path, "w") as fh:
        for k, (aa, xyz) in enumerate(zip(seq, ca)):
            fh.write("ATOM  %5d  CA  %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n"
                     % (k + 1, three[aa], chain, k + 1, xyz[0], xyz[1], xyz[2]))
        fh.write("TER\nEND\n")


def test_front_ends(tmp_path, weights_file, monkeypatch):
    """`dmpfold --native`: stdout byte for byte the run's without it, the JSON line (stderr or --scores FILE) the numbers
    of Engine.scores; aln_to_coords(native=, return_scores=True); `dmpfold-batch --natives`: summary, npz arrays and
    <stem>.scores.json carry the same numbers, and the target without a native file is predicted and left unscored."""
    import dmpfold2_amd.predict as P
    from dmpfold2_amd import aln_to_coords, run_dmpfold
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", "2")
    P._ENGINES.clear()
    try:
        paths, queries = [], {}
        for name, stem in (("pf10963_n3_m0", "pf"), ("synth_L40_N64_n2_m0", "s40")):
            rows = golden_rows(load_golden(name))
            p = tmp_path / f"{stem}.aln"
            p.write_text("\n".join(rows) + "\n")
            paths.append(str(p))
            queries[stem] = rows[0]
        natives = tmp_path / "natives"
        natives.mkdir()
        q = queries["pf"]
        seq = q[2:30] + q[33:]                                         # the structure lacks both ends' worth and a loop
        seq = seq[:10] + ("A" if seq[10] != "A" else "G") + seq[11:]   # and carries a mutation
        walk = _random_walk(len(seq), 77)
        _write_pdb(str(natives / "pf.pdb"), seq, walk)
        kw = dict(device="cuda:0", iterations=1, minsteps=0, weights_file=weights_file)
        plain = aln_to_coords(paths[0], **kw)
        c, f, sc = aln_to_coords(paths[0], native=str(natives / "pf.pdb"), return_scores=True, **kw)
        assert torch.equal(c, plain[0]) and torch.equal(f, plain[1]) and len(aln_to_coords(paths[0], return_scores=True, **kw)) == 3
        assert sc["lnorm"] == float(len(seq)) and sc["n_pairs"] == len(seq) and 0.0 < sc["tm"] < 1.0
        assert np.isnan(sc["deviation"][:2]).all() and np.isnan(sc["deviation"][30:33]).all()
        rows_nat, lnorm = S.native_from_pdb(q, str(natives / "pf.pdb"))
        _check(sc, c, rows_nat, lnorm, "front end pf")
        assert P._ENGINES[0].get_option("score_native") == 0
        want = S.scores_json(sc)
        args = ["-i", paths[0], "-d", "cuda:0", "-n", "1", "-m", "0", "-w", weights_file]
        texts, errs = [], []
        for extra in ([], ["--native", str(natives / "pf.pdb")],
                      ["--native", str(natives / "pf.pdb"), "--native-chain", "A", "--scores", str(tmp_path / "pf.json")]):
            out, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                run_dmpfold(args + extra)
            texts.append(out.getvalue())
            errs.append(err.getvalue())
        assert texts[0].startswith("REMARK") and texts[0] == texts[1] == texts[2]
        assert json.loads(errs[1].strip().split("\n")[-1]) == want and "tm" not in errs[2]
        assert json.loads((tmp_path / "pf.json").read_text()) == want
        for fmt in ("npz", "pdb"):
            out_dir = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i"] + paths + ["-o", str(out_dir), "-n", "1", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--natives", str(natives)])
            assert rc == 0, buf.getvalue()
            summary = json.loads(buf.getvalue().strip().split("\n")[-1])
            assert summary["targets"] == 2 and summary["scored_targets"] == 1 and list(summary["scores"]) == ["pf"]
            assert summary["scores"]["pf"] == want
            assert summary["mean_tm"] == want["tm"] == summary["median_tm"] and summary["median_lddt"] == want["lddt"]
            if fmt == "pdb":
                assert (out_dir / "pf.pdb").read_text() == texts[0] and (out_dir / "s40.pdb").exists()
                assert json.loads((out_dir / "pf.scores.json").read_text()) == want
                assert not (out_dir / "s40.scores.json").exists()
            else:
                z = np.load(str(out_dir / "pf.npz"))
                assert np.array_equal(z["coords"], c.cpu().numpy()) and np.array_equal(z["confs"], f.cpu().numpy())
                assert float(z["tm"]) == sc["tm"] and int(z["n_pairs"]) == sc["n_pairs"] and list(z["counts"]) == sc["counts"]
                assert np.array_equal(z["deviation"], sc["deviation"], equal_nan=True) and np.array_equal(z["R"], sc["R"])
                z40 = np.load(str(out_dir / "s40.npz"))
                assert "tm" not in z40.files and "coords" in z40.files
    finally:
        P._ENGINES.clear()
