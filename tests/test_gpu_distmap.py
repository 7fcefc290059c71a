"""The chosen pass's predicted distance map on the GPU (option "emit_distmap"; include/dmpfold_hip.h).

What comes back is pinned to the reference - the golden head plane for pass 0, the CPU oracle's `p1.dm` where the
best-of rule keeps a middle pass (tests/test_distmap_cpu.py derives which) - and, where one CPU pass takes minutes, to
invariances: the map of a run is bit for bit the map of the shorter run that ends with the chosen pass, and that run's
Gram matrix ("gram" of dmp_debug_fetch, the last pass's) is the one the returned map gives.
"""
import contextlib
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_rows
from test_distmap_cpu import BEST_PASS

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: the checker)

GUARD = 4096                        # NaN elements behind every raw output buffer, as tests/abi.py makes them
PRECISIONS = [0, 1, 2]


def scale_tol(ref, rel):
    """The project's tolerance for a whole trunk pass (tests/test_gpu_parity.py)."""
    return rel * max(1.0, float(np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------ engines and oracle
@pytest.fixture(scope="module")
def eng(synth_sd):
    """One engine for every single-engine test (all their fixtures were captured with the seed-0 weights)."""
    from dmpfold2_amd.predict import Engine
    e = Engine("cuda:0", 300, 3000)
    e.set_weights({k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()})
    yield e
    e.close()


@contextlib.contextmanager
def _precision(eng, p):
    before = eng.get_option("precision")
    eng.set_option("precision", p)
    try:
        yield eng
    finally:
        eng.set_option("precision", before)
        eng.set_option("emit_distmap", 0)
        eng.set_option("recycle_tol_mA", 0)


_ORACLE = {}


def _oracle(key, aln, W, iterations, minsteps=0):
    """Oracle capture of a run, computed once and shared by the three precisions (never modified)."""
    if key not in _ORACLE:
        cap = {}
        coords, confs = O.predict(aln, W, None, iterations, minsteps, "canonical", cap)
        cap["coords"], cap["confs"] = coords, confs
        _ORACLE[key] = cap
    return _ORACLE[key]


def _inputs(name):
    """(fixture, None, alnmat, minsteps) of a fixture captured with the seed-0 weights (the `eng` fixture's)."""
    g = load_golden(name)
    if name.startswith("synth_L300"):                              # the alignment is regenerated, its digest is on record
        import hashlib
        from dmpfold2_amd import synth
        from dmpfold2_amd.predict import encode_aln
        alnmat = encode_aln(synth.synth_msa(300, 2000, int(g["msa_seed"])))
        assert hashlib.sha256(alnmat.tobytes()).hexdigest() == bytes(g["alnmat_sha256"]).decode()
        return g, None, np.ascontiguousarray(alnmat), int(g["minsteps"])
    return g, None, np.ascontiguousarray(g["alnmat"]), int(g["minsteps"])


def _one_row(L):
    from dmpfold2_amd import synth
    return np.ascontiguousarray(O.encode_aln(synth.synth_msa(L, 1, 1000 + L)))


def _raw_predict(eng, aln, iterations, minsteps, floats):
    """dmp_predict into NaN-poisoned buffers: `floats` elements for d_conf, a NaN guard tail behind both outputs.
    Returns (coords (L,5,3), the whole d_conf allocation guard included) after synchronising."""
    n, L = aln.shape
    d_msa = torch.from_numpy(np.ascontiguousarray(aln)).to(eng.device)
    coords = torch.full((15 * L + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    conf = torch.full((floats + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), n, L, None, 0, iterations, minsteps, coords.data_ptr(),
                             conf.data_ptr(), eng.stream())
    assert rc == 0, eng.lib.dmp_last_error()
    eng.sync_check()
    assert bool(torch.isnan(coords[15 * L:]).all()), "the guard behind d_coords was written"
    return coords[:15 * L].view(L, 5, 3), conf


def _map_rms(dm, ca):
    """float64 restatement of the header's definition from the returned map and the refined trace."""
    ca = np.asarray(ca, dtype=np.float64)
    d = ca[:, None, :] - ca[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    iu = np.triu_indices(len(ca), 1)
    e = np.asarray(dm, dtype=np.float64)[iu] - dist[iu]
    return float(np.sqrt((e * e).mean()))


def _gram_identity(eng, dm, L, tag):
    """"gram" of the run just made (its LAST pass) against M_ij = 0.5 ((dm_0j^2 + dm_i0^2) - dm_ij^2) formed in float64
    from `dm`.  gram_kernel rounds the two squares, their sum, the third square and the difference to float32 (fewer
    where the compiler fuses a multiply into the add); each rounding is at most 2^-24 of its result, the results are
    bounded by D^2, D^2, 2 D^2, D^2 and 2 D^2 with D = max dm, and the halving is exact: |error| <= 3.5 x 2^-24 x D^2.
    The bound asserted is 4 x 2^-24 x D^2."""
    gram = eng.fetch("gram", L * L).cpu().numpy().astype(np.float64).reshape(L, L)
    d = dm.cpu().numpy().astype(np.float64)
    want = 0.5 * ((d[0][None, :] ** 2 + d[:, 0][:, None] ** 2) - d ** 2)
    bound = 4.0 * 2.0 ** -24 * float(d.max()) ** 2
    err = float(np.abs(gram - want).max())
    print(tag, "gram identity: max error", err, "bound", bound, file=sys.stderr)
    assert err <= bound, (tag, err, bound)


# ------------------------------------------------------------------------------------------------ 1. pass 0, golden
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reference_pin_pass0(eng, precision):
    """PF10963 with iterations = 0: the map is |sym(head_p0[0])| of the reference's captured head plane."""
    g, _, aln, _ = _inputs("pf10963_n0_m0")
    h0 = g["head_p0"][0]
    ref = np.abs((h0 + h0.T) * np.float32(0.5))
    with _precision(eng, precision):
        coords, confs, dm, info = eng.predict(aln, None, 0, 0, distmap=True)
        eng.sync_check()
        assert eng.get_option("emit_distmap") == 0                 # set for the call only
    assert tuple(confs.shape) == (82,) and tuple(dm.shape) == (82, 82) and tuple(info.shape) == (3,)
    assert confs.untyped_storage().data_ptr() == dm.untyped_storage().data_ptr() == info.untyped_storage().data_ptr()
    err, tol = float(np.abs(dm.cpu().numpy() - ref).max()), scale_tol(ref, 1e-4)
    print("pf10963_n0_m0 precision", precision, "max |dm - reference|", err, "tol", tol, file=sys.stderr)
    assert err <= tol
    assert info[:2].tolist() == [0.0, 1.0]
    assert torch.equal(dm, dm.t())
    assert np.abs(confs.cpu().numpy() - g["confs"]).max() < 1e-4
    assert abs(float(info[2]) - _map_rms(dm.cpu().numpy(), coords.cpu().numpy()[:, 1])) <= 1e-6 * float(info[2])


# ------------------------------------------------------------------------------------------------ 2. a middle pass, oracle
# the reference's own spread of pass 1's dm, 8 threads against 1 (profiles/distmap.txt), in Angstrom
ORACLE_FLOOR = {"synth_L40_N64_n2_m0": 3.6e-4, "pf10963_n3_m0": 3.1e-4}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(ORACLE_FLOOR))
def test_chosen_pass_is_neither_first_nor_last(eng, oracle_weights, name, precision):
    """best 1 of 3 (L = 40) and 1 of 4 (PF10963): the map is the oracle's p1.dm within max(scale_tol(ref, 1e-4),
    4 x the reference's thread-count spread of that map); the maps of pass 0 and of the last pass are more than 100
    tolerances away, so a wrong pass cannot hide.  Measured deviations of the three precisions: profiles/distmap.txt."""
    g, _, aln, _ = _inputs(name)
    n = int(g["iterations"])
    passes, best, _ = BEST_PASS[name]
    assert passes == n + 1 and best == 1
    cap = _oracle(name, aln, oracle_weights, n)
    ref = cap["p1.dm"].numpy()
    tol = max(scale_tol(ref, 1e-4), 4.0 * ORACLE_FLOOR[name])
    for other in (0, n):
        gap = float(np.abs(ref - cap[f"p{other}.dm"].numpy()).max())
        assert gap > 100.0 * tol, (other, gap, tol)
    with _precision(eng, precision):
        coords, confs, dm, info = eng.predict(aln, None, n, 0, distmap=True)
        eng.sync_check()
        assert eng.fetch("best_pass", 1).tolist() == [1.0]
    err = float(np.abs(dm.cpu().numpy() - ref).max())
    print(name, "precision", precision, "max |dm - oracle p1.dm|", err, "tol", tol, file=sys.stderr)
    assert info[:2].tolist() == [1.0, float(n + 1)]
    assert err <= tol
    assert torch.equal(dm, dm.t())


# ------------------------------------------------------------------------------------------------ 3. headline width
@pytest.mark.parametrize("precision", PRECISIONS)
def test_headline_width_middle_pass(eng, precision):
    """L = 300, N = 2000, best pass 4 of 11: the -n 10 run's map is bit for bit the -n 4 run's, `info` agrees except
    passes_run, and the -n 4 run's Gram matrix is the one the map gives (bound: _gram_identity)."""
    name = "synth_L300_N2000_n10_m0"
    _, _, aln, _ = _inputs(name)
    assert BEST_PASS[name][:2] == (11, 4)
    with _precision(eng, precision):
        _, confs10, dm10, info10 = eng.predict(aln, None, 10, 0, distmap=True)
        eng.sync_check()
        _, confs4, dm4, info4 = eng.predict(aln, None, 4, 0, distmap=True)
        eng.sync_check()
        assert info10[:2].tolist() == [4.0, 11.0] and info4[:2].tolist() == [4.0, 5.0]
        assert torch.equal(dm10, dm4) and torch.equal(confs10, confs4)
        assert info10[2].item() == info4[2].item() and np.isfinite(info4[2].item())
        assert torch.equal(dm4, dm4.t())
        _gram_identity(eng, dm4, 300, f"{name} precision {precision}")


# ------------------------------------------------------------------------------------------------ 4. lengths
LENGTHS = [8, 31, 32, 33, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("L", LENGTHS)
def test_length_sweep(eng, oracle_weights, L, precision):
    """One-row alignments, -n 1 -m 0, around the tile edge of keep_best_dm (64) and the row dealing of emit_distmap:
    every element written, none beyond; symmetry; the Gram identity through a second run that ends with the chosen
    pass; map_rms against its float64 restatement; up to L = 65 the oracle's map of the chosen pass (the bound of
    test 2 without a floor term: scale_tol(ref, 1e-4)); and a run with -m 5, where the trace is the refined one."""
    from dmpfold2_amd.predict import distmap_floats, split_distmap_buffer
    aln = _one_row(L)
    n_out = distmap_floats(L)
    with _precision(eng, precision):
        eng.set_option("emit_distmap", 1)
        coords, buf = _raw_predict(eng, aln, 1, 0, n_out)
        assert bool(torch.isnan(buf[n_out:]).all()), "the guard behind L + L*L + 3 floats was written"
        assert not bool(torch.isnan(buf[:n_out]).any()), "an element of the extension was not written"
        confs, dm, info = split_distmap_buffer(buf[:n_out], L)
        best = int(info[0])
        assert info[0].item() in (0.0, 1.0) and info[1].item() == 2.0
        assert eng.fetch("best_pass", 1).tolist() == [float(best)]
        assert torch.equal(eng.fetch("best_dm", L * L).view(L, L), dm)
        assert torch.equal(dm, dm.t())
        ca = eng.fetch("best_ca_refined", 3 * L).cpu().numpy().reshape(L, 3)
        assert np.array_equal(ca, coords.cpu().numpy()[:, 1])
        want = _map_rms(dm.cpu().numpy(), ca)
        assert abs(float(info[2]) - want) <= 1e-6 * want, (float(info[2]), want)
        if L <= 65:
            cap = _oracle(("one_row", L), aln, oracle_weights, 1)
            means = [float(cap[f"p{p}.conf"].mean()) for p in (0, 1)]
            if abs(means[1] - means[0]) > 1e-3:                    # (the project's bound on a per-pass mean)
                assert best == int(means[1] > means[0]), (means, best)
            ref = cap[f"p{best}.dm"].numpy()
            err, tol = float(np.abs(dm.cpu().numpy() - ref).max()), scale_tol(ref, 1e-4)
            print("L", L, "precision", precision, "best", best, "max |dm - oracle|", err, "tol", tol, file=sys.stderr)
            assert err <= tol
        # the run that ends with the chosen pass: same map, and its Gram matrix is the last pass's
        _, buf_b = _raw_predict(eng, aln, best, 0, n_out)
        _, dm_b, info_b = split_distmap_buffer(buf_b[:n_out], L)
        assert info_b[:2].tolist() == [float(best), float(best + 1)]
        assert torch.equal(dm_b, dm) and info_b[2].item() == info[2].item()
        _gram_identity(eng, dm_b, L, f"L {L} precision {precision}")
        # with the minimiser on: map_rms is formed with the refined trace
        coords_m, buf_m = _raw_predict(eng, aln, 1, 5, n_out)
        assert bool(torch.isnan(buf_m[n_out:]).all()) and not bool(torch.isnan(buf_m[:n_out]).any())
        _, dm_m, info_m = split_distmap_buffer(buf_m[:n_out], L)
        ca_m = eng.fetch("best_ca_refined", 3 * L).cpu().numpy().reshape(L, 3)
        raw_m = eng.fetch("best_ca", 3 * L).cpu().numpy().reshape(L, 3)
        assert not np.array_equal(ca_m, raw_m)                     # the minimiser moved it
        want_m = _map_rms(dm_m.cpu().numpy(), ca_m)
        assert abs(float(info_m[2]) - want_m) <= 1e-6 * want_m, (float(info_m[2]), want_m)
        assert torch.equal(dm_m, dm_m.t())


# ------------------------------------------------------------------------------------------------ 5. buffers and the option
@pytest.mark.parametrize("precision", PRECISIONS)
def test_buffers_and_option(eng, precision):
    from dmpfold2_amd import _lib
    from dmpfold2_amd.predict import distmap_floats
    g, _, aln, _ = _inputs("pf10963_n3_m0")
    L = aln.shape[1]
    n_out = distmap_floats(L)
    with _precision(eng, precision):
        assert eng.get_option("emit_distmap") == 0                 # the default
        plain_c, plain_f = eng.predict(aln, None, 3, 0)
        eng.sync_check()
        plain_c, plain_f = plain_c.clone(), plain_f.clone()
        assert eng.fetch("best_dm", L * L).numel() == 0            # nothing is kept with the option off ...
        assert eng.fetch("best_pass", 1).tolist() == [1.0]         # ... but the pass taken is always on record
        # off: nothing beyond the L confidences is written
        c_off, buf_off = _raw_predict(eng, aln, 3, 0, n_out)
        assert bool(torch.isnan(buf_off[L:]).all())
        assert torch.equal(c_off, plain_c) and torch.equal(buf_off[:L], plain_f)
        # only 0 and 1 are values
        for bad in (2, -1):
            rc = eng.lib.dmp_ctx_set_option(eng.ctx, b"emit_distmap", bad)
            assert rc == -1 and b"emit_distmap" in eng.lib.dmp_last_error()          # DMP_ERR_ARG
            assert eng.get_option("emit_distmap") == 0
        with pytest.raises(_lib.DmpError):
            eng.set_option("emit_distmap", 2)
        # on: all L + L*L + 3 floats, the guard intact, coordinates and confidences unchanged
        eng.set_option("emit_distmap", 1)
        assert eng.get_option("emit_distmap") == 1                 # the read-back
        c_on, buf_on = _raw_predict(eng, aln, 3, 0, n_out)
        assert not bool(torch.isnan(buf_on[:n_out]).any()) and bool(torch.isnan(buf_on[n_out:]).all())
        assert torch.equal(c_on, plain_c) and torch.equal(buf_on[:L], plain_f)
        assert buf_on[L + L * L:n_out][:2].tolist() == [1.0, 4.0]
        assert torch.equal(eng.fetch("best_dm", L * L), buf_on[L:L + L * L])
        # an engine whose option was set by hand: the Python call allocates the long buffer (nothing is overrun), and what
        # it returns follows its keyword
        out = eng.predict(aln, None, 3, 0)
        eng.sync_check()
        assert len(out) == 2 and tuple(out[1].shape) == (L,)
        assert torch.equal(out[0], plain_c) and torch.equal(out[1], plain_f)
        assert out[1].untyped_storage().nbytes() >= 4 * n_out
        out = eng.predict(aln, None, 3, 0, distmap=True)
        eng.sync_check()
        assert len(out) == 4 and torch.equal(out[2].reshape(-1), buf_on[L:L + L * L])
        assert eng.get_option("emit_distmap") == 1                 # on before the call, on after it
        # off again: bit for bit the plain call
        eng.set_option("emit_distmap", 0)
        c_again, buf_again = _raw_predict(eng, aln, 3, 0, n_out)
        assert bool(torch.isnan(buf_again[L:]).all())
        assert torch.equal(c_again, plain_c) and torch.equal(buf_again[:L], plain_f)
        out = eng.predict_checked(aln, None, 3, 0, distmap=True)
        assert len(out) == 4 and torch.equal(out[0], plain_c) and torch.equal(out[1], plain_f)
        assert torch.equal(out[2].reshape(-1), buf_on[L:L + L * L]) and torch.equal(out[3], buf_on[L + L * L:n_out])
        assert eng.get_option("emit_distmap") == 0


# ------------------------------------------------------------------------------------------------ 6. convergence stop
@pytest.mark.parametrize("precision", PRECISIONS)
def test_with_convergence_stop(eng, precision):
    """A row of tests/test_recycle_converge_cpu.py's table: L = 300 at 200 mA stops after pass 8 of 10.  Map and info
    are bit for bit the plain run's at that depth; passes_run is the stop pass + 1."""
    from test_recycle_converge_cpu import CASES
    name, iterations, tol_mA, passes = CASES[0]
    assert (name, iterations, passes) == ("synth_L300_N2000_n10_m0", 10, 9)
    _, _, aln, minsteps = _inputs(name)
    with _precision(eng, precision):
        c_s, f_s, dm_s, info_s = eng.predict(aln, None, iterations, minsteps, converge=tol_mA * 1e-3, distmap=True)
        eng.sync_check()
        assert eng.passes_run == passes and info_s[1].item() == float(passes)
        assert eng.get_option("recycle_tol_mA") == 0 and eng.get_option("emit_distmap") == 0
        c_p, f_p, dm_p, info_p = eng.predict(aln, None, passes - 1, minsteps, distmap=True)
        eng.sync_check()
        assert torch.equal(dm_s, dm_p) and torch.equal(info_s, info_p)
        assert torch.equal(c_s, c_p) and torch.equal(f_s, f_p)
        assert info_s[0].item() == 4.0


# ------------------------------------------------------------------------------------------------ 7. pipeline
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("streams", [2, 4])
def test_pipeline(synth_sd, streams, precision):
    """PF10963, L = 40 and L = 24, each twice, on 2 and on 4 engines: every ticket's confs, distmap and info are bit for
    bit the lone engine's ("tridiag_cluster" 0, as the scheduler's engines); with the option off `result` has its old
    shape."""
    from dmpfold2_amd.predict import Engine, Pipeline
    names = ["pf10963_n3_m0", "synth_L40_N64_n2_m0", "synth_L24_N3050_n1_m0"] * 2
    alns = {n: np.ascontiguousarray(load_golden(n)["alnmat"]) for n in set(names)}
    msas = [alns[n] for n in names]
    max_L, max_N = max(m.shape[1] for m in msas), max(m.shape[0] for m in msas)
    dev = torch.device("cuda:0")
    sdt = {k: torch.from_numpy(np.array(v)) for k, v in synth_sd.items()}
    single = Engine(dev, max_L, max_N)
    single.set_weights(sdt)
    single.set_option("precision", precision)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, max_L, max_N, sdt, streams=streams, precision=precision)
    try:
        refs = {}
        for n in set(names):
            out = single.predict(alns[n], None, 3, 0, distmap=True)
            single.sync_check()
            refs[n] = [x.clone() for x in out]
        assert all(e.get_option("emit_distmap") == 0 for e in pipe.engines)
        t = pipe.submit(torch.from_numpy(msas[0]).to(dev), 3, 0)
        pipe.drain()
        pipe.sync_check()
        old = pipe.result(t)
        assert len(old) == 2 and tuple(old[1].shape) == (msas[0].shape[1],)
        assert torch.equal(old[0], refs[names[0]][0]) and torch.equal(old[1], refs[names[0]][1])
        pipe.set_distmap(True)
        assert all(e.get_option("emit_distmap") == 1 for e in pipe.engines)          # reaches every engine
        tickets = pipe.submit_many([torch.from_numpy(m).to(dev) for m in msas], 3, 0)
        res = pipe.collect(tickets)
        for t, n in zip(tickets, names):
            assert not isinstance(res[t], Exception), res[t]
            coords, confs, dm, info = res[t]
            L = alns[n].shape[1]
            assert tuple(confs.shape) == (L,) and tuple(dm.shape) == (L, L) and tuple(info.shape) == (3,)
            for got, ref, what in zip((coords, confs, dm, info), refs[n], ("coords", "confs", "distmap", "info")):
                assert torch.equal(got, ref), (n, what)
            assert info[1].item() == 4.0                           # the ticket's own pass count
        assert refs["pf10963_n3_m0"][3][0].item() == 1.0
        pipe.set_distmap(False)
        assert all(e.get_option("emit_distmap") == 0 for e in pipe.engines)
        out = pipe.run([torch.from_numpy(msas[1]).to(dev)], 3, 0)
        pipe.sync_check()
        assert len(out[0]) == 2 and torch.equal(out[0][1], refs[names[1]][1])
        # the option by its name, not through set_distmap: the buffer follows what the engines hold
        pipe.set_option("emit_distmap", 1)
        t = pipe.submit(torch.from_numpy(msas[1]).to(dev), 3, 0)
        pipe.drain()
        pipe.sync_check()
        res = pipe.result(t)
        assert len(res) == 4
        for got, ref, what in zip(res, refs[names[1]], ("coords", "confs", "distmap", "info")):
            assert torch.equal(got, ref), what
        # and the C entry point itself into a poisoned buffer: L + L*L + 3 floats written, the guard behind them intact
        from dmpfold2_amd import _lib
        from dmpfold2_amd.predict import distmap_floats
        n, L = msas[1].shape
        n_out = distmap_floats(L)
        d_msa = torch.from_numpy(msas[1]).to(dev)
        coords = torch.full((15 * L + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        buf = torch.full((n_out + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        t = _lib.check(pipe.lib.dmp_pipeline_submit(pipe._p, d_msa.data_ptr(), n, L, None, 3, 0, coords.data_ptr(),
                                                    buf.data_ptr(), None))
        _lib.check(pipe.lib.dmp_pipeline_wait(pipe._p, 2))
        pipe.sync_check()
        pipe.lib.dmp_pipeline_release(pipe._p, t)
        assert not bool(torch.isnan(buf[:n_out]).any()) and bool(torch.isnan(buf[n_out:]).all())
        assert bool(torch.isnan(coords[15 * L:]).all())
        assert torch.equal(buf[L:L + L * L].view(L, L), refs[names[1]][2]) and torch.equal(buf[:L], refs[names[1]][1])
        # one engine alone: the buffer is sized for the engine that writes most, the extension is not handed out
        pipe.set_option("emit_distmap", 0)
        pipe.engines[-1].set_option("emit_distmap", 1)
        t = pipe.submit(torch.from_numpy(msas[1]).to(dev), 3, 0)
        pipe.drain()
        pipe.sync_check()
        res = pipe.result(t)
        assert len(res) == 2 and tuple(res[1].shape) == (L,) and torch.equal(res[1], refs[names[1]][1])
        assert res[1].untyped_storage().nbytes() >= 4 * n_out
        pipe.engines[-1].set_option("emit_distmap", 0)
    finally:
        pipe.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 8. front ends
@pytest.mark.parametrize("precision", PRECISIONS)
def test_front_ends(tmp_path, weights_file, monkeypatch, precision):
    """aln_to_coords(return_distmap=True) with and without the alignment matrix; `dmpfold --distmap FILE`: stdout byte
    for byte the run's without it, the file the API's map; `dmpfold-batch --distmap` in npz and pdb formats: the
    single-target route's arrays and bytes."""
    import dmpfold2_amd.predict as P
    from dmpfold2_amd import aln_to_coords, run_dmpfold
    from dmpfold2_amd import batch
    monkeypatch.setenv("DMPFOLD_PRECISION", str(precision))
    P._ENGINES.clear()
    try:
        paths = []
        for name, stem in (("pf10963_n3_m0", "pf"), ("synth_L40_N64_n2_m0", "s40")):
            p = tmp_path / f"{stem}.aln"
            p.write_text("\n".join(golden_rows(load_golden(name))) + "\n")
            paths.append(str(p))
        kw = dict(device="cuda:0", iterations=3, minsteps=0, weights_file=weights_file)
        plain = aln_to_coords(paths[0], **kw)
        assert len(plain) == 2
        c, f, dm = aln_to_coords(paths[0], return_distmap=True, **kw)
        assert tuple(dm.shape) == (82, 82) and torch.equal(c, plain[0]) and torch.equal(f, plain[1])
        c2, f2, alnmat, dm2 = aln_to_coords(paths[0], return_alnmat=True, return_distmap=True, **kw)
        assert alnmat.dtype == np.uint8 and alnmat.shape[1] == 82 and torch.equal(dm2, dm) and torch.equal(c2, c)
        assert len(aln_to_coords(paths[0], return_alnmat=True, **kw)) == 3
        assert P._ENGINES[0].get_option("emit_distmap") == 0 and P._ENGINES[0].get_option("precision") == precision
        single = {}
        for a in paths:
            stem = os.path.splitext(os.path.basename(a))[0]
            texts = []
            for extra in ([], ["--distmap", str(tmp_path / f"{stem}.single.npy")]):
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    run_dmpfold(["-i", a, "-d", "cuda:0", "-n", "3", "-m", "0", "-w", weights_file] + extra)
                texts.append(buf.getvalue())
            assert texts[0].startswith("REMARK") and texts[0] == texts[1]
            single[stem] = texts[0]
        assert np.array_equal(np.load(str(tmp_path / "pf.single.npy")), dm.cpu().numpy())
        for fmt in ("npz", "pdb"):
            out = tmp_path / f"out_{fmt}"
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rc = batch.main(["-i"] + paths + ["-o", str(out), "-n", "3", "-m", "0", "-w", weights_file, "--format", fmt,
                                 "--streams", "2", "--distmap"])
            assert rc == 0, buf.getvalue()
            for stem in single:
                want = (tmp_path / f"{stem}.single.npy").read_bytes()
                if fmt == "pdb":
                    assert (out / f"{stem}.pdb").read_text() == single[stem]
                    assert (out / f"{stem}.distmap.npy").read_bytes() == want
                else:
                    z = np.load(str(out / f"{stem}.npz"))
                    assert np.array_equal(z["distmap"], np.load(str(tmp_path / f"{stem}.single.npy")))
                    assert int(z["best_pass"]) == 1 and int(z["passes_run"]) == 4 and np.isfinite(z["map_rms"])
        z = np.load(str(tmp_path / "out_npz" / "pf.npz"))
        assert np.array_equal(z["coords"], c.cpu().numpy()) and np.array_equal(z["confs"], f.cpu().numpy())
    finally:
        P._ENGINES.clear()


# ------------------------------------------------------------------------------------------------ 9. software-latched fault
@pytest.mark.parametrize("precision", PRECISIONS)
def test_latched_fault_gives_nan_in_the_whole_extension(eng, precision):
    """A residue code of 22 raises the device-side flag DMP_FAULT_BAD_CODE (a software flag, not a GPU fault): the
    coordinates, the confidences, the map and the three tail floats all come back NaN, and the guard stays."""
    from dmpfold2_amd.predict import FAULT_BAD_CODE, distmap_floats
    aln = _one_row(33).copy()
    aln[0, 5] = 22
    n_out = distmap_floats(33)
    with _precision(eng, precision):
        eng.set_option("emit_distmap", 1)
        d_msa = torch.from_numpy(aln).to(eng.device)
        coords = torch.zeros((33, 5, 3), dtype=torch.float32, device=eng.device)
        buf = torch.zeros((n_out + GUARD,), dtype=torch.float32, device=eng.device)
        buf[n_out:] = 7.0                                          # a guard that NaN would spoil
        rc = eng.lib.dmp_predict(eng.ctx, d_msa.data_ptr(), 1, 33, None, 0, 1, 0, coords.data_ptr(), buf.data_ptr(),
                                 eng.stream())
        assert rc == 0
        assert eng.sync_faults() == FAULT_BAD_CODE
        assert bool(torch.isnan(coords).all()) and bool(torch.isnan(buf[:n_out]).all())
        assert bool((buf[n_out:] == 7.0).all()), "the NaN fill went past L + L*L + 3 floats"
        # the next prediction on the engine is whole again
        good = _one_row(33)
        _, buf2 = _raw_predict(eng, good, 1, 0, n_out)
        assert not bool(torch.isnan(buf2[:n_out]).any()) and bool(torch.isnan(buf2[n_out:]).all())
