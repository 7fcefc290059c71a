"""Convergence stop of the recycling loop on the GPU (option "recycle_tol_mA"; include/dmpfold_hip.h).

The expected stop pass of every (fixture, tolerance) pair comes from the reference's own per-pass traces
(tests/test_recycle_converge_cpu.py derives it and asserts its margins); here the engine is held to it, and to the
defining property: a run that stopped after pass k is bit for bit the plain run with iterations = k.
"""
import contextlib
import io
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import load_golden, ca_rmsd
from test_recycle_converge_cpu import CASES, recycle_deltas

pytestmark = pytest.mark.gpu

import dmpfold_oracle as O          # noqa: E402  (test infrastructure: the checker)


def _inputs(name):
    """(fixture, state_dict, alnmat, minsteps) of a fixture, built as the tests that pin it against the reference do."""
    import hashlib
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import encode_aln
    g = load_golden(name)
    if name.startswith("pf10963"):
        return g, synth.synth_weights(0, coord_scale=5.0), g["alnmat"], 0
    if name.startswith("actsmall"):
        sd = synth.synth_weights(int(g["weights_seed"]), coord_scale=float(g["coord_scale"]), act_scale=float(g["act_scale"]))
        assert synth.weights_checksum(sd) == bytes(g["weights_sha256"]).decode()
        return g, sd, g["alnmat"], 0
    if name.startswith("synth_L300"):
        sd, L, rows = synth.synth_weights(0, coord_scale=5.0), 300, 2000
    else:
        sd = synth.headline_fixture_weights(g["coord_fc"], float(g["coord_gru_mds_scale"]), seed=int(g["weights_seed"]))
        assert synth.weights_checksum(sd) == bytes(g["weights_sha256"]).decode()
        L, rows = 500, int(g["msa_rows"])
    alnmat = encode_aln(synth.synth_msa(L, rows, int(g["msa_seed"])))
    assert hashlib.sha256(alnmat.tobytes()).hexdigest() == bytes(g["alnmat_sha256"]).decode()
    return g, sd, alnmat, int(g["minsteps"])


def _engine(sd, alnmat, precision):
    from dmpfold2_amd.predict import Engine
    eng = Engine("cuda:0", alnmat.shape[1], alnmat.shape[0])
    eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    eng.set_option("precision", precision)
    return eng


def _record(eng, L):
    """Everything a prediction leaves behind that a second run can be compared with, on the host."""
    P = eng.passes_run
    return {"passes": P,
            "ca_pass": eng.fetch("ca_pass", P * L * 3).cpu().numpy().reshape(P, L, 3),
            "conf_means": eng.fetch("conf_means", P).cpu().numpy(),
            "best_ca": eng.fetch("best_ca", L * 3).cpu().numpy(),
            "best_ca_refined": eng.fetch("best_ca_refined", L * 3).cpu().numpy()}


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("name,iterations,tol_mA,passes", CASES)
def test_stop_pass_and_bit_identity(name, iterations, tol_mA, passes, precision):
    """Every row of the issue's table, in the three arithmetic settings: the run stops where the reference's traces say
    it must, the recorded d_p are the rule's (float64 restatement on the run's OWN traces: 1e-5 relative) and the
    reference's (within 4 x the per-pass CA bound of test_gpu_headline._check_passes: max(1e-3, 4 x the fixture's floor)),
    and outputs and per-pass records equal those of the plain run with iterations = passes - 1, bit for bit.  For the two
    full-size fixtures the reference's best pass precedes the stop, so the stopped run is also held to the reference's
    final structure at exactly the bounds of the tests that pin those fixtures at full depth."""
    g, sd, alnmat, minsteps = _inputs(name)
    L = alnmat.shape[1]
    eng = _engine(sd, alnmat, precision)
    try:
        assert eng.get_option("recycle_tol_mA") == 0
        eng.set_option("recycle_tol_mA", tol_mA)
        coords, confs = eng.predict(alnmat, None, iterations, minsteps)
        eng.sync_check()
        got = _record(eng, L)
        delta = eng.fetch("pass_delta", got["passes"]).cpu().numpy()
        print(name, "precision", precision, "passes", got["passes"], "pass_delta", np.array2string(delta, precision=5), file=sys.stderr)
        assert got["passes"] == passes
        assert delta.shape == (passes,) and np.isinf(delta[0]) and delta[0] > 0
        # the rule, restated in float64 on the traces this run recorded (pass 0 is recorded after its refinement)
        own = recycle_deltas(got["ca_pass"])
        assert (np.abs(delta[1:] - own[1:]) <= 1e-5 * own[1:]).all(), (delta, own)
        tol = np.float32(tol_mA) * np.float32(1e-3)
        stopped = passes < iterations + 1
        assert (delta[1:-1] > tol).all() and (delta[-1] <= tol) == stopped
        # the reference's values; a fixture made with the minimiser on records pass 0 BEFORE its refinement
        seed0 = None
        if minsteps > 0:
            seed0 = O.refine_coords(torch.from_numpy(np.array(g["ca_pass"][0])), minsteps).numpy()
        P = min(passes, len(g["ca_pass"]))
        ref = recycle_deltas(g["ca_pass"][:P], seed0)
        floor = np.asarray(g["noise_ca_pass"], dtype=np.float64)[:P]
        bound = 4.0 * np.maximum(1e-3, 4.0 * floor)
        print(name, "|d - reference d|", np.array2string(np.abs(delta[1:P] - ref[1:]), precision=2), "bound",
              np.array2string(bound[1:], precision=2), file=sys.stderr)
        assert (np.abs(delta[1:P] - ref[1:]) <= bound[1:]).all()
        if name.startswith("synth_L300"):
            final, dconf = ca_rmsd(coords.cpu().numpy()[:, 1], g["coords"][:, 1]), float(np.abs(confs.cpu().numpy() - g["confs"]).max())
            print(name, "final", final, "max|dconf|", dconf, file=sys.stderr)
            assert final <= 1e-3
            assert dconf < max(1e-4, 3.0 * float(g["noise_conf"]))
        if name.startswith("fit_L500"):
            final, dconf = ca_rmsd(coords.cpu().numpy()[:, 1], g["coords"][:, 1]), float(np.abs(confs.cpu().numpy() - g["confs"]).max())
            print(name, "final", final, "max|dconf|", dconf, file=sys.stderr)
            assert final <= max(1e-3, 3.0 * float(g["noise_ca_rmsd"]))
            assert dconf < max(1e-4, 3.0 * float(g["noise_conf"]))
        # the plain run of that depth
        eng.set_option("recycle_tol_mA", 0)
        ref_c, ref_f = eng.predict(alnmat, None, passes - 1, minsteps)
        eng.sync_check()
        plain = _record(eng, L)
        assert plain["passes"] == passes
        assert eng.fetch("pass_delta", passes).numel() == 0            # nothing is recorded with the option off
        assert torch.equal(coords, ref_c) and torch.equal(confs, ref_f)
        for k in ("ca_pass", "conf_means", "best_ca", "best_ca_refined"):
            assert np.array_equal(got[k], plain[k]), k
    finally:
        eng.close()


def test_option_hygiene():
    """Default 0; negative -> DMP_ERR_ARG (the value stays); "passes_run" cannot be set; the per-call `converge` of the
    Python layer leaves the option as it was; after a converged run, option 0 gives the fixed-depth run bit for bit."""
    from dmpfold2_amd import _lib
    g, sd, alnmat, _ = _inputs("actsmall_L128_N500_n3_m0")
    eng = _engine(sd, alnmat, 0)
    try:
        assert eng.get_option("recycle_tol_mA") == 0
        first_c, first_f = eng.predict(alnmat, None, 10, 0)
        eng.sync_check()
        assert eng.passes_run == 11
        eng.set_option("recycle_tol_mA", 7)
        assert eng.get_option("recycle_tol_mA") == 7
        rc = eng.lib.dmp_ctx_set_option(eng.ctx, b"recycle_tol_mA", -1)
        assert rc == -1 and b"recycle_tol_mA" in eng.lib.dmp_last_error()          # DMP_ERR_ARG
        assert eng.get_option("recycle_tol_mA") == 7
        with pytest.raises(_lib.DmpError):
            eng.set_option("passes_run", 3)
        eng.set_option("recycle_tol_mA", 0)
        with pytest.raises(ValueError):
            eng.predict(alnmat, None, 10, 0, converge=-0.5)
        coords, confs = eng.predict_checked(alnmat, None, 10, 0, converge=0.01)
        assert eng.passes_run == 3 and eng.get_option("recycle_tol_mA") == 0
        again_c, again_f = eng.predict(alnmat, None, 10, 0)
        eng.sync_check()
        assert eng.passes_run == 11
        assert torch.equal(again_c, first_c) and torch.equal(again_f, first_f)
    finally:
        eng.close()
    # a tolerance nothing meets: every pass runs, with the extra kernel in every tail, and the bits are the plain run's
    g2, sd2, _, _ = _inputs("pf10963_n10_m0")
    eng = _engine(sd2, g2["alnmat"], 0)
    try:
        plain_c, plain_f = eng.predict(g2["alnmat"], None, 10, 0)
        eng.sync_check()
        on_c, on_f = eng.predict(g2["alnmat"], None, 10, 0, converge=0.001)
        eng.sync_check()
        assert eng.passes_run == 11
        assert torch.equal(on_c, plain_c) and torch.equal(on_f, plain_f)
        # iterations = 0 and 1 have no boundary to decide at
        for n in (0, 1):
            eng.predict(g2["alnmat"], None, n, 0, converge=100.0)
            eng.sync_check()
            assert eng.passes_run == n + 1
        # the tolerance of a run that is met at once: pass 1 is the last
        eng.predict(g2["alnmat"], None, 10, 0, converge=100.0)
        eng.sync_check()
        assert eng.passes_run == 2
    finally:
        eng.close()


def test_unit_interface_waits_at_the_pass_boundary():
    """The unit calls: at the boundary in front of every pass >= 2 dmp_predict_next_unit answers DMP_UNIT_WAIT until the
    pass tail has completed (it never blocks), then DMP_UNIT_NONE or the next unit; the result is dmp_predict's."""
    import time
    g, sd, alnmat, _ = _inputs("actsmall_L128_N500_n3_m0")
    eng = _engine(sd, alnmat, 0)
    try:
        ref_c, ref_f = eng.predict(alnmat, None, 10, 0, converge=0.01)
        eng.sync_check()
        assert eng.passes_run == 3
        lib, ctx, s = eng.lib, eng.ctx, eng.stream()
        N, L = alnmat.shape
        d_msa = torch.from_numpy(np.ascontiguousarray(alnmat)).to(eng.device)
        coords = torch.empty((L, 5, 3), dtype=torch.float32, device=eng.device)
        confs = torch.empty((L,), dtype=torch.float32, device=eng.device)
        eng.set_option("recycle_tol_mA", 10)
        assert lib.dmp_predict_begin_units(ctx, d_msa.data_ptr(), N, L, None, 0, 10, 0) == 0
        kinds, waits, deadline = [], 0, time.time() + 60.0
        while True:
            assert time.time() < deadline
            kind = lib.dmp_predict_next_unit(ctx)
            if kind == 0:
                break
            if kind == 3:
                waits += 1
                time.sleep(2e-4)
                continue
            kinds.append(kind)
            assert lib.dmp_predict_issue_unit(ctx, s) == 0
        assert lib.dmp_predict_end(ctx, coords.data_ptr(), confs.data_ptr(), s) == 0
        eng.sync_check()
        assert eng.passes_run == 3 and kinds.count(2) == 3 * 16
        print("unit interface: DMP_UNIT_WAIT answers at the two boundaries:", waits, file=sys.stderr)
        assert torch.equal(coords, ref_c) and torch.equal(confs, ref_f)
    finally:
        eng.close()


# (weights and tolerance of the batch, its targets, trunk passes the issue's table gives for each - None: not in the table)
BATCHES = {
    # the batch the issue names.  A pipeline holds ONE weight set and one tolerance, and the two fixtures were captured
    # with different weights: on the actsmall fixture's the table covers the actsmall targets only; what the PF10963
    # alignment does on those weights is taken from the single-engine route (it converges as well: the weights decide)
    "actsmall_weights_10mA": ("actsmall_L128_N500_n3_m0", 10, ["pf10963_n10_m0", "actsmall_L128_N500_n3_m0", "pf10963_n10_m0",
                                                              "pf10963_n10_m0", "actsmall_L128_N500_n3_m0", "pf10963_n10_m0"],
                              [None, 3, None, None, 3, None]),
    # a batch the table covers in full: the L = 300 fixture and PF10963 were captured with the SAME weights and are
    # listed at the same tolerance, one stopping after pass 8 and one never - predictions that end early beside ones
    # that run to their planned depth
    "seed0_weights_200mA": ("synth_L300_N2000_n10_m0", 200, ["pf10963_n10_m0", "synth_L300_N2000_n10_m0", "pf10963_n10_m0",
                                                            "pf10963_n10_m0", "synth_L300_N2000_n10_m0", "pf10963_n10_m0"],
                            [11, 9, 11, 11, 9, 11]),
}


@pytest.mark.parametrize("batch", list(BATCHES))
def test_pipeline_mixed_batch(batch):
    """Six targets, all with iterations = 10, through one pipeline of four engines.  Every result equals the single
    engine's ("tridiag_cluster" 0, as the scheduler's engines) bit for bit, each target runs the passes the table gives
    for it, the counters [8]-[10] are the sums over the batch, and the pipeline drains."""
    from dmpfold2_amd import _lib
    from dmpfold2_amd.predict import Engine, Pipeline
    wname, tol_mA, names, table = BATCHES[batch]
    _, sd, _, _ = _inputs(wname)
    alns = {n: _inputs(n)[2] for n in set(names)}
    msas = [alns[n] for n in names]
    max_L, max_N = max(m.shape[1] for m in msas), max(m.shape[0] for m in msas)
    dev = torch.device("cuda:0")
    sdt = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    single = Engine(dev, max_L, max_N)
    single.set_weights(sdt)
    single.set_option("precision", 0)
    single.set_option("tridiag_cluster", 0)
    pipe = Pipeline(dev, max_L, max_N, sdt, streams=4, precision=0)
    try:
        assert all(e.get_option("recycle_tol_mA") == 0 for e in pipe.engines)
        with pytest.raises(_lib.DmpError):
            pipe.set_option("recycle_tol_mA", -5)
        pipe.set_converge(tol_mA * 1e-3)
        assert all(e.get_option("recycle_tol_mA") == tol_mA for e in pipe.engines)      # reaches every engine
        refs, passes = [], []
        for m in msas:
            c, f = single.predict(m, None, 10, 0, converge=tol_mA * 1e-3)
            single.sync_check()
            refs.append((c.clone(), f.clone()))
            passes.append(single.passes_run)
        print(batch, "single-engine passes", passes, file=sys.stderr)
        assert all(t is None or t == p for t, p in zip(table, passes)), (table, passes)
        tickets = pipe.submit_many([torch.from_numpy(m).to(dev) for m in msas], 10, 0)
        waiter = threading.Thread(target=lambda: _lib.check(pipe.lib.dmp_pipeline_wait(pipe._p, 2)), daemon=True)
        waiter.start()
        waiter.join(timeout=120.0)
        assert not waiter.is_alive(), "the pipeline did not drain"
        pipe.sync_check()
        stats = pipe.stats()
        print(batch, "pipeline stats", stats, file=sys.stderr)
        assert stats["passes_run"] == sum(passes)
        assert stats["early_stops"] == sum(p < 11 for p in passes) and stats["passes_saved"] == sum(11 - p for p in passes)
        if None not in table:
            assert (stats["passes_run"], stats["early_stops"], stats["passes_saved"]) == (2 * 9 + 4 * 11, 2, 2 * 2)
        assert stats["riders_left"] == 0 and not pipe.busy()
        for t, (ref_c, ref_f), m in zip(tickets, refs, msas):
            coords, confs = pipe.result(t)
            assert torch.equal(coords, ref_c) and torch.equal(confs, ref_f), m.shape
        # a caller built for the eight counters this ABI first had keeps working
        import ctypes as C
        v = (C.c_longlong * 9)(*([-7] * 9))
        _lib.check(pipe.lib.dmp_pipeline_stats(pipe._p, v, 8))
        assert v[8] == -7
        # option off again on the idle pipeline: fixed depth
        pipe.set_converge(None)
        assert all(e.get_option("recycle_tol_mA") == 0 for e in pipe.engines)
        t = pipe.submit(torch.from_numpy(msas[1]).to(dev), 3, 0)
        pipe.drain()
        pipe.sync_check()
        c3, f3 = single.predict(msas[1], None, 3, 0)
        single.sync_check()
        coords, confs = pipe.result(t)
        assert torch.equal(coords, c3) and torch.equal(confs, f3)
        assert pipe.stats()["passes_run"] == sum(passes) + 4 and pipe.stats()["early_stops"] == stats["early_stops"]
    finally:
        pipe.close()
        single.close()


def test_cli_flag_that_never_triggers_changes_no_byte(tmp_path, weights_file):
    """-c 0.2 on the reference's example alignment (min d_p = 4.0 A): the PDB text is the run's without the flag."""
    from dmpfold2_amd import run_dmpfold
    g = load_golden("pf10963_n10_m0")
    aln = tmp_path / "PF10963.aln"
    aln.write_text(bytes(g["aln_text"]).decode("latin-1"))
    texts = []
    for extra in ([], ["-c", "0.2"]):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            run_dmpfold(["-i", str(aln), "-d", "cuda:0", "-n", "10", "-m", "0", "-w", weights_file] + extra)
        texts.append(buf.getvalue())
    assert texts[0].startswith("REMARK") and texts[0].count("ATOM") > 82 * 4
    assert texts[0] == texts[1]
