"""Convergence stop of the recycling loop (option "recycle_tol_mA", `converge=` / -c / --converge): what can be checked
without a GPU.

The stop rule is defined on the traces `ca_pass` records, and the reference-captured fixtures carry the reference's own
`ca_pass`: the pass after which a run with a given tolerance must stop follows from a fixture alone.  `recycle_deltas`
below is the float64 restatement of the rule (include/dmpfold_hip.h, option "recycle_tol_mA");
tests/test_gpu_recycle_converge.py imports it and holds the engine to the stop passes derived here.  Each (fixture,
tolerance) pair is only a fair expectation for another arithmetic if the decision is not a close call, so the margins
are asserted too.
"""
import numpy as np
import pytest

from conftest import load_golden

# (fixture, iterations the run is given, tolerance in mA, trunk passes expected); None = never stops early
CASES = [
    ("synth_L300_N2000_n10_m0", 10, 200, 9),
    ("fit_L500_N5000_n30_m200", 30, 180, 12),
    ("actsmall_L128_N500_n3_m0", 10, 10, 3),
    ("pf10963_n10_m0", 10, 200, 11),
]
FINAL_OUTPUT_CASES = ("synth_L300_N2000_n10_m0", "fit_L500_N5000_n30_m200")


def clamped_distances(x):
    """D(x)_ij = sqrt(max(|x_i - x_j|^2, 1e-8)) in float64 (network.py:272 on a float64 copy of the trace)."""
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    return np.sqrt(np.maximum((d * d).sum(-1), 1e-8))


def recycle_delta(ca, seed):
    """d = sqrt(mean over i < j of (D(ca)_ij - D(seed)_ij)^2), Angstrom."""
    iu = np.triu_indices(len(ca), 1)
    e = clamped_distances(ca)[iu] - clamped_distances(seed)[iu]
    return float(np.sqrt((e * e).mean()))


def recycle_deltas(ca_pass, seed0=None):
    """[+inf, d_1, d_2 ...] of a run's recorded traces; `seed0`: the trace that seeded pass 1 where that is not
    ca_pass[0] (a reference fixture made with the minimiser on records pass 0 BEFORE its refinement)."""
    out = [np.inf]
    for p in range(1, len(ca_pass)):
        out.append(recycle_delta(ca_pass[p], seed0 if (p == 1 and seed0 is not None) else ca_pass[p - 1]))
    return np.array(out)


def stop_pass(deltas, tol, iterations):
    """The last pass of a run of `iterations` with tolerance `tol` (A): the first p >= 1 with float32(d_p) <= tol."""
    for p in range(1, min(iterations, len(deltas) - 1) + 1):
        if np.float32(deltas[p]) <= np.float32(tol):
            return p
    return iterations


@pytest.mark.parametrize("name,iterations,tol_mA,passes", CASES)
def test_expected_stop_pass_follows_from_the_fixture(name, iterations, tol_mA, passes):
    g = load_golden(name)
    d = recycle_deltas(g["ca_pass"])
    tol = tol_mA * 1e-3
    print(name, "d_p", np.array2string(d, precision=4))
    last = stop_pass(d, tol, iterations)
    assert last + 1 == passes
    known = d[1:min(iterations, len(d) - 1) + 1]
    # no earlier pass is within the tolerance, and no recorded value - the neighbours of the tolerance least of all - is
    # a close call: d_p and the tolerance differ by a factor of at least 1.2 either way (a perturbation of the trace
    # changes d_p in proportion, so the margin is a ratio)
    assert (known[:last - 1] > tol).all()
    assert (np.maximum(known / tol, tol / known) >= 1.2).all(), (known, tol)
    if passes == iterations + 1:
        assert len(d) == iterations + 1 and known.min() > tol          # never: the whole run is on record
    else:
        assert known[last - 1] <= tol
    if name in FINAL_OUTPUT_CASES:
        # the reference's best pass precedes the stop with a clear margin: its full-depth answer is the stopped run's too
        means = np.asarray(g["conf_mean_pass"], dtype=np.float64)
        best = int(np.argmax(means))
        assert best <= last
        assert means[best] - np.delete(means, best).max() > 1e-3


def test_issue_table_values():
    """The neighbours of each tolerance as the issue lists them (three significant digits)."""
    d = recycle_deltas(load_golden("synth_L300_N2000_n10_m0")["ca_pass"])
    assert abs(d[7] - 0.328) < 1e-3 and abs(d[8] - 0.131) < 1e-3
    d = recycle_deltas(load_golden("fit_L500_N5000_n30_m200")["ca_pass"])
    assert abs(d[10] - 0.231) < 1e-3 and abs(d[11] - 0.145) < 1e-3
    d = recycle_deltas(load_golden("actsmall_L128_N500_n3_m0")["ca_pass"])
    assert abs(d[1] - 0.0197) < 1e-4 and abs(d[2] - 0.0072) < 1e-4
    d = recycle_deltas(load_golden("pf10963_n10_m0")["ca_pass"])
    assert abs(d[1:].min() - 4.0) < 0.05


def test_restatement_properties():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(40, 3)) * 10.0
    assert recycle_delta(x, x) == 0.0
    # rigid motions do not count: the rule looks at distance maps
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    assert recycle_delta(x @ q + 5.0, x) < 1e-12
    # a uniform 1 % expansion moves every distance by 1 %
    D = clamped_distances(x)[np.triu_indices(40, 1)]
    assert abs(recycle_delta(1.01 * x, x) - 0.01 * np.sqrt((D * D).mean())) < 1e-9
    d = recycle_deltas(np.stack([x, x + 1e-3 * rng.normal(size=x.shape), x]))
    assert np.isinf(d[0]) and d[1] > 0 and stop_pass(d, 0.01, 2) == 1 and stop_pass(d, 1e-9, 2) == 2
    assert stop_pass(np.array([np.inf, np.nan, 0.0]), 0.01, 2) == 2        # NaN never stops


def test_tolerance_conversion():
    from dmpfold2_amd.predict import converge_to_mA
    assert converge_to_mA(None) == 0 and converge_to_mA(0) == 0 and converge_to_mA(0.2) == 200
    assert converge_to_mA(0.18) == 180 and converge_to_mA(0.01) == 10 and converge_to_mA("0.001") == 1
    for bad in (-0.1, float("nan"), float("inf"), -1):
        with pytest.raises(ValueError):
            converge_to_mA(bad)


def test_dmpfold_cli_accepts_and_rejects_tolerances(capsys):
    from dmpfold2_amd.predict import dmpfold_parser
    ap = dmpfold_parser()
    assert ap.parse_args(["-i", "x.aln"]).converge is None
    assert ap.parse_args(["-i", "x.aln", "-c", "0.2"]).converge == 0.2
    assert ap.parse_args(["-i", "x.aln", "--converge", "0"]).converge == 0.0
    args = ap.parse_args(["-i", "x.aln", "-n", "30", "-m", "200", "-c", "0.18"])
    assert (args.iterations, args.minsteps, args.converge) == (30, 200, 0.18)
    for bad in ("-0.1", "-1", "nan", "abc", "inf"):
        with pytest.raises(SystemExit) as ei:
            ap.parse_args(["-i", "x.aln", "-c", bad])
        assert ei.value.code == 2
    capsys.readouterr()


def test_batch_cli_accepts_and_rejects_tolerances(capsys):
    from dmpfold2_amd.batch import batch_parser
    ap = batch_parser()
    assert ap.parse_args(["-l", "t.txt", "-o", "out"]).converge is None
    assert ap.parse_args(["-l", "t.txt", "-o", "out", "--converge", "0.2"]).converge == 0.2
    assert ap.parse_args(["-l", "t.txt", "-o", "out", "--converge", "0"]).converge == 0.0
    for bad in ("-0.5", "nan", "x"):
        with pytest.raises(SystemExit) as ei:
            ap.parse_args(["-l", "t.txt", "-o", "out", "--converge", bad])
        assert ei.value.code == 2
    capsys.readouterr()


def test_option_round_trip_through_the_c_abi():
    """Creating a context needs a GPU; the header's promises about the option names are checked in the GPU file.  Here:
    the binding has no new symbol (the feature goes through existing entry points)."""
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65
