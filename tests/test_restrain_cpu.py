"""The restrained final refinement (options "restrain_milli" / "restrain_cut_mA", include/dmpfold_hip.h) without a GPU: the
NumPy restatement of the step (tests/restrain_ref.py) against the properties the definition implies, and the host plumbing -
the limits of the Python boundary, the command lines, the report, and that nothing moves while the flag is absent."""
import json
import os

import numpy as np
import pytest

import restrain_ref as R
from conftest import GOLDEN

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def trace():
    """The 3FGX chain-A C-alpha trace (96 residues)."""
    return np.load(os.path.join(GOLDEN, "kat_refine_backbone.npz"))["ca_in"].astype(np.float32)


def _noisy(trace, sigma=0.5, seed=0):
    return (trace + np.random.default_rng(seed).normal(0.0, sigma, trace.shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_force_or_no_cutoff_is_the_plain_step(trace, dtype):
    """k = 0, cut = 0 and no map at all give the plain step's bits; the plain step is the reference minimiser's."""
    x = _noisy(trace)
    dm = R.distances(trace).astype(np.float32)
    plain = R.step(x, None, 0.0, 15.0, dtype)
    assert plain.dtype == dtype
    assert np.array_equal(R.step(x, dm, 0.0, 15.0, dtype), plain)
    assert np.array_equal(R.step(x, dm, 1.0, 0.0, dtype), plain)
    # cut = 0 through the restraint term itself (not the short cut of `step`): every pair fails the test, the sum is +-0
    assert not R.restraint_mask(dm, dtype(0.0)).any()
    assert np.array_equal(R.steric_accel(x, dtype) + R.restraint_accel(x, dm, 1.0, 0.0, dtype) + R.bond_accel(x, dtype),
                          R.steric_accel(x, dtype) + R.bond_accel(x, dtype))
    assert not np.array_equal(R.step(x, dm, 1.0, 15.0, dtype), plain)
    if dtype is np.float32:
        import torch
        import dmpfold_oracle as O
        ref = O.refine_coords(torch.from_numpy(x), 1).numpy()
        # the same float32 operations up to the order of the partner sum: a few ulp of a coordinate of up to 64 A
        assert np.abs(plain - ref).max() <= 4 * 2.0 ** -24 * 64


def test_a_nan_entry_is_skipped_not_multiplied_in(trace):
    x = _noisy(trace)
    dm = R.distances(trace).astype(np.float32)
    holed = dm.copy()
    holed[10, 40] = holed[40, 10] = np.nan
    a = R.restraint_accel(x, holed, 1.0, 15.0, np.float32)
    assert np.isfinite(a).all()
    far = dm.copy()
    far[10, 40] = far[40, 10] = 99.0                      # above the cutoff: skipped the same way
    assert np.array_equal(a, R.restraint_accel(x, far, 1.0, 15.0, np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_restraint_forces_of_a_symmetric_map_sum_to_zero(trace, dtype):
    """a_j's term from i is minus a_i's term from j (the map is symmetric, e and dr are even, dx is odd), so the forces sum
    to zero over the chain up to rounding: L^2 terms of at most 3 k each, summed in `dtype`."""
    x = _noisy(trace)
    dm = R.distances(trace).astype(np.float32)
    assert np.array_equal(dm, dm.T)
    L, k = len(x), 2.0
    a = R.restraint_accel(x, dm, k, 15.0, dtype)
    eps = np.finfo(dtype).eps
    assert np.abs(a).max() > 1.0                          # there are forces
    assert np.abs(a.sum(axis=0, dtype=np.float64)).max() <= L * L * 3 * k * eps
    # centroid drift of the restraint's own displacement: within the rounding of the coordinates it is added to
    moved = np.asarray(x, dtype) + a * dtype(0.001)
    drift = np.abs(moved.mean(axis=0, dtype=np.float64) - np.asarray(x, np.float64).mean(axis=0)).max()
    assert drift <= 2 * eps * np.abs(x).max()


def test_restraints_lower_the_distance_error_on_a_realisable_map(trace):
    """Map = the trace's own distances, start = the trace + noise, 100 steps, k = 1: the restrained run ends closer to the
    map (RMS distance error over i < j) than the plain run."""
    dm = R.distances(trace).astype(np.float32)
    start = _noisy(trace)
    plain = R.refine(start, 100, None, 0.0, 15.0, np.float32)
    restrained = R.refine(start, 100, dm, 1.0, 15.0, np.float32)
    e0, e_plain, e_res = R.map_rms(dm, start), R.map_rms(dm, plain), R.map_rms(dm, restrained)
    print(f"map_rms: start {e0:.4f}  plain {e_plain:.4f}  restrained {e_res:.4f}")
    assert e_res < e_plain
    assert R.map_rms(dm, R.refine(start, 100, dm, 1.0, 15.0, np.float64)) < R.map_rms(dm, R.refine(start, 100, None, 0, 15.0, np.float64))


# ------------------------------------------------------------------------------------------------ host plumbing
def test_restrain_to_milli_limits():
    from dmpfold2_amd.predict import restrain_to_milli, restrain_cutoff_to_mA, restrain_options
    assert restrain_to_milli(None) == 0 and restrain_to_milli(0) == 0 and restrain_to_milli(1) == 1000
    assert restrain_to_milli(0.0015) == 2 and restrain_to_milli(100.0) == 100000 and restrain_to_milli("2.5") == 2500
    for bad in (-0.001, -1, 100.001, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            restrain_to_milli(bad)
    assert restrain_cutoff_to_mA(15.0) == 15000 and restrain_cutoff_to_mA(0) == 0 and restrain_cutoff_to_mA(100) == 100000
    for bad in (-1.0, 100.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            restrain_cutoff_to_mA(bad)
    assert restrain_options(None, "nonsense") is None                 # no restraint asked for: nothing is looked at
    assert restrain_options(1.0) == (1000, 15000) and restrain_options(0.5, 8.0) == (500, 8000)
    with pytest.raises(ValueError):
        restrain_options(1.0, -2.0)


def test_cli_parsing():
    from dmpfold2_amd.predict import dmpfold_parser
    from dmpfold2_amd.batch import batch_parser
    p = dmpfold_parser()
    a = p.parse_args(["-i", "x.aln"])
    assert a.restrain is None and a.restrain_cutoff == 15.0
    assert p.parse_args(["-i", "x.aln", "-r", "1"]).restrain == 1.0
    a = p.parse_args(["-i", "x.aln", "--restrain", "0.25", "--restrain-cutoff", "12"])
    assert (a.restrain, a.restrain_cutoff) == (0.25, 12.0)
    b = batch_parser()
    a = b.parse_args(["-o", "out"])
    assert a.restrain is None and a.restrain_cutoff == 15.0
    a = b.parse_args(["-o", "out", "--restrain", "2", "--restrain-cutoff", "10.5"])
    assert (a.restrain, a.restrain_cutoff) == (2.0, 10.5)
    for parser, lead in ((p, ["-i", "x.aln"]), (b, ["-o", "out"])):
        for bad in (["--restrain", "-1"], ["--restrain", "101"], ["--restrain", "nan"], ["--restrain", "abc"],
                    ["--restrain", "1", "--restrain-cutoff", "-3"], ["--restrain", "1", "--restrain-cutoff", "inf"]):
            with pytest.raises(SystemExit):
                parser.parse_args(lead + bad)
    with pytest.raises(SystemExit):
        b.parse_args(["-o", "out", "-r", "1"])                          # the short form is the single-target tool's


def test_report_on_a_six_residue_toy():
    """Hand-computed: a chain along x with the last residue folded back onto the second.
    CA x = 0, 3.8, 7.6, 11.4, 15.2; residue 5 at (3.8, 2, 0).
    Pairs with |i - j| >= 2 (10 of them) and their distances: (0,2) 7.6, (0,3) 11.4, (0,4) 15.2, (0,5) sqrt(3.8^2 + 4) = 4.294,
    (1,3) 7.6, (1,4) 11.4, (1,5) 2.0, (2,4) 7.6, (2,5) sqrt(3.8^2 + 4) = 4.294, (3,5) sqrt(7.6^2 + 4) = 7.859.
    One pair is closer than 3.0: clashes = 1.  Bonds: four of 3.8 (deviation 0.02) and (4,5) = sqrt(11.4^2 + 4) = 11.574:
    bond_dev_max = 11.574 - 3.78.  Map: 5 everywhere but (0,1) = 4, (0,2) = 20, (1,4) = 9.99, (2,4) = 10 and (3,5) = NaN, cutoff 10:
    of the ten pairs (0,2), (2,4) and (3,5) are not below the cutoff, (0,1) is no pair at all: restrained_pairs = 7."""
    from dmpfold2_amd.predict import restrain_report
    ca = np.array([[0, 0, 0], [3.8, 0, 0], [7.6, 0, 0], [11.4, 0, 0], [15.2, 0, 0], [3.8, 2, 0]], dtype=np.float32)
    coords = np.zeros((6, 5, 3), dtype=np.float32) + 1000.0            # the other atoms are not looked at
    coords[:, 1] = ca
    dm = np.full((6, 6), 5.0, dtype=np.float32)
    for (i, j), v in {(0, 1): 4.0, (0, 2): 20.0, (1, 4): 9.99, (2, 4): 10.0, (3, 5): np.nan}.items():
        dm[i, j] = dm[j, i] = v
    rep = restrain_report(1.5, 10.0, 100, dm, 3.25, coords)
    assert list(rep) == ["k", "cutoff", "steps", "map_rms", "restrained_pairs", "clashes", "bond_dev_max"]
    assert (rep["k"], rep["cutoff"], rep["steps"], rep["map_rms"]) == (1.5, 10.0, 100, 3.25)
    assert rep["restrained_pairs"] == 7 and rep["clashes"] == 1
    assert abs(rep["bond_dev_max"] - (np.sqrt(11.4 ** 2 + 4.0) - 3.78)) < 1e-5
    json.dumps(rep)                                                    # plain Python numbers
    import torch
    assert restrain_report(1.5, 10.0, 100, torch.from_numpy(dm), 3.25, torch.from_numpy(coords)) == rep
    # an engine whose "emit_distmap" was taken away by hand: no map, the trace's figures stay
    rep = restrain_report(1.5, 10.0, 100, None, None, coords)
    assert rep["restrained_pairs"] is None and rep["map_rms"] is None and rep["clashes"] == 1


class _Stub:
    """get_option / set_option of an engine, every call recorded."""

    def __init__(self, **options):
        self.options = dict(options)
        self.gets, self.sets = [], []

    def get_option(self, name):
        self.gets.append(name)
        return self.options[name]

    def set_option(self, name, value):
        self.sets.append((name, value))
        self.options[name] = value


def test_call_options_set_and_restore_the_restraint():
    from dmpfold2_amd.predict import Engine, Extras, restrain_options
    before = {"restrain_milli": 0, "restrain_cut_mA": 15000, "emit_distmap": 0}
    stub = _Stub(**before)
    with Engine._call_options(stub, None, Extras(), restrain_options(1.0, 12.0)):
        assert stub.options == {"restrain_milli": 1000, "restrain_cut_mA": 12000, "emit_distmap": 1}
    assert stub.options == before
    # k = 0 asked for: the option goes off for the call, the map is not turned on
    stub = _Stub(restrain_milli=500, restrain_cut_mA=15000, emit_distmap=0)
    with Engine._call_options(stub, None, Extras(), restrain_options(0.0)):
        assert stub.options == {"restrain_milli": 0, "restrain_cut_mA": 15000, "emit_distmap": 0}
    assert stub.options["restrain_milli"] == 500


def test_without_the_flag_nothing_is_touched(tmp_path):
    """restrain None: the call's options never name the two options, the parsers' defaults lead there, and write_result
    writes the files it wrote."""
    import torch
    from dmpfold2_amd.predict import Engine, Extras, dmpfold_parser, restrain_options
    from dmpfold2_amd.batch import batch_parser, write_result
    for args in (dmpfold_parser().parse_args(["-i", "x.aln"]), batch_parser().parse_args(["-o", "out"])):
        assert restrain_options(args.restrain, args.restrain_cutoff) is None
    stub = _Stub(recycle_tol_mA=0, emit_distmap=0, score_native=0)
    with Engine._call_options(stub, None, Extras(), None):
        pass
    with Engine._call_options(stub, None, Extras()):
        pass
    assert stub.sets == [] and not any("restrain" in name for name in stub.gets)
    coords = torch.arange(8 * 15, dtype=torch.float32).reshape(8, 5, 3)
    confs = torch.linspace(0.1, 0.9, 8)
    alnmat = np.zeros((1, 8), dtype=np.uint8)
    for fmt in ("pdb", "ca", "npz"):
        plain, flagged = tmp_path / (fmt + "_plain"), tmp_path / (fmt + "_restrained")
        plain.mkdir()
        flagged.mkdir()
        write_result(str(plain), "t.aln", coords, confs, alnmat, fmt)
        rep = {"k": 1.0, "cutoff": 15.0, "steps": 100, "map_rms": 2.5, "restrained_pairs": 20, "clashes": 0, "bond_dev_max": 0.25}
        write_result(str(flagged), "t.aln", coords, confs, alnmat, fmt, restrain=rep)
        assert sorted(os.listdir(plain)) == ["t.npz" if fmt == "npz" else "t.pdb"]
        if fmt == "npz":
            a, b = np.load(plain / "t.npz"), np.load(flagged / "t.npz")
            assert sorted(a.files) == ["alnmat", "confs", "coords"]
            assert sorted(set(b.files) - set(a.files)) == sorted("restrain_" + k for k in rep)
            assert b["restrain_steps"].dtype == np.int32 and int(b["restrain_restrained_pairs"]) == 20
            assert b["restrain_map_rms"].dtype == np.float32 and float(b["restrain_bond_dev_max"]) == 0.25
        else:
            assert sorted(os.listdir(flagged)) == ["t.pdb", "t.restrain.json"]
            assert (plain / "t.pdb").read_bytes() == (flagged / "t.pdb").read_bytes()
            assert json.loads((flagged / "t.restrain.json").read_text()) == {"restrain": rep}


def test_batch_summary_part():
    from dmpfold2_amd.batch import restrain_summary
    reports = {"a": {"k": 1.0, "cutoff": 15.0, "steps": 100, "map_rms": 2.0, "restrained_pairs": 10, "clashes": 0, "bond_dev_max": 0.1},
               "b": {"k": 1.0, "cutoff": 15.0, "steps": 100, "map_rms": 4.0, "restrained_pairs": 30, "clashes": 4, "bond_dev_max": 0.5},
               "c": {"k": 1.0, "cutoff": 15.0, "steps": 100, "map_rms": 9.0, "restrained_pairs": 20, "clashes": 2, "bond_dev_max": 0.3}}
    s = restrain_summary(reports)
    assert s["restrained_targets"] == 3 and s["restrain"] == reports
    assert (s["mean_map_rms"], s["median_map_rms"]) == (5.0, 4.0)
    assert (s["mean_restrained_pairs"], s["median_restrained_pairs"]) == (20.0, 20.0)
    assert (s["mean_clashes"], s["median_clashes"]) == (2.0, 2.0)
    assert abs(s["mean_bond_dev_max"] - 0.3) < 1e-12 and s["median_bond_dev_max"] == 0.3


def test_abi_is_unchanged():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dmpfold_hip.h")) as fh:
        header = fh.read()
    assert "#define DMP_ABI_VERSION 5" in header
    assert '"restrain_milli"' in header and '"restrain_cut_mA"' in header
