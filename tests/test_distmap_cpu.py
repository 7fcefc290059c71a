"""The chosen pass's predicted distance map (option "emit_distmap", `distmap=` / `return_distmap=` / --distmap): what
can be checked without a GPU.

The pass whose map comes back is the one the reference's best-of rule keeps (network.py:302: strict '>' on the mean
confidence logit), and the reference-captured fixtures carry the reference's own per-pass means: the expected
`best_pass` of a fixture follows from the fixture alone.  `best_pass_of` below restates the rule;
tests/test_gpu_distmap.py imports it and the table, and holds the engine to them.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden


def best_pass_of(means):
    """The 0-based pass the strict '>' rule keeps, on float32 means as the reference compares them."""
    best, best_mean = 0, np.float32(means[0])
    for p in range(1, len(means)):
        if np.float32(means[p]) > best_mean:
            best, best_mean = p, np.float32(means[p])
    return best


# fixture -> (trunk passes, best pass, least distance of the best mean from the runner-up the GPU tests rely on)
BEST_PASS = {
    "pf10963_n0_m0": (1, 0, None),
    "synth_L40_N64_n2_m0": (3, 1, 2.6e-2),
    "pf10963_n3_m0": (4, 1, 8.3e-2),
    "synth_L300_N2000_n10_m0": (11, 4, 1e-3),
}


@pytest.mark.parametrize("name", list(BEST_PASS))
def test_expected_best_pass_follows_from_the_fixture(name):
    passes, best, margin = BEST_PASS[name]
    means = np.asarray(load_golden(name)["conf_mean_pass"], dtype=np.float32).reshape(-1)
    assert len(means) == passes
    assert best_pass_of(means) == best
    if margin is not None:
        # not a close call: another arithmetic (1e-4 on a confidence, 1e-3 on a per-pass mean) keeps the same pass
        gap = float(means[best]) - float(np.delete(means, best).max())
        print(name, "best", best, "of", passes, "runner-up", gap, "away")
        assert gap > margin
    # the same pass wins a shorter run that still contains it (the `-n best` runs of the GPU tests)
    assert best_pass_of(means[:best + 1]) == best


def test_the_fixture_with_two_equal_means_is_left_out():
    """actsmall's two best per-pass means are 7e-9 apart: which one a float32 engine keeps is a coin toss, so no test
    of the chosen pass uses it."""
    means = np.asarray(load_golden("actsmall_L128_N500_n3_m0")["conf_mean_pass"], dtype=np.float64)
    top = np.sort(means)[-2:]
    assert top[1] - top[0] < 1e-7


def test_best_pass_rule_properties():
    assert best_pass_of([0.5]) == 0
    assert best_pass_of([0.5, 0.5, 0.5]) == 0                  # strict: a tie keeps the earlier pass
    assert best_pass_of([0.1, 0.3, 0.3, 0.2]) == 1
    assert best_pass_of([0.1, float("nan"), 0.05]) == 0        # NaN never wins
    assert best_pass_of([-0.7, -0.8, -0.6]) == 2


def test_buffer_layout_helper():
    from dmpfold2_amd.predict import distmap_floats, split_distmap_buffer
    assert distmap_floats(82) == 82 + 82 * 82 + 3 and distmap_floats(82, False) == 82
    assert distmap_floats(2048) == 2048 + 2048 * 2048 + 3
    L = 5
    for buf in (torch.arange(distmap_floats(L), dtype=torch.float32), np.arange(distmap_floats(L), dtype=np.float32)):
        confs, dm, info = split_distmap_buffer(buf, L)
        assert tuple(confs.shape) == (L,) and tuple(dm.shape) == (L, L) and tuple(info.shape) == (3,)
        assert float(confs[0]) == 0 and float(confs[-1]) == L - 1
        assert float(dm[0, 0]) == L and float(dm[1, 0]) == 2 * L and float(dm[-1, -1]) == L + L * L - 1    # row-major
        assert [float(v) for v in info] == [L + L * L, L + L * L + 1, L + L * L + 2]
        buf[L + 1] = -1.0                                      # views of the one allocation, not copies
        assert float(dm[0, 1]) == -1.0
    for bad in (torch.zeros(distmap_floats(L) - 1), torch.zeros(L), torch.zeros((1, distmap_floats(L)))):
        with pytest.raises(ValueError):
            split_distmap_buffer(bad, L)


def test_dmpfold_cli_distmap_flag():
    from dmpfold2_amd.predict import dmpfold_parser
    ap = dmpfold_parser()
    assert ap.parse_args(["-i", "x.aln"]).distmap is None
    args = ap.parse_args(["-i", "x.aln", "-n", "3", "--distmap", "out/x.npy", "-c", "0.2"])
    assert (args.distmap, args.iterations, args.converge) == ("out/x.npy", 3, 0.2)
    with pytest.raises(SystemExit) as ei:
        ap.parse_args(["-i", "x.aln", "--distmap"])            # the flag needs its file
    assert ei.value.code == 2


def test_batch_cli_distmap_flag():
    from dmpfold2_amd.batch import batch_parser
    ap = batch_parser()
    assert ap.parse_args(["-l", "t.txt", "-o", "out"]).distmap is False
    args = ap.parse_args(["-l", "t.txt", "-o", "out", "--distmap", "--format", "npz"])
    assert args.distmap is True and args.format == "npz"


def _synthetic(L=7):
    g = load_golden("pf10963_n0_m0")
    rng = np.random.default_rng(3)
    dm = rng.random((L, L)).astype(np.float32) * 30.0
    dm = np.maximum(dm, dm.T)
    info = np.array([4.0, 11.0, 1.25], dtype=np.float32)
    return (torch.from_numpy(g["coords"][:L].copy()), torch.from_numpy(g["confs"][:L].copy()), g["alnmat"][:, :L],
            torch.from_numpy(dm), torch.from_numpy(info))


def test_npy_writer(tmp_path):
    from dmpfold2_amd.predict import save_distmap_npy
    _, _, _, dm, _ = _synthetic()
    for name in ("a.npy", "b.map"):                            # the file named is the file written, whatever its suffix
        p = tmp_path / name
        save_distmap_npy(str(p), dm)
        back = np.load(str(p))
        assert back.dtype == np.float32 and np.array_equal(back, dm.numpy())
    save_distmap_npy(str(tmp_path / "c.npy"), dm.double().numpy()[::1])      # arrays too; always float32 on disk
    assert (tmp_path / "c.npy").read_bytes() == (tmp_path / "a.npy").read_bytes()


def test_batch_writers(tmp_path):
    from dmpfold2_amd.batch import write_result
    coords, confs, alnmat, dm, info = _synthetic()
    out = tmp_path / "out"
    out.mkdir()
    z = np.load(write_result(str(out), "t/x.aln", coords, confs, alnmat, "npz", dm, info))
    assert set(z.files) == {"coords", "confs", "alnmat", "distmap", "best_pass", "passes_run", "map_rms"}
    assert np.array_equal(z["distmap"], dm.numpy()) and z["distmap"].dtype == np.float32
    assert int(z["best_pass"]) == 4 and int(z["passes_run"]) == 11 and z["map_rms"] == np.float32(1.25)
    assert np.array_equal(z["coords"], coords.numpy()) and np.array_equal(z["confs"], confs.numpy())
    # without the map: the arrays the format always had, and no file beside the structure
    z0 = np.load(write_result(str(out), "t/y.aln", coords, confs, alnmat, "npz"))
    assert set(z0.files) == {"coords", "confs", "alnmat"}
    for fmt in ("pdb", "ca"):
        stem = f"s_{fmt}"
        plain = open(write_result(str(out), f"t/{stem}_plain.aln", coords, confs, alnmat, fmt)).read()
        assert not (out / f"{stem}_plain.distmap.npy").exists()
        path = write_result(str(out), f"t/{stem}.aln", coords, confs, alnmat, fmt, dm, info)
        assert path.endswith(f"{stem}.pdb") and open(path).read() == plain      # the structure's text does not change
        assert np.array_equal(np.load(str(out / f"{stem}.distmap.npy")), dm.numpy())


def test_no_new_entry_point():
    """The feature goes through an option, the existing output buffer and dmp_debug_fetch."""
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65
