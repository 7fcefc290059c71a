"""Option "exposure" without a GPU: the committed sphere points, the NumPy restatement of the definition (tests/exposure_ref.py)
on its known answers and edge cases, the proof that its neighbour prefilter changes no count, the layout of the exposure block
in the d_conf buffer, the host side's unpacking, and the front ends' arguments.  tests/test_gpu_exposure.py compares the library
with the restatement."""
import itertools
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import exposure_ref as X
from test_ss_cpu import backbone, flat_hairpin, ideal_helix, native_3fgx

from dmpfold2_amd import score as S

NO_GLY = np.zeros(4096, dtype=np.uint8)
POINTS = S.exposure_points()


@pytest.fixture(scope="module")
def fgx():
    """The restatement on 3FGX chain A (L = 96, no glycine flagged), made once."""
    return X.exposure(backbone(native_3fgx()), NO_GLY, POINTS)


# ---- the sphere points -------------------------------------------------------------------------------------------------------
def test_committed_header_holds_the_points_bit_for_bit():
    with open(os.path.join(ROOT, "dmpfold2_amd", "csrc", "exposure_points.h")) as f:
        text = "".join(line for line in f if not line.lstrip().startswith("//"))
    lits = re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+(?=f)", text)
    assert len(lits) == 768
    got = np.asarray([float.fromhex(v) for v in lits], dtype=np.float64)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)            # each literal is a float32
    assert np.array_equal(got.astype(np.float32).view(np.uint32), POINTS.reshape(-1).view(np.uint32))
    assert POINTS.shape == (256, 3) and POINTS.dtype == np.float32
    assert np.abs(np.sqrt((POINTS.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-7
    assert np.all(np.diff(POINTS[:, 2]) < 0) and POINTS[0, 2] == np.float32(1.0 - 1.0 / 256.0)


def test_generator_writes_the_committed_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_exposure_points", os.path.join(ROOT, "tools", "make_exposure_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "dmpfold2_amd", "csrc", "exposure_points.h")) as f:
        assert f.read() == mod.text()


# ---- the definition's known answers ------------------------------------------------------------------------------------------
def test_isolated_atom_is_wholly_exposed():
    n = X.surface_atoms(np.zeros((1, 3), np.float32), [3.27], [True], POINTS)
    assert n.tolist() == [256]
    far = X.surface_atoms(np.asarray([[0, 0, 0], [6.5, 0, 0]], np.float32), [3.2, 3.2], [True, True], POINTS)
    assert far.tolist() == [256, 256]                                         # 6.5 > 3.2 + 3.2: the spheres do not meet


def test_coincident_atoms_bury_the_one_that_fits_inside():
    """Two atoms on one centre: every point of the smaller lies inside the larger, none of the larger's inside the smaller.
    (With EQUAL radii each point lies on the partner's sphere up to the rounding of the unit vector - a boundary the definition
    decides by its arithmetic, not one a test can name; the two counts then still hold no point twice.)"""
    c = np.asarray([[1.5, -2.0, 0.25]] * 2, np.float32)
    assert X.surface_atoms(c, [2.80, 3.27], [True, True], POINTS).tolist() == [0, 256]
    same = X.surface_atoms(c, [3.2, 3.2], [True, True], POINTS)
    assert same[0] == same[1] and 0 <= same[0] <= 256
    near = X.surface_atoms(np.asarray([[0, 0, 0], [0, 0, 1.0]], np.float32), [3.2, 3.2], [True, True], POINTS)
    assert near[0] == near[1] and 0 < near[0] < 256 and near[0] == int((POINTS[:, 2].astype(np.float64) * 3.2 <= 0.5).sum())


def test_glycine_cb_neither_has_nor_blocks_points():
    bb = backbone(ideal_helix(16))
    row = NO_GLY[:16].copy()
    row[[5, 9]] = 7
    e = X.exposure(bb, row, POINTS)
    assert np.all(e["n"][[5, 9], 4] == -1) and np.all(e["n"][row != 7] >= 0) and e["atoms"] == 5 * 16 - 2
    # the same counts as a structure from which those two atoms were taken away ...
    present = np.ones((16, 5), dtype=bool)
    present[[5, 9], 4] = False
    gone = X.surface_atoms(bb.reshape(-1, 3)[present.reshape(-1)], np.tile(X.RADII, 16)[present.reshape(-1)],
                           np.ones(present.sum(), dtype=bool), POINTS)
    assert np.array_equal(e["n"][present], gone)
    # ... and its neighbours see more than with the CB in place; the pair counts use the CB position all the same
    full = X.exposure(bb, NO_GLY, POINTS)
    assert np.all(e["n"][present] >= full["n"][present]) and (e["n"][present] > full["n"][present]).any()
    for k in ("hse_up", "hse_down", "cn10"):
        assert np.array_equal(e[k], full[k])
    assert e["sums"][4] == int(e["n"][row != 7, 4].sum()) and e["buried_atoms"] == int((e["n"] == 0).sum())


def test_3fgx_chain_a(fgx):
    """3FGX chain A on the oracle-rebuilt backbone: 6314.45 square Angstrom (the prototype's 6314), mean hse_up 12.40, hse_down
    14.65, cn10 13.90; 480 atoms, 68 of them without an exposed point."""
    total = X.area(fgx["n"])
    print(total, fgx["hse_up"].mean(), fgx["hse_down"].mean(), fgx["cn10"].mean(), fgx["sums"], fgx["buried_atoms"])
    assert abs(total - 6314.0) <= 0.01 * 6314.0
    assert round(float(fgx["hse_up"].mean()), 1) == 12.4 and round(float(fgx["hse_down"].mean()), 1) == 14.6
    assert fgx["atoms"] == 480 and fgx["sums"] == [462, 1330, 408, 3188, 7915] and fgx["buried_atoms"] == 68
    assert np.all((fgx["n"] >= 0) & (fgx["n"] <= 256))
    near = fgx["hse_up"] + fgx["hse_down"]
    assert np.all(near >= 2) and np.all(near < 96)


def test_half_sphere_counts_on_a_line():
    """Residues on the x axis 3.8 apart, every CB straight up (+z) from its CA and tilted towards +x: `up` counts the residues
    ahead within 13 A (3 of them), `down` those behind - a perpendicular w counts as down."""
    L = 9
    bb = np.zeros((L, 5, 3), np.float32)
    bb[:, :, 0] = (3.8 * np.arange(L))[:, None]
    bb[:, 4, 2] = 1.5
    bb[:, 4, 0] += 0.25
    e = X.exposure(bb, NO_GLY, POINTS)
    assert e["hse_up"].tolist() == [3, 3, 3, 3, 3, 3, 2, 1, 0] and e["hse_down"].tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3]
    assert e["cn10"].tolist() == [2, 3, 4, 4, 4, 4, 4, 3, 2]
    bb[:, 4, 0] = bb[:, 1, 0]                                                 # v . w = 0 exactly: not up, so down
    e = X.exposure(bb, NO_GLY, POINTS)
    assert e["hse_up"].sum() == 0 and e["hse_down"].tolist() == [3, 4, 5, 6, 6, 6, 5, 4, 3]


def test_nan_coordinates_fail_every_comparison():
    bb = backbone(ideal_helix(12))
    bb[4, 1] = np.nan
    e = X.exposure(bb, NO_GLY, POINTS)
    assert e["n"][4, 1] == 256                                                # its points are NaN: none is buried
    assert e["hse_up"][4] == 0 and e["hse_down"][4] == 0 and np.all(e["n"] >= 0)


# ---- the prefilter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["helix", "hairpin", "3fgx", "blob"])
def test_prefilter_changes_no_count(name, fgx):
    rng = np.random.default_rng(7)
    trace = {"helix": ideal_helix(40), "hairpin": flat_hairpin(), "3fgx": native_3fgx(),
             "blob": (rng.standard_normal((48, 3)) * 3.0).astype(np.float32)}[name]
    bb = backbone(trace)
    row = (rng.integers(0, 20, size=bb.shape[0])).astype(np.uint8)
    a = fgx if name == "3fgx" else X.exposure(bb, row, POINTS)
    b = X.exposure(bb, NO_GLY if name == "3fgx" else row, POINTS, prefilter=False)
    assert np.array_equal(a["n"], b["n"]) and a["sums"] == b["sums"] and a["buried_atoms"] == b["buried_atoms"]


# ---- the layout --------------------------------------------------------------------------------------------------------------
GRID = list(itertools.product((False, True), (False, True), (False, True), (None, 3, 61), (None, (3, 120)), (None, 11), (False, True)))


def _lay(L, distmap, score, score_map, align_m, search, passes, ss, **kw):
    return S.Layout(L, distmap, score, score_map and distmap and score, align_m, search, 2048, passes if score else None, ss=ss, **kw)


@pytest.mark.parametrize("L", [8, 96, 2048])
def test_layout_off_is_todays_and_on_moves_what_lies_behind(L):
    names = ("info_off", "score_off", "mapscore_off", "pass_off", "ss_off", "exposure_off", "align_off", "align_end", "search_off",
             "search_end", "total")
    behind = ("align_off", "align_end", "search_off", "search_end", "total")
    for row in GRID:
        off, on = _lay(L, *row), _lay(L, *row, exposure=True)
        assert off.exposure is False and on.exposure is True and off != on and off == _lay(L, *row, exposure=False)
        assert S.Layout._fields == ("L", "distmap", "score", "score_map", "align_m", "search", "max_L", "passes", "ss", "exposure") and off.ss == on.ss == row[-1]
        # off: the grid of tests/test_ss_cpu.py, stated again from the lengths of the blocks
        assert off.exposure_off == off.align_off == off.ss_off + (S.ss_floats(L) if row[-1] else 0)
        for name in names:
            assert getattr(on, name) - getattr(off, name) == (32 + 16 * L if name in behind else 0), (row, name)
        assert on.align_off - on.exposure_off == S.exposure_floats(L) == 32 + 16 * L
        assert on._replace(distmap=on.distmap).exposure is True and on._replace(exposure=False) == off
        assert on._replace(ss=not on.ss).exposure is True and on._replace(ss=not on.ss).ss is (not row[-1])
        buf = np.arange(on.total, dtype=np.float64)
        got, base = on.split(buf), off.split(buf[:off.total])
        assert base.exposure_block is None and got.exposure_block.shape == (32 + 16 * L,) and got.exposure_block[0] == on.exposure_off
        assert (got.ss_block is None) == (not row[-1]) and (got.ss_block is None or got.ss_block.shape == (32 + 8 * L,))
        for f in S.Outputs._fields[:10]:            # (every part but the exposure block)
            a, b = getattr(got, f), getattr(base, f)
            assert (a is None) == (b is None)
            if a is not None and f != "coords":
                assert a.size == b.size and a.reshape(-1)[0] - b.reshape(-1)[0] == (32 + 16 * L if f in ("align_block", "search_block") else 0)
        with pytest.raises(ValueError):
            on.split(buf[:-1])


def test_outputs_carry_both_blocks_beside_the_tuple():
    parts = {name: object() for name in S.Outputs._fields[:9]}
    ss, ex = object(), object()
    out = S.Outputs(**parts, ss_block=ss, exposure_block=ex)
    assert S.Outputs._fields == ("coords", "confs", "distmap", "info", "score_block", "align_block", "search_block", "map_block", "pass_block",
                                "ss_block", "exposure_block")
    assert S.Outputs(**parts).exposure_block is None and S.Outputs(**parts, ss_block=ss).exposure_block is None
    pub = out.public()
    assert len(pub) == 11 and pub[-2] is ss and pub[-1] is ex and out.public(exposure=False) == pub[:-1]
    assert out.public(ss=False)[-1] is ex and out.public(blocks=False) == pub[:4]
    back = S.Outputs.of(pub, True, True, True, True, True, True, ss=True, exposure=True)
    assert back.ss_block is ss and back.exposure_block is ex and all(a is b for a, b in zip(back, out))
    only = S.Outputs.of(out.public(ss=False), True, True, True, True, True, True, exposure=True)
    assert only.ss_block is None and only.exposure_block is ex
    kept = out._replace(coords=None)
    assert kept.ss_block is ss and kept.exposure_block is ex and out._replace(exposure_block=None).ss_block is ss
    assert out == S.Outputs(**parts, ss_block=ss, exposure_block=ex) and out != S.Outputs(**parts, ss_block=ss)
    assert "exposure_block=" in repr(out)


# ---- the host side -----------------------------------------------------------------------------------------------------------
def test_unpack_and_json_round_trip(fgx):
    L = 96
    helix = X.exposure(backbone(ideal_helix(L)), NO_GLY, POINTS)
    seq = ("AVILMFWC" + "GDEKRSTN") * 6
    ex = S.unpack_exposure(X.block_of(fgx, L, helix), L, seq=seq)
    assert ex["points"] == 256 and ex["atoms"] == fgx["atoms"] and ex["sums"] == fgx["sums"] and ex["buried_atoms"] == fgx["buried_atoms"]
    assert np.array_equal(ex["n"], fgx["n"]) and ex["n"].dtype == np.int64 and ex["n"].shape == (L, 5)
    for k in ("hse_up", "hse_down", "cn10"):
        assert np.array_equal(ex[k], fgx[k]) and ex["mean_" + k] == float(fgx[k].mean())
    assert ex["area"] == pytest.approx(X.area(fgx["n"]), rel=1e-12) and ex["area_res"].sum() == pytest.approx(ex["area"], rel=1e-12)
    assert ex["area_atom"][3, 1] == 4.0 * np.pi * 3.27 * 3.27 * fgx["n"][3, 1] / 256.0
    assert np.array_equal(ex["cb_exposed"], fgx["n"][:, 4] / 256.0)
    hyd = np.asarray([c in "AVILMFWC" for c in seq])
    assert ex["cb_hydrophobic"] == pytest.approx(float((fgx["n"][hyd, 4] / 256.0).mean()))
    gly = np.asarray([c == "G" for c in seq])
    assert ex["cb_other"] == pytest.approx(float((fgx["n"][~hyd, 4] / 256.0).mean())) and not gly[hyd].any()
    assert ex["burial_ratio"] == pytest.approx(ex["cb_hydrophobic"] / ex["cb_other"])
    assert ex["has_native"] and np.array_equal(ex["native"]["n"], helix["n"]) and ex["native"]["atoms"] == helix["atoms"]
    want = np.corrcoef(ex["area_res"], ex["native"]["area_res"])[0, 1]
    assert ex["r_area"] == pytest.approx(want) and -1.0 <= ex["r_cn10"] <= 1.0 and -1.0 <= ex["r_hse_up"] <= 1.0
    js = json.loads(json.dumps({"exposure": S.exposure_json(ex)}))["exposure"]
    assert js["area"] == ex["area"] and js["sums"] == fgx["sums"] and js["native"]["atoms"] == helix["atoms"] and js["has_native"] is True
    assert js["burial_ratio"] == ex["burial_ratio"] and js["r_area"] == ex["r_area"] and "n" not in js and "hse_up" not in js
    full = json.loads(json.dumps(S.exposure_json(ex, arrays=True)))
    assert full["n"] == fgx["n"].tolist() and full["cn10"] == fgx["cn10"].tolist() and len(full["area_res"]) == L
    # glycines: -1 in n, no area, NaN in cb_exposed, outside both burial means
    row = NO_GLY[:L].copy()
    row[::8] = 7
    g = X.exposure(backbone(native_3fgx()), row, POINTS)
    eg = S.unpack_exposure(X.block_of(g, L), L, seq=row)
    assert np.all(eg["n"][::8, 4] == -1) and np.all(eg["area_atom"][::8, 4] == 0.0) and np.isnan(eg["cb_exposed"][::8]).all()
    assert not eg["has_native"] and "native" not in eg and "r_area" not in eg and eg["atoms"] == 5 * L - 12
    assert np.isnan(eg["cb_other"]) and eg["cb_hydrophobic"] == pytest.approx(float(np.nanmean(eg["cb_exposed"])))     # code 0 = A
    assert S.exposure_json(eg)["burial_ratio"] is None
    alone = S.unpack_exposure(X.block_of(fgx, L), L)
    assert not alone["has_native"] and "cb_hydrophobic" not in alone and "burial_ratio" not in S.exposure_json(alone)
    nan = S.unpack_exposure(np.full(S.exposure_floats(L), np.nan, dtype=np.float32), L)
    assert nan["points"] == 0 and nan["atoms"] == 0 and np.all(nan["n"] == -1) and nan["area"] == 0.0 and not nan["has_native"]
    with pytest.raises(ValueError):
        S.unpack_exposure(np.zeros(S.exposure_floats(L) - 1, dtype=np.float32), L)
    with pytest.raises(ValueError):
        S.unpack_exposure(X.block_of(fgx, L), L, seq="A" * (L - 1))


# ---- the front ends ----------------------------------------------------------------------------------------------------------
def test_extras_default_and_front_end_arguments():
    from dmpfold2_amd import batch, _lib
    from dmpfold2_amd.predict import dmpfold_parser, Extras, Flags, Prediction, agree_ss
    assert Extras().exposure is False and Extras(exposure=True).exposure is True and Extras._fields == ("distmap", "native", "structure", "library", "score_map", "score_passes", "ss", "exposure")
    assert Extras(exposure=True).ss is False and Extras(ss=True, exposure=True)._replace(distmap=True).exposure is True
    assert Extras(True)._replace(exposure=True).exposure is True and Extras(ss=True)._replace(exposure=True).ss is True
    assert Extras(exposure=True) != Extras() and Extras(exposure=True) == Extras(exposure=True)
    assert Flags(True, True, False, False, False, 0).exposure is False and Flags._fields[-2:] == ("ss", "exposure")
    assert Prediction._fields[-1] == "exposure" and Prediction(*range(8)).exposure is None
    assert agree_ss([1, 1], "exposure", "set_exposure") is True
    with pytest.raises(RuntimeError, match="exposure"):
        agree_ss([1, 0], "exposure", "set_exposure")
    args = dmpfold_parser().parse_args(["-i", "x.aln", "--exposure", "--exposure-file", "x.json"])
    assert args.exposure is True and args.exposure_file == "x.json" and args.ss is False
    plain = dmpfold_parser().parse_args(["-i", "x.aln"])
    assert plain.exposure is False and plain.exposure_file is None
    assert batch.batch_parser().parse_args(["-o", "out", "--exposure"]).exposure is True
    assert batch.batch_parser().parse_args(["-o", "out"]).exposure is False
    assert len(_lib.SIGNATURES) == 65


def test_batch_summary_and_files(tmp_path, fgx):
    from dmpfold2_amd import batch
    import torch
    L = 96
    seq = np.arange(L) % 20
    ex = S.unpack_exposure(X.block_of(fgx, L), L, seq=seq)
    js = S.exposure_json(ex)
    summary = batch.exposure_summary({"a": js, "b": js})
    assert summary["exposure_targets"] == 2 and summary["exposure"]["a"]["area"] == ex["area"]
    assert summary["mean_exposure_area"] == pytest.approx(ex["area"]) and summary["median_exposure_burial_ratio"] == pytest.approx(ex["burial_ratio"])
    assert "mean_exposure_r_area" not in summary
    coords, confs = torch.zeros((L, 5, 3)), torch.zeros((L,))
    alnmat = seq[None].astype(np.uint8)
    path = batch.write_result(str(tmp_path), "t.aln", coords, confs, alnmat, "npz", exposure=ex)
    z = np.load(path)
    assert np.array_equal(z["exp_n"], fgx["n"]) and z["exp_n"].shape == (L, 5) and np.array_equal(z["exp_area"], ex["area_res"])
    for k in ("hse_up", "hse_down", "cn10"):
        assert np.array_equal(z["exp_" + k], fgx[k])
    batch.write_result(str(tmp_path), "t.aln", coords, confs, alnmat, "ca", exposure=ex)
    assert json.loads((tmp_path / "t.exposure.json").read_text()) == {"exposure": json.loads(json.dumps(js))}
