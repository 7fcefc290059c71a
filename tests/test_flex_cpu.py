"""Option "flex" on the host (no GPU, no library): tests/flex_ref.py against its own bounds, the fairness of the traces the GPU
test uses, the layout arithmetic, score.unpack_flex / flex_json on reference blocks, the hidden flags of both parsers.  On the
parent commit none of the names exist and every test here fails."""
import json

import numpy as np
import pytest

import domains_ref as D
import flex_ref as F

from dmpfold2_amd import score as S

CONSTRUCTED = ("80+80", "100+150", "3x80", "insertion")
GLOBULES = (8, 9, 16, 63, 64, 65, 96, 128, 129, 257, 300, 321, 385)     # seed 0: what tests/test_gpu_flex.py runs, and the issue's list
_LEGS = {}


def _leg(key, cut_mA=7300):
    if (key, cut_mA) not in _LEGS:
        ca = D.constructed(key)[0] if isinstance(key, str) else D.globule(key, 0)
        _LEGS[(key, cut_mA)] = (ca, F.leg(ca, cut_mA))
    return _LEGS[(key, cut_mA)]


# ------------------------------------------------------------------------------------------------ the reference and its bounds
@pytest.mark.parametrize("key", CONSTRUCTED + GLOBULES)
def test_the_rounded_reference_stays_inside_its_bounds(key):
    ca, ref = _leg(key)
    res = F.check(ref, ref.raw())
    assert not F.failed(res), res
    assert max(r for r, _ in res.values()) < 0.25, res             # one rounding against 8 x (one rounding + float64 terms)


def test_the_bounds_bite():
    """A perturbed answer fails the check that names what was perturbed."""
    ca, ref = _leg(129)
    assert ref.msf_comparable and ref.alone.all()

    def broken(change):
        raw = {k: v.copy() for k, v in ref.raw().items()}
        change(raw)
        return F.failed(F.check(ref, raw))

    def set_(key, index, value):
        def change(raw):
            raw[key][index] = value
        return change

    assert "integers" in broken(set_("degree", 5, ref.degree[5] + 1))
    assert "integers" in broken(set_("header", 0, ref.contacts + 1))
    assert "integers" in broken(set_("header", 2, 2.0))
    assert "lambda" in broken(lambda raw: raw["header"].__setitem__(9, raw["header"][9] * np.float32(1 + 3e-6)))
    assert "orth" in broken(lambda raw: raw["modes"].__setitem__(3, raw["modes"][3] * np.float32(1 + 3e-6)))
    mixed = broken(lambda raw: raw["modes"].__setitem__(2, (raw["modes"][2] + np.float32(1e-4) * raw["modes"][3])))
    assert "residual" in mixed or "orth" in mixed
    assert "sign" in broken(lambda raw: raw["modes"].__setitem__(4, -raw["modes"][4]))
    # a rotation inside the plane of two separated modes leaves them orthonormal: the residual and the mode check see it
    # (1e-3 rad: the residual it makes is the angle times the gap of 0.23, against a bound of 8 x 2 EPS32 sigma = 2.7e-5)
    c, s = np.float32(np.cos(1e-3)), np.float32(np.sin(1e-3))

    def rotate(raw):
        a, b = raw["modes"][1].copy(), raw["modes"][2].copy()
        raw["modes"][1], raw["modes"][2] = c * a + s * b, c * b - s * a
    assert {"residual", "mode"} <= set(broken(rotate))
    assert "msf" in broken(lambda raw: raw["msf"].__setitem__(7, raw["msf"][7] * np.float32(1 + 3e-6)))
    assert "msf_self" in broken(lambda raw: raw["msf"].__setitem__(7, raw["msf"][7] * np.float32(1 + 6e-6)))
    assert "finite" in broken(set_("msf", 0, np.nan))


def test_the_definition_on_small_graphs():
    """A path and a complete graph, whose spectra are known in closed form; the zero rule; two components."""
    path = np.zeros((12, 3), dtype=np.float32)
    path[:, 0] = 3.8 * np.arange(12)
    ref = F.leg(path, 4000)
    assert ref.contacts == 11 and ref.sigma == 4 and list(ref.degree) == [1] + [2] * 10 + [1] and ref.components == 1
    assert np.allclose(ref.eigenvalues, 2.0 - 2.0 * np.cos(np.arange(8) * np.pi / 12), atol=1e-12)
    assert len(F.hinges(ref.modes[1])) == 1 and F.hinges(ref.modes[1])[0] == 5
    full = F.leg(np.zeros((9, 3), dtype=np.float32) + np.arange(9, dtype=np.float32)[:, None] * 0.1)
    assert full.contacts == 36 and full.sigma == 16 and full.components == 1 and np.allclose(full.eigenvalues[1:], 9.0)
    assert not full.alone[1:].any() and not full.msf_comparable and np.allclose(full.width[1:], 0.0, atol=1e-12)
    two = F.leg(np.concatenate([path, path + np.float32(500.0)]), 4000)
    assert two.components == 2 and two.used == 6 and not two.connected()
    lone = F.leg(np.concatenate([path[:8], np.full((1, 3), np.nan, dtype=np.float32)]), 4000)      # a NaN row touches nothing
    assert lone.degree[8] == 0 and lone.components == 2
    none = F.leg(np.arange(24, dtype=np.float32).reshape(8, 3) * 100.0)
    assert none.sigma == 0 and none.components == 8 and none.used == 0 and not none.msf.any()


# ------------------------------------------------------------------------------------------------ the inputs are fair
@pytest.mark.parametrize("key", CONSTRUCTED + GLOBULES)
def test_the_traces_are_fair(key):
    """What the GPU test leans on, asserted, so that a changed generator fails here instead of silently weakening it: the network
    is connected at 7.3 A, the seven non-zero eigenvalues and the one behind them have a relative gap of at least 0.019 (the
    issue's figure; the smallest here is 0.0217, at L = 300), and no pair lies within 1e-4 A of the cutoff (the smallest here
    is 1.9e-4 A, at L = 385; the contact test itself is exact in float64, so this guards the fixtures, not the kernel)."""
    ca, ref = _leg(key)
    assert ref.connected() and ref.components == 1 and ref.used == 7
    assert ref.relative_gap() >= 0.019, ref.relative_gap()
    assert F.cutoff_margin(ca) >= 1e-4, F.cutoff_margin(ca)
    # the hinge mode has no component so near zero that a rounding could move a sign change
    assert np.abs(ref.modes[1]).min() > 1e-5
    if not isinstance(key, str) and key in (8, 9, 16, 63, 64, 65, 129, 257, 321, 385):
        assert ref.alone.all() and ref.msf_comparable, key          # the GPU sweep compares these in full


def test_the_cutoffs_of_the_gpu_test_are_what_it_says():
    ca, low = _leg(96, 4000)
    _, high = _leg(96, 20000)
    assert low.connected() and low.contacts == 95 and low.sigma == 4           # the bare chain
    assert high.connected() and high.contacts > 96 * 95 // 4 and high.alone.all()
    assert F.cutoff_margin(ca, 4000) > 1e-4 and F.cutoff_margin(ca, 20000) > 1e-4
    for ref in (low, high):
        assert not F.failed(F.check(ref, ref.raw()))


def test_80_80_has_its_hinge_at_the_linker():
    ca, ref = _leg("80+80")
    h = F.hinges(ref.modes[1])
    assert any(abs(i - 79.5) <= 5 for i in h), h
    assert abs(ref.eigenvalues[1] - 0.081) < 1e-3 and abs(ref.eigenvalues[2] - 0.173) < 1e-3
    sides = np.arange(160) < 80
    assert F.parse_agreement(ref.modes[1], sides) > 0.95


# ------------------------------------------------------------------------------------------------ layout, unpacking, JSON
def test_layout_arithmetic():
    for L in (8, 65, 300):
        assert S.flex_floats(L) == 48 + 20 * L == F.block(L, 7300, _leg(8)[1].raw() if L == 8 else F.leg(D.globule(L, 0))).shape[0]
        off = S.Layout(L, score=True, domains=True, score_domains=True, align_m=7)
        on = off._replace(flex=True)
        assert off.flex is False and on.flex is True and S.Layout(L).flex_off == S.Layout(L).align_off
        assert on.flex_off == off.align_off == off.domain_score_off + S.domain_score_floats(L)
        assert on.align_off == on.flex_off + S.flex_floats(L) and on.total == off.total + S.flex_floats(L)
        for name in ("score_off", "mapscore_off", "ss_off", "exposure_off", "domains_off", "domain_search_off", "domain_score_off"):
            assert getattr(on, name) == getattr(off, name), name
        buf = np.arange(on.total, dtype=np.float32)
        out = on.split(buf)
        assert out.flex_block.shape == (S.flex_floats(L),) and out.flex_block[0] == on.flex_off and off.split(buf[:off.total]).flex_block is None
        assert np.array_equal(on.flex_block(buf), out.flex_block) and off.flex_block(buf) is None
        assert out._replace(coords=None).flex_block is out.flex_block
        alone = S.Layout(L, flex=True)
        assert alone.flex_off == L and alone.total == L + S.flex_floats(L)
    assert S.FLEX.option == "flex" and S.FLEX.field == "flex_block" and S.FLEX not in S.BLOCKS and S.FLEX.floats(10, True) == 248
    assert [S.flex_cut_mA(v) for v in (4, 7.3, 20.0)] == [4000, 7300, 20000]
    for bad in (3.999, 20.001, float("nan"), -1):
        with pytest.raises(ValueError):
            S.flex_cut_mA(bad)


def test_unpack_and_json_on_a_reference_block():
    ca, ref = _leg("80+80")
    model = F.leg(D.globule(160, 3))
    L = 160
    blk = F.block(L, 7300, model, ref)
    assert np.array_equal(blk.view(np.uint32), S.pack_flex(L, 7300, [model.raw() | {"eigenvalues": model.eigenvalues} | dict(zip(S.FLEX_FIELDS, model.raw()["header"][:4])),
                                                                    ref.raw() | {"eigenvalues": ref.eigenvalues} | dict(zip(S.FLEX_FIELDS, ref.raw()["header"][:4]))]).view(np.uint32))
    confs = np.linspace(0.2, 0.9, L)
    parse = D.parse(ca)
    dom = S.unpack_domains(D.block(D.parse(D.globule(160, 3)), parse), L)
    fx = S.unpack_flex(blk, L, confs=confs, domains=dom)
    assert fx["L"] == L and fx["cutoff"] == 7.3 and fx["has_native"] and fx["contacts"] == model.contacts and fx["sigma"] == model.sigma
    assert fx["components"] == 1 and fx["used"] == 7 and fx["first_mode"] == 1 and np.array_equal(fx["degree"], model.degree)
    assert fx["hinges"] == F.hinges(model.modes[1]) and len(fx["collectivity"]) == 7 and all(1.0 / L <= c <= 1.0 for c in fx["collectivity"])
    assert abs(fx["msf_norm"].mean() - 1.0) < 1e-12 and -1.0 <= fx["r_conf"] <= 1.0 and -1.0 <= fx["rho_conf"] <= 1.0
    assert "parse_agreement" not in fx or dom["domains"] >= 2
    nat = fx["native"]
    assert nat["hinges"] == F.hinges(ref.modes[1]) and "r_conf" not in nat
    assert nat["parse_agreement"] == F.parse_agreement(ref.modes[1], parse["labels"] == 0) > 0.95
    assert -1.0 <= fx["r_msf"] <= 1.0 and 0.0 <= fx["rmsip"] <= 1.0 + 1e-6
    same = S.unpack_flex(F.block(L, 7300, ref, ref), L)
    assert abs(same["r_msf"] - 1.0) < 1e-12 and abs(same["rmsip"] - 1.0) < 1e-6
    # Spearman's is Pearson's of the ranks, ties sharing theirs
    assert np.array_equal(S._ranks([3.0, 1.0, 3.0, 2.0]), [2.5, 0.0, 2.5, 1.0])
    mono = S.unpack_flex(blk, L, confs=1.0 - np.exp(model.msf))
    assert abs(mono["rho_conf"] - 1.0) < 1e-12 and mono["r_conf"] < 1.0
    # a uniform mode is fully collective, a mode on one residue is not
    assert abs(S.flex_collectivity(np.ones(50)) - 1.0) < 1e-12 and abs(S.flex_collectivity(np.eye(50)[3]) - 1.0 / 50) < 1e-12
    # one leg, a latched fault, a wrong size
    one = S.unpack_flex(F.block(L, 9000, model), L)
    assert not one["has_native"] and "native" not in one and one["cutoff"] == 9.0
    dead = S.unpack_flex(np.full(S.flex_floats(L), np.nan, dtype=np.float32), L)
    assert dead["contacts"] == 0 and dead["hinges"] == [] and not dead["has_native"] and dead["first_mode"] is None
    with pytest.raises(ValueError):
        S.unpack_flex(blk[:-1], L)
    js = S.flex_json(fx)
    assert json.loads(json.dumps(js)) == js and js["native"]["hinges"] == nat["hinges"] and "modes" not in js
    assert js["eigenvalues"][1] == float(np.float32(model.eigenvalues[1])) and js["r_msf"] == fx["r_msf"]
    full = S.flex_json(fx, arrays=True)
    assert len(full["modes"]) == 8 and len(full["msf"]) == L and full["degree"] == model.degree.tolist()
    assert json.loads(json.dumps(S.flex_json(dead)))["eigenvalues"] == [None] * 8
    # the sides of the first cut: a level-1 domain against the rest
    three = S.unpack_domains(D.block(D.parse(D.constructed("3x80")[0])), 240)
    sides = S.flex_parse_sides(three)
    nodes = D.parse(D.constructed("3x80")[0])["nodes"]
    want = np.array([(int(k) >> (int(k).bit_length() - 2)) == 2 for k in nodes])
    assert sides is not None and (np.array_equal(sides, want) or np.array_equal(sides, ~want))
    assert S.flex_parse_sides(S.unpack_domains(D.block(D.parse(D.globule(64, 0))), 64)) is None


# ------------------------------------------------------------------------------------------------ the two parsers
def test_the_parsers_take_the_flags_and_their_help_does_not_mention_them():
    from dmpfold2_amd import batch
    from dmpfold2_amd import predict as P
    single, many = P.dmpfold_parser(), batch.batch_parser()
    assert "flex" not in single.format_help() and "flex" not in many.format_help()
    a = single.parse_args(["-i", "x.aln", "--flex", "--flex-cutoff", "9.5", "--flex-file", "f.json"])
    assert a.flex is True and a.flex_cutoff == 9.5 and a.flex_file == "f.json" and P.flex_arguments(single, a) == 9.5
    plain = single.parse_args(["-i", "x.aln"])
    assert not any(hasattr(plain, k) for k in ("flex", "flex_cutoff", "flex_file")) and P.flex_arguments(single, plain) is None
    assert P.flex_arguments(single, single.parse_args(["-i", "x.aln", "--flex"])) == 7.3
    for bad in (["--flex-cutoff", "8"], ["--flex-file", "f"], ["--flex", "--flex-cutoff", "3"], ["--flex", "--flex-cutoff", "21"]):
        with pytest.raises(SystemExit):
            P.flex_arguments(single, single.parse_args(["-i", "x.aln"] + bad))
    b = many.parse_args(["-i", "x.aln", "-o", "out", "--flex", "--flex-cutoff", "6"])
    assert b.flex is True and b.flex_cutoff == 6.0
    assert not hasattr(many.parse_args(["-i", "x.aln", "-o", "out"]), "flex")
    for bad in (["--flex-cutoff", "8"], ["--flex", "--flex-cutoff", "30"]):
        with pytest.raises(SystemExit):
            batch.main(["-i", "x.aln", "-o", "out"] + bad)
    assert batch._FLEX is None
    with batch.batch_flex(8.0):
        assert batch._FLEX == 8.0
    assert batch._FLEX is None
    with pytest.raises(ValueError):
        with batch.batch_flex(2.0):
            pass
    assert "flex_cutoff" in str(__import__("inspect").signature(P.aln_to_flex)) and callable(P.Engine.set_flex) and callable(P.Pipeline.use_flex)
    brief = batch.flex_brief({"first_mode": 1, "eigenvalues": [0.0, 0.25] + [1.0] * 6, "components": 1, "hinges": [4, 9], "r_conf": 0.5})
    assert brief == {"lambda_1": 0.25, "components": 1, "hinges": 2, "r_conf": 0.5}
    summary = batch.flex_summary({"a": brief, "b": dict(brief, lambda_1=0.75, r_conf=None)})
    assert summary["flex_targets"] == 2 and summary["mean_flex_lambda_1"] == 0.5 and summary["median_flex_r_conf"] == 0.5


def test_write_result_takes_the_flex_result(tmp_path):
    import torch
    from dmpfold2_amd import batch
    ca, ref = _leg(16)
    L = 16
    fx = S.unpack_flex(F.block(L, 7300, ref), L, confs=np.linspace(0.1, 0.9, L))
    coords, confs = torch.zeros((L, 5, 3)), torch.linspace(0.1, 0.9, L)
    alnmat = np.zeros((1, L), dtype=np.uint8)
    path = batch.write_result(str(tmp_path), "t16.aln", coords, confs, alnmat, "npz", flex=fx)
    z = np.load(path)
    assert z["flex_eig"].shape == (8,) and z["flex_modes"].shape == (8, L) and z["flex_msf"].dtype == np.float32
    assert np.array_equal(z["flex_degree"], ref.degree) and z["flex_degree"].dtype == np.int32
    batch.write_result(str(tmp_path), "t16.aln", coords, confs, alnmat, "pdb", flex=fx)
    assert json.loads((tmp_path / "t16.flex.json").read_text()) == json.loads(json.dumps({"flex": S.flex_json(fx)}))
    (tmp_path / "plain").mkdir()
    batch.write_result(str(tmp_path / "plain"), "t16.aln", coords, confs, alnmat, "pdb")
    assert not (tmp_path / "plain" / "t16.flex.json").exists()
