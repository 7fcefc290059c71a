"""Option "assign_ss" without a GPU: a vectorised NumPy restatement (`yardstick`) of the definition in include/dmpfold_hip.h,
its known answers on backbones rebuilt from C-alpha traces by the oracle's ca_to_backbone, its edge cases, the layout of the SS
block in the d_conf buffer, the host side's unpacking, and the front ends' arguments.  tests/test_gpu_ss.py compares the
library with `yardstick`."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import dmpfold_oracle as O          # noqa: E402

from dmpfold2_amd import score as S  # noqa: E402

COS70 = 0.3420201433256687
PAD = 6


def backbone(ca):
    """float32 (L, 5, 3) N, CA, C, O, CB from a C-alpha trace, by the oracle (float32, as the library builds it)."""
    ca = torch.from_numpy(np.ascontiguousarray(ca, dtype=np.float32)).reshape(1, -1, 3)
    return O.ca_to_backbone(ca).reshape(-1, 5, 3).numpy().astype(np.float32)


def _sq(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _dist(a, b):
    return np.sqrt(_sq(a[:, None, :] - b[None, :, :]))


def _shift(m, a, b):
    """out[i, j] = m[i + a, j + b], False outside"""
    L = m.shape[0]
    p = np.zeros((L + 2 * PAD, L + 2 * PAD), dtype=bool)
    p[PAD:PAD + L, PAD:PAD + L] = m
    return p[PAD + a:PAD + a + L, PAD + b:PAD + b + L]


def _first_two(m):
    """the two lowest column indices set in each row of a boolean matrix, -1 where absent"""
    L = m.shape[0]
    idx = np.where(m, np.arange(L)[None, :], L)
    part = np.sort(idx, axis=1)[:, :2] if L >= 2 else idx
    part = np.where(part == L, -1, part)
    return part[:, 0], part[:, 1]


def yardstick(coords, first_row):
    """The definition of include/dmpfold_hip.h on float32 coordinates (L, 5, 3) and the alignment's first row (codes):
    float64 formed from the float32 values, every operation in the order written.  -> dict with ss (L,) int codes, the header
    counts, e_acc / p_acc / e_don / p_don, bp1 / bp2, hb (L, L) bool, and fragile = (the smallest |E + 0.5| over the defined
    pairs, the smallest |a.b - cos70 |a||b|| over the bend residues): how far the nearest decision is from flipping."""
    X = np.asarray(coords, dtype=np.float32).astype(np.float64)
    L = X.shape[0]
    N, CA, C, Ox = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    pro = np.asarray(first_row).reshape(-1)[:L] == 14
    v = C[:-1] - Ox[:-1]
    vv = _sq(v)
    donor = np.zeros(L, dtype=bool)
    donor[1:] = ~pro[1:] & (vv > 0)
    H = np.zeros((L, 3))
    H[1:] = N[1:] + v / np.sqrt(np.where(vv > 0, vv, 1.0))[:, None]
    don, dch, doh, dcn = _dist(Ox, N), _dist(C, H), _dist(Ox, H), _dist(C, N)
    close = (don < 0.5) | (dch < 0.5) | (doh < 0.5) | (dcn < 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = 27.888 * (((1.0 / don + 1.0 / dch) - 1.0 / doh) - 1.0 / dcn)
    E = np.where(close, -9.9, np.where(e < -9.9, -9.9, e))
    ii, jj = np.arange(L)[:, None], np.arange(L)[None, :]
    valid = donor[None, :] & (np.abs(ii - jj) >= 2)
    hb = valid & (E < -0.5)
    Ev = np.where(valid, E, np.inf)
    out = {"hb": hb, "E": E, "valid": valid, "n_hb": int(hb.sum())}
    has_row, has_col = valid.any(axis=1), valid.any(axis=0)
    out["p_acc"] = np.where(has_row, Ev.argmin(axis=1), -1)
    out["e_acc"] = np.where(has_row, Ev.min(axis=1, initial=np.inf), 0.0).astype(np.float32)
    out["p_don"] = np.where(has_col, Ev.argmin(axis=0), -1)
    out["e_don"] = np.where(has_col, Ev.min(axis=0, initial=np.inf), 0.0).astype(np.float32)
    # turns and helices
    t = {n: np.array([hb[i, i + n] if i + n < L else False for i in range(L)] + [False] * 8, dtype=bool) for n in (3, 4, 5)}
    Hf, Gf, If, Tf = (np.zeros(L + 8, dtype=bool) for _ in range(4))
    for i in range(1, L - 4):
        if t[4][i - 1] and t[4][i]:
            Hf[i:i + 4] = True
    for i in range(1, L - 3):
        if t[3][i - 1] and t[3][i] and not Hf[i:i + 3].any():
            Gf[i:i + 3] = True
    for i in range(1, L - 5):
        if t[5][i - 1] and t[5][i] and not (Hf[i:i + 5] | Gf[i:i + 5]).any():
            If[i:i + 5] = True
    for n in (3, 4, 5):
        for i in range(L):
            if t[n][i]:
                Tf[i + 1:i + n] = True
    Hf, Gf, If, Tf = Hf[:L], Gf[:L], If[:L], Tf[:L]
    # bridges
    hbT = hb.T
    dom = (ii >= 1) & (jj >= 1) & (ii <= L - 2) & (jj <= L - 2) & (np.abs(ii - jj) >= 3)
    P = dom & ((_shift(hb, -1, 0) & _shift(hbT, 1, 0)) | (_shift(hbT, 0, -1) & _shift(hb, 0, 1)))
    A = dom & ((hb & hbT) | (_shift(hb, -1, 1) & _shift(hbT, 1, -1)))
    Ef = ((P & (_shift(P, -1, -1) | _shift(P, 1, 1))) | (A & (_shift(A, -1, 1) | _shift(A, 1, -1)))).any(axis=1)
    Bf = (P | A).any(axis=1)
    out["bp1"], out["bp2"] = _first_two(P | A)
    out["n_parallel"], out["n_antiparallel"] = int(np.triu(P, 1).sum()), int(np.triu(A, 1).sum())
    # bends
    Sf = np.zeros(L, dtype=bool)
    bend = np.inf
    if L >= 5:
        a, b = CA[2:-2] - CA[:-4], CA[4:] - CA[2:-2]
        ab = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        rhs = COS70 * (np.sqrt(_sq(a)) * np.sqrt(_sq(b)))
        Sf[2:L - 2] = ab < rhs
        bend = float(np.abs(ab - rhs).min())
    code = np.select([Hf, Ef, Bf, Gf, If, Tf, Sf], [7, 6, 5, 4, 3, 2, 1], 0)
    out["ss"] = code
    out["counts"] = [int((code == k).sum()) for k in range(8)]
    out["fragile"] = (float(np.abs(E[valid] + 0.5).min()) if valid.any() else np.inf, bend)
    return out


def three(code):
    return np.select([np.isin(code, (7, 4, 3)), np.isin(code, (6, 5))], [2, 1], 0)


def letters(code):
    return "".join(S.SS_CODES[int(c)] for c in code)


def block_of(y, L, native=None):
    """The SS block the library would write for the yardstick's result `y` (and `native`, the native's)."""
    b = np.zeros(S.ss_floats(L), dtype=np.float32)
    b[0] = y["n_hb"]
    b[1:9] = y["counts"]
    b[9], b[10] = y["n_parallel"], y["n_antiparallel"]
    arr = b[32:].reshape(8, L)
    arr[0] = y["ss"]
    arr[1], arr[2], arr[3], arr[4] = y["e_acc"], y["p_acc"], y["e_don"], y["p_don"]
    arr[5], arr[6] = y["bp1"], y["bp2"]
    arr[7] = np.nan
    if native is not None:
        b[11] = 1
        b[12] = int((three(native["ss"]) == three(y["ss"])).sum())
        b[13] = int((native["ss"] == y["ss"]).sum())
        b[14:22] = native["counts"]
        arr[7] = native["ss"]
    return b


# ---- the traces of the known answers -----------------------------------------------------------------------------------------
def ideal_helix(L, radius=2.3, turn=100.0, rise=1.5):
    k = np.arange(L)
    a = np.deg2rad(turn) * k
    return np.stack([radius * np.cos(a), radius * np.sin(a), rise * k], axis=1).astype(np.float32)


def flat_hairpin(n=8, step=3.3, pleat=0.9, apart=4.8, turn=2):
    """Two antiparallel strands of n residues in the plane z = +-pleat, `apart` from each other, `turn` residues between."""
    up = [(step * k, 0.0, pleat * (1 if k % 2 == 0 else -1)) for k in range(n)]
    x_end = step * (n - 1)
    bend = [(x_end + step * 0.75, apart * (t + 1) / (turn + 1), 0.0) for t in range(turn)]
    down = [(step * (n - 1 - k), apart, pleat * (1 if (n - 1 - k) % 2 == 0 else -1)) for k in range(n)]
    return np.asarray(up + bend + down, dtype=np.float32)


def native_3fgx():
    return load_golden("kat_refine_backbone")["ca_in"].astype(np.float32)


NO_PRO = np.zeros(4096, dtype=np.uint8)
FLOOR_3FGX_H, FLOOR_3FGX_E = 40, 8        # about 80 % of what the yardstick gives (test_3fgx_chain_a)


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_ideal_helix_is_all_h_inside():
    y = yardstick(backbone(ideal_helix(24)), NO_PRO)
    print(letters(y["ss"]), y["fragile"], file=sys.stderr)
    assert np.all(y["ss"][1:24 - 2] == 7) and y["ss"][0] != 7
    assert y["n_parallel"] == y["n_antiparallel"] == 0 and np.all(y["bp1"] == -1)
    # the i -> i + 4 bonds: residue i accepts from i + 4
    assert np.all(y["p_acc"][:18] == np.arange(18) + 4) and letters(y["ss"]) == "-" + "H" * 21 + "--"


def test_flat_hairpin_pairs_its_strands():
    y = yardstick(backbone(flat_hairpin()), NO_PRO)
    print(letters(y["ss"]), y["fragile"], file=sys.stderr)
    first, second = list(range(2, 7)), list(range(11, 16))
    assert np.all(y["ss"][first] == 6) and np.all(y["ss"][second] == 6)
    assert all(y["bp1"][i] in range(10, 18) for i in first) and all(y["bp1"][i] in range(0, 8) for i in second)
    assert y["n_antiparallel"] >= 5 and y["n_parallel"] == 0 and y["counts"][7] == 0


def test_3fgx_chain_a():
    """The real 3FGX chain A trace (L = 96) on the oracle-rebuilt backbone: the yardstick gives 51 H and 10 E residues (62 hydrogen
    bonds, 16 '-', 11 S, 8 T), in helices and one hairpin; the floors are about 80 % of that.  Its fragile margins (|E + 0.5| and the
    bend) exceed 1e-4, so the GPU test compares all 96 residues of the native leg."""
    y = yardstick(backbone(native_3fgx()), NO_PRO)
    print(letters(y["ss"]), y["counts"], y["n_hb"], y["fragile"], file=sys.stderr)
    assert y["counts"][7] >= FLOOR_3FGX_H and y["counts"][6] >= FLOOR_3FGX_E
    assert min(y["fragile"]) > 1e-4
    assert (y["counts"][7], y["counts"][6]) == (51, 10)


def test_proline_removes_exactly_that_residues_donated_bonds():
    bb = backbone(ideal_helix(24))
    y0 = yardstick(bb, NO_PRO)
    row = NO_PRO[:24].copy()
    row[10] = 14
    y1 = yardstick(bb, row)
    assert y0["hb"][:, 10].any() and not y1["hb"][:, 10].any()
    rest = np.ones(24, dtype=bool)
    rest[10] = False
    assert np.array_equal(y0["hb"][:, rest], y1["hb"][:, rest])
    assert y1["p_don"][10] == -1 and y1["e_don"][10] == 0.0 and y1["n_hb"] == y0["n_hb"] - int(y0["hb"][:, 10].sum())
    row0 = NO_PRO[:24].copy()
    row0[0] = 14                                            # residue 0 never donates: nothing changes
    assert np.array_equal(yardstick(bb, row0)["hb"], y0["hb"])


# ---- edge cases --------------------------------------------------------------------------------------------------------------
def test_shortest_length():
    y = yardstick(backbone(ideal_helix(8)), NO_PRO)
    assert y["ss"].shape == (8,) and sum(y["counts"]) == 8 and y["p_acc"].shape == (8,)
    assert np.all(y["ss"][1:4] == 7) or y["counts"][7] == 0          # a helix of 8 holds at most Hf on 1 .. L - 2


def test_coincident_atoms_take_the_clamp():
    bb = backbone(ideal_helix(12))
    bb[8, 0] = bb[2, 3]                                     # N of 8 on O of 2: d(O, N) = 0
    y = yardstick(bb, NO_PRO)
    assert y["E"][2, 8] == -9.9 and y["hb"][2, 8] and y["e_acc"][2] == np.float32(-9.9) and y["p_acc"][2] == 8
    assert np.isfinite(y["e_acc"]).all() and np.isfinite(y["e_don"]).all()


def test_a_residue_without_a_hydrogen_direction_does_not_donate():
    bb = backbone(ideal_helix(12))
    bb[5, 3] = bb[5, 2]                                     # O of 5 on C of 5: vv = 0 for residue 6
    y = yardstick(bb, NO_PRO)
    assert not y["valid"][:, 6].any() and y["p_don"][6] == -1 and y["e_don"][6] == 0.0
    assert y["valid"][:, 7].any() and np.isfinite(y["e_acc"]).all()


# ---- the layout --------------------------------------------------------------------------------------------------------------
GRID = list(itertools.product((False, True), (False, True), (False, True), (None, 3, 61), (None, (3, 120)), (None, 11)))


def _lay(L, distmap, score, score_map, align_m, search, passes, **kw):
    return S.Layout(L, distmap, score, score_map and distmap and score, align_m, search, 2048, passes if score else None, **kw)


@pytest.mark.parametrize("L", [8, 96, 2048])
def test_layout_off_is_todays_and_on_moves_what_lies_behind(L):
    names = ("info_off", "score_off", "mapscore_off", "pass_off", "align_off", "align_end", "search_off", "search_end", "total")
    for row in GRID:
        off, on = _lay(L, *row), _lay(L, *row, ss=True)
        assert off.ss is False and off == _lay(L, *row, ss=False) and off != on and on.ss is True
        assert off.ss_off == off.align_off and S.Layout._fields == ("L", "distmap", "score", "score_map", "align_m", "search", "max_L", "passes", "ss", "exposure")
        for name in names:
            moved = 32 + 8 * L if name in ("align_off", "align_end", "search_off", "search_end", "total") else 0
            assert getattr(on, name) - getattr(off, name) == moved, (row, name)
        assert on.ss_off == off.align_off and on.align_off - on.ss_off == S.ss_floats(L) == 32 + 8 * L
        assert on._replace(distmap=on.distmap).ss is True and on._replace(ss=False) == off
        buf = np.arange(on.total, dtype=np.float64)
        got, base = on.split(buf), off.split(buf[:off.total])
        assert base.ss_block is None and got.ss_block.shape == (32 + 8 * L,) and got.ss_block[0] == on.ss_off
        assert np.array_equal(on.ss_block(buf), got.ss_block) and off.ss_block(buf) is None
        for f in S.Outputs._fields[:9]:             # (every part but the two late blocks)
            a, b = getattr(got, f), getattr(base, f)
            assert (a is None) == (b is None)
            if a is not None and f not in ("coords",):
                assert a.size == b.size and a.reshape(-1)[0] - b.reshape(-1)[0] == (32 + 8 * L if f in ("align_block", "search_block") else 0)
        with pytest.raises(ValueError):
            on.split(buf[:-1])


def test_outputs_carry_the_block_beside_the_tuple():
    parts = {name: object() for name in S.Outputs._fields[:9]}
    block = object()
    out = S.Outputs(**parts, ss_block=block)
    assert S.Outputs._fields == ("coords", "confs", "distmap", "info", "score_block", "align_block", "search_block", "map_block", "pass_block",
                                "ss_block", "exposure_block")
    assert S.Outputs(**parts).ss_block is None
    pub = out.public()
    assert len(pub) == 10 and pub[-1] is block and out.public(ss=False) == pub[:-1] == S.Outputs(**parts).public()
    assert out.public(blocks=False) == pub[:4]
    back = S.Outputs.of(pub, True, True, True, True, True, True, ss=True)
    assert back.ss_block is block and all(a is b for a, b in zip(back, out))
    assert out._replace(coords=None).ss_block is block and out._replace(ss_block=None).ss_block is None


# ---- the host side -----------------------------------------------------------------------------------------------------------
def test_unpack_and_json_round_trip():
    L = 96
    y = yardstick(backbone(native_3fgx()), NO_PRO)
    n = yardstick(backbone(ideal_helix(L)), NO_PRO)
    ss = S.unpack_ss(block_of(y, L, n), L)
    assert ss["ss8"] == letters(y["ss"]) and ss["ss8_native"] == letters(n["ss"]) and len(ss["ss3"]) == L
    assert set(ss["ss3"]) <= set("HEC") and ss["ss3"].count("H") == sum(ss["counts"][c] for c in "HGI")
    assert ss["n_hb"] == y["n_hb"] and [ss["counts"][c] for c in S.SS_CODES] == y["counts"]
    assert ss["helix"] + ss["strand"] + ss["coil"] == pytest.approx(1.0) and ss["helix"] == ss["ss3"].count("H") / L
    for k in ("p_acc", "p_don", "bp1", "bp2"):
        assert np.array_equal(ss[k], y[k]) and ss[k].dtype == np.int64
    assert np.array_equal(ss["e_acc"], y["e_acc"]) and np.array_equal(ss["e_don"], y["e_don"])
    assert ss["has_native"] and ss["q8_match"] == int((y["ss"] == n["ss"]).sum()) and ss["q8"] == ss["q8_match"] / L
    assert ss["q3_match"] == sum(a == b for a, b in zip(ss["ss3"], ss["ss3_native"])) and ss["q3"] == ss["q3_match"] / L
    js = json.loads(json.dumps(S.ss_json(ss)))
    assert js["ss8"] == ss["ss8"] and js["q3"] == ss["q3"] and js["counts"] == ss["counts"] and "e_acc" not in js
    full = json.loads(json.dumps(S.ss_json(ss, arrays=True)))
    assert full["bp1"] == [int(v) for v in y["bp1"]] and len(full["e_acc"]) == L
    alone = S.unpack_ss(block_of(y, L), L)
    assert not alone["has_native"] and "q3" not in alone and "ss8_native" not in alone
    nan = S.unpack_ss(np.full(S.ss_floats(L), np.nan, dtype=np.float32), L)
    assert nan["ss8"] == "?" * L and nan["n_hb"] == 0 and np.all(nan["bp1"] == -1) and not nan["has_native"]
    with pytest.raises(ValueError):
        S.unpack_ss(np.zeros(S.ss_floats(L) - 1, dtype=np.float32), L)


# ---- the front ends ----------------------------------------------------------------------------------------------------------
def test_extras_default_and_front_end_arguments():
    from dmpfold2_amd import batch, _lib
    from dmpfold2_amd.predict import dmpfold_parser, Extras
    assert Extras().ss is False and Extras(ss=True).ss is True and Extras._fields == ("distmap", "native", "structure", "library", "score_map", "score_passes", "ss", "exposure")
    assert Extras(ss=True)._replace(distmap=True).ss is True and Extras(True)._replace(ss=True).ss is True
    args = dmpfold_parser().parse_args(["-i", "x.aln", "--ss", "--ss-file", "x.json"])
    assert args.ss is True and args.ss_file == "x.json"
    plain = dmpfold_parser().parse_args(["-i", "x.aln"])
    assert plain.ss is False and plain.ss_file is None
    assert batch.batch_parser().parse_args(["-o", "out", "--ss"]).ss is True
    assert batch.batch_parser().parse_args(["-o", "out"]).ss is False
    assert len(_lib.SIGNATURES) == 65
