"""Host side of option "score_native" (dmpfold2_amd/score.py) and the yardstick the GPU tests compare with.

The yardstick is a float64 NumPy restatement of the scores as include/dmpfold_hip.h defines them (the reference has none
of them).  Besides the values it returns the smallest |value - cutoff| it met at any comparison - d_cut, the five count
cutoffs, the lDDT radius and its thresholds: two float64 evaluations of the same formula differ by about 1e-13, so with a
margin of 1e-9 Angstrom or more every set and every integer count is the same on both sides.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

from dmpfold2_amd import score as S

CUTS = (0.5, 1.0, 2.0, 4.0, 8.0)
NEAR_TIE = 1e-9


def _tool():
    spec = importlib.util.spec_from_file_location("accuracy_3fgx", os.path.join(ROOT, "tools", "accuracy_3fgx.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the yardstick
def seed_fragments(n):
    """[(start, length)] in seed order: the distinct lengths f_0 = n, f_k = max(n >> k, min(4, n)), every start."""
    lens = []
    for k in range(6):
        f = n if k == 0 else max(n >> k, min(4, n))
        if f not in lens:
            lens.append(f)
    return [(s, f) for f in lens for s in range(n - f + 1)]


def _kabsch(P, Q):
    pc, qc = P.mean(0), Q.mean(0)
    H = (P - pc).T @ (Q - qc)
    U, _, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, qc - R @ pc


def _dev(R, t, P, Q):
    e = P @ R.T + t - Q
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def _pairdist(X):
    d = X[:, None, :] - X[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def yardstick(model, native, lnorm=0.0):
    """(scores, margin): `scores` has the keys of score.unpack_scores in float64 / int, `margin` is the smallest distance
    of any compared value from its cutoff.  `model` (L, 3) float32, `native` (L, 3) float32 with NaN rows."""
    model = np.asarray(model, dtype=np.float32)
    native = np.asarray(native, dtype=np.float32)
    L = model.shape[0]
    present = ~np.isnan(native[:, 0])
    idx = np.nonzero(present)[0]
    n = int(present.sum())
    nan = float("nan")
    out = {"n_pairs": n, "rmsd": nan, "tm": nan, "gdt_ts": nan, "gdt_ha": nan, "lddt": nan, "counts": [nan] * 5,
           "R": np.full((3, 3), nan), "t": np.full(3, nan), "lddt_res": np.full(L, nan), "deviation": np.full(L, nan)}
    if n < 3:
        return out, float("inf")
    P = model[idx].astype(np.float64)
    Q = native[idx].astype(np.float64)
    lnorm = float(np.float32(lnorm))
    if lnorm == 0.0:
        lnorm = float(n)
    d0 = max(1.24 * float(np.cbrt(lnorm - 15.0)) - 1.8, 0.5) if lnorm > 15 else 0.5
    d_cut = min(max(d0, 4.5), 8.0)
    margin = float("inf")
    best_tm, best_Rt, best_cnt, rmsd = -1.0, None, [0] * 5, nan
    for seed, (start, frag) in enumerate(seed_fragments(n)):
        sel = np.zeros(n, dtype=bool)
        sel[start:start + frag] = True
        for it in range(20):
            R, t = _kabsch(P[sel], Q[sel])
            d = _dev(R, t, P, Q)
            margin = min(margin, float(np.abs(d - d_cut).min()), min(float(np.abs(d - c).min()) for c in CUTS))
            tm = float((1.0 / (1.0 + (d / d0) * (d / d0))).sum() / lnorm)
            if tm > best_tm:                                   # strict: ties stay with the lowest seed, the earliest iteration
                best_tm, best_Rt = tm, (R, t)
            for c, cut in enumerate(CUTS):
                best_cnt[c] = max(best_cnt[c], int((d < cut).sum()))
            if seed == 0 and it == 0:
                rmsd = float(np.sqrt((d * d).sum() / n))
            new = d < d_cut
            if int(new.sum()) < 3 or bool((new == sel).all()):
                break
            sel = new
    R, t = best_Rt
    out.update(rmsd=rmsd, tm=best_tm, counts=best_cnt, R=R, t=t)
    out["gdt_ts"] = (best_cnt[1] + best_cnt[2] + best_cnt[3] + best_cnt[4]) / 4.0 / lnorm
    out["gdt_ha"] = (best_cnt[0] + best_cnt[1] + best_cnt[2] + best_cnt[3]) / 4.0 / lnorm
    out["deviation"][idx] = _dev(R, t, P, Q)
    # lDDT-C-alpha from integer counts
    dn, dm = _pairdist(Q), _pairdist(P)
    off = ~np.eye(n, dtype=bool)
    margin = min(margin, float(np.abs(dn - 15.0)[off].min()))
    near = (dn < 15.0) & off
    e = np.abs(dm - dn)
    pres = np.zeros(n, dtype=np.int64)
    for tau in (0.5, 1.0, 2.0, 4.0):
        if near.any():
            margin = min(margin, float(np.abs(e - tau)[near].min()))
        pres += ((e < tau) & near).sum(1)
    part = near.sum(1)
    res = np.zeros(n)
    res[part > 0] = pres[part > 0] / (4.0 * part[part > 0])
    out["lddt_res"][idx] = res
    out["lddt"] = float(pres.sum() / (4.0 * part.sum())) if part.sum() > 0 else 0.0
    return out, margin


def ulp32(x):
    """Spacing of float32 at x (an array of float64 or float32 values)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def compare_with_yardstick(got, want, margin, tag=""):
    """`got`: score.unpack_scores of the library's block; `want`, `margin`: yardstick().  The integer-derived outputs must
    equal float32(yardstick) exactly; tm, rmsd, R, t and the deviations lie within 1 float32 ulp of float32(yardstick)
    (entries of R within 1e-6 of zero: within 1e-6 absolute) - both sides are float64, about 1e-13 apart, so only the
    final rounding can differ.  Returns the largest differences seen, in ulps, for the record."""
    if not margin >= NEAR_TIE:
        pytest.fail(f"{tag}: near tie (margin {margin:.3e} A), choose another seed")
    seen = {}
    assert got["n_pairs"] == want["n_pairs"], (tag, got["n_pairs"], want["n_pairs"])
    assert list(got["counts"]) == [int(c) for c in want["counts"]], (tag, got["counts"], want["counts"])
    for name in ("gdt_ts", "gdt_ha", "lddt"):
        assert np.float32(got[name]) == np.float32(want[name]), (tag, name, got[name], want[name])
    w = np.asarray(want["lddt_res"], dtype=np.float64).astype(np.float32)
    assert np.array_equal(np.asarray(got["lddt_res"], dtype=np.float32), w, equal_nan=True), (tag, "lddt_res")
    for name in ("tm", "rmsd", "R", "t", "deviation"):
        g = np.asarray(got[name], dtype=np.float32).astype(np.float64).reshape(-1)
        w = np.asarray(want[name], dtype=np.float64).reshape(-1).astype(np.float32).astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, name, "NaN pattern")
        ok = ~np.isnan(w)
        diff = np.abs(g[ok] - w[ok])
        ulps = diff / ulp32(w[ok])
        fine = ulps <= 1.0
        if name == "R":
            fine |= (np.abs(w[ok]) <= 1e-6) & (diff <= 1e-6)
        seen[name] = float(ulps[np.abs(w[ok]) > 1e-6].max()) if (np.abs(w[ok]) > 1e-6).any() else 0.0
        assert bool(fine.all()), (tag, name, "max ulps", float(ulps.max()), "max abs", float(diff.max()))
    return seen


# ------------------------------------------------------------------------------------------------ native parsing
def _atom(serial, name, alt, res, chain, num, xyz, rec="ATOM"):
    return "%-6s%5d %-4s%1s%3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00\n" % (rec, serial, name, alt, res, chain, num, *xyz)


def _pdb(tmp_path):
    """Chain A: ALA 1, GLY 2 (two alternate locations), residue 3 missing, LEU 4, MSE 5 (HETATM); chain B: TRP 1;
    a second model that must not be read."""
    lines = ["MODEL        1\n"]
    lines.append(_atom(1, " N  ", " ", "ALA", "A", 1, (0.0, 0.0, 0.0)))
    lines.append(_atom(2, " CA ", " ", "ALA", "A", 1, (1.0, 2.0, 3.0)))
    lines.append(_atom(3, " CA ", "A", "GLY", "A", 2, (4.0, 5.0, 6.0)))
    lines.append(_atom(4, " CA ", "B", "GLY", "A", 2, (4.5, 5.5, 6.5)))
    lines.append(_atom(5, " CA ", " ", "LEU", "A", 4, (7.0, 8.0, 9.0)))
    lines.append(_atom(6, " CA ", " ", "MSE", "A", 5, (10.0, 11.0, 12.0), rec="HETATM"))
    lines.append(_atom(7, " CA ", " ", "TRP", "B", 1, (-1.0, -2.0, -3.0)))
    lines.append(_atom(8, "CA  ", " ", " CA", "B", 2, (9.0, 9.0, 9.0), rec="HETATM"))       # a calcium ion, not a C-alpha
    lines += ["ENDMDL\n", "MODEL        2\n", _atom(9, " CA ", " ", "ALA", "A", 1, (99.0, 99.0, 99.0)), "ENDMDL\n"]
    p = tmp_path / "native.pdb"
    p.write_text("".join(lines))
    return str(p)


def test_read_native_ca_chains_altlocs_models(tmp_path):
    p = _pdb(tmp_path)
    ca, seq = S.read_native_ca(p)
    assert seq == "AGLM" and ca.dtype == np.float32
    assert np.array_equal(ca, np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], dtype=np.float32))
    ca_a, seq_a = S.read_native_ca(p, "A")
    assert seq_a == seq and np.array_equal(ca_a, ca)
    ca_b, seq_b = S.read_native_ca(p, "B")
    assert seq_b == "W" and np.array_equal(ca_b, np.array([[-1, -2, -3]], dtype=np.float32))
    assert S.read_native_ca(p, "C")[0].shape == (0, 3)
    with pytest.raises(ValueError):
        S.native_from_pdb("AGSLM", p, "C")


def test_native_rows_gap_and_mutation(tmp_path):
    """The query has the residue the structure lacks (a NaN row) and differs from it in one letter (still paired)."""
    p = _pdb(tmp_path)
    rows, lnorm = S.native_from_pdb("AGSLM", p)
    assert lnorm == 4.0 and rows.dtype == np.float32 and rows.shape == (5, 3)
    assert np.isnan(rows[2]).all() and not np.isnan(rows[[0, 1, 3, 4]]).any()
    assert np.array_equal(rows[3], np.array([7, 8, 9], dtype=np.float32))
    rows_m, _ = S.native_from_pdb("AGSIM", p)                          # L -> I: a mutation, paired all the same
    assert np.array_equal(rows_m, rows, equal_nan=True)
    with pytest.raises(ValueError):
        S.native_rows("AG", "AGL", np.zeros((2, 3), dtype=np.float32))


# ------------------------------------------------------------------------------------------------ alignment
def _native_3fgx():
    nat = load_golden("kat_refine_backbone")
    return nat["ca_in"].astype(np.float32), bytes(nat["seq1"]).decode()


def _query_pf10963():
    with open(os.path.join(ROOT, "tests", "golden", "PF10963.aln")) as fh:
        return fh.readline().rstrip()


def test_alignment_equals_the_tools_pair_list():
    tool = _tool()
    _, seq = _native_3fgx()
    query = _query_pf10963()
    cases = [(query, seq), (seq, query),
             ("ACDEFGHIK", "DEFGHIKLMN"),          # gaps at the start of one, the end of the other
             ("MMMACDEFG", "ACDEFGWWW"),
             ("ACDEFG", "WWACDKEFGYY"),            # an insertion in the middle, overhangs at both ends
             ("A", "CCCC"), ("AAAA", "AA")]
    for a, b in cases:
        assert S.align_pairs(a, b) == tool.needleman_wunsch(a, b), (a, b)
    assert len(S.align_pairs(query, seq)) > 60


def test_alignment_is_row_vectorised_at_full_length():
    """2048 x 2048 in well under the seconds a cell-by-cell Python loop takes (4 M cells)."""
    import time
    rng = np.random.default_rng(5)
    a = "".join(rng.choice(list(S.AA1), 2048))
    b = a[:700] + a[760:1500] + "".join(rng.choice(list(S.AA1), 40)) + a[1500:]
    t0 = time.perf_counter()
    pairs = S.align_pairs(a, b)
    dt = time.perf_counter() - t0
    assert len(pairs) >= 1900 and all(a[i] == b[j] for i, j in pairs[:700])
    assert dt < 2.0, dt


# ------------------------------------------------------------------------------------------------ layout
def test_block_layout_and_conf_floats():
    assert S.conf_floats(96) == 96
    assert S.conf_floats(96, distmap=True) == 96 + 96 * 96 + 3
    assert S.conf_floats(96, score=True) == 96 + 5 * 96 + 24
    assert S.conf_floats(96, True, True) == 96 + 96 * 96 + 3 + 5 * 96 + 24
    assert S.score_offset(96) == 96 and S.score_offset(96, True) == 96 + 96 * 96 + 3
    assert S.score_floats(8) == 64
    rows = np.arange(24, dtype=np.float32).reshape(8, 3)
    rows[3] = np.nan
    blk = S.pack_native(rows, 12.0, 8)
    assert blk.shape == (64,) and blk.dtype == np.float32
    assert np.array_equal(blk[:24].reshape(8, 3), rows, equal_nan=True) and blk[24] == 12.0 and np.isnan(blk[25:]).all()
    assert np.isnan(S.empty_native(8)[:24]).all() and S.empty_native(8)[24] == 0.0
    r, ln = S.as_native(rows, 8)
    assert ln == 0.0 and np.array_equal(r, rows, equal_nan=True)
    assert S.as_native((rows, 7), 8)[1] == 7.0
    with pytest.raises(ValueError):
        S.as_native(rows, 9)
    with pytest.raises(ValueError):
        S.unpack_scores(np.zeros(63, dtype=np.float32), 8)


def test_unpack_scores_round_trip():
    L = 8
    blk = np.arange(S.score_floats(L), dtype=np.float32) + 0.5
    blk[3 * L + 1] = 7.0
    blk[3 * L + 7:3 * L + 12] = [1, 2, 3, 4, 5]
    sc = S.unpack_scores(blk, L)
    assert sc["lnorm"] == blk[3 * L] and sc["n_pairs"] == 7
    for k, name in enumerate(("rmsd", "tm", "gdt_ts", "gdt_ha", "lddt")):
        assert sc[name] == float(blk[3 * L + 2 + k])
    assert sc["counts"] == [1, 2, 3, 4, 5]
    assert np.array_equal(sc["R"].reshape(-1), blk[3 * L + 12:3 * L + 21]) and np.array_equal(sc["t"], blk[3 * L + 21:3 * L + 24])
    assert np.array_equal(sc["lddt_res"], blk[3 * L + 24:4 * L + 24]) and np.array_equal(sc["deviation"], blk[4 * L + 24:])
    assert np.array_equal(sc["native"].reshape(-1), blk[:3 * L])
    # the same from a tensor
    import torch
    sc_t = S.unpack_scores(torch.from_numpy(blk), L)
    assert sc_t["tm"] == sc["tm"] and np.array_equal(sc_t["deviation"], sc["deviation"])
    js = S.scores_json(sc)
    assert js["n_pairs"] == 7 and js["counts"] == [1, 2, 3, 4, 5] and js["tm"] == sc["tm"]
    blk[3 * L + 3] = np.nan
    assert S.scores_json(S.unpack_scores(blk, L))["tm"] is None


# ------------------------------------------------------------------------------------------------ yardstick sanity
def _rotation(seed):
    q = np.random.default_rng(seed).normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def test_seed_fragments():
    assert seed_fragments(3) == [(0, 3)]
    assert seed_fragments(4) == [(0, 4)]
    assert seed_fragments(8) == [(0, 8)] + [(s, 4) for s in range(5)]
    assert len(seed_fragments(96)) == 1 + 49 + 73 + 85 + 91 + 93 and len(seed_fragments(2048)) == 8262
    assert all(len(seed_fragments(n)) <= 1 + 5 * n for n in range(3, 300))


def test_yardstick_rigid_copy_gives_one():
    """A rigidly moved copy in float64: TM = 1 within 1e-12 (the yardstick rounds its inputs to float32, so the copy is made
    from coordinates that survive it: a quarter turn about z and an integer shift)."""
    ca, _ = _native_3fgx()
    model = np.round(ca * 8) / 8
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    native = (model.astype(np.float64) @ R.T + np.array([3.0, -5.0, 7.0])).astype(np.float32)
    sc, _ = yardstick(model, native)
    assert abs(sc["tm"] - 1.0) < 1e-12 and sc["rmsd"] < 1e-12 and sc["lddt"] == 1.0
    assert sc["counts"] == [len(ca)] * 5 and sc["gdt_ts"] == 1.0 and sc["gdt_ha"] == 1.0
    assert np.abs(sc["R"] - R).max() < 1e-12 and np.abs(sc["t"] - [3.0, -5.0, 7.0]).max() < 1e-10


def test_yardstick_not_below_the_tools_reduced_search():
    """3FGX against a perturbed copy: the tool's seeds are a subset of the yardstick's (n >= 4, d0 <= 8)."""
    tool = _tool()
    ca, _ = _native_3fgx()
    rng = np.random.default_rng(11)
    model = (ca.astype(np.float64) @ _rotation(2).T + 4.0 + rng.normal(scale=1.5, size=ca.shape)).astype(np.float32)
    model[20:35] += np.float32(9.0)
    for lnorm in (float(len(ca)), 60.0):
        sc, margin = yardstick(model, ca, lnorm)
        assert margin > 0
        want = tool.tm_score(model.astype(np.float64), ca.astype(np.float64), lnorm)
        assert sc["tm"] >= want - 1e-12, (sc["tm"], want)
        assert 0.2 < sc["tm"] < 1.0 and 0.0 < sc["lddt"] < 1.0 and sc["rmsd"] > 1.0
    nat = ca.copy()
    nat[::7] = np.nan
    sc, _ = yardstick(model, nat)
    assert sc["n_pairs"] == int((~np.isnan(nat[:, 0])).sum())
    assert np.isnan(sc["deviation"][::7]).all() and np.isnan(sc["lddt_res"][::7]).all()
    assert not np.isnan(np.delete(sc["deviation"], np.arange(0, len(ca), 7))).any()
    few = np.full_like(ca, np.nan)
    few[:2] = ca[:2]
    sc, _ = yardstick(model, few)
    assert sc["n_pairs"] == 2 and np.isnan(sc["tm"]) and np.isnan(sc["R"]).all()


def test_abi_is_unchanged():
    from dmpfold2_amd import _lib
    assert len(_lib.SIGNATURES) == 65 and _lib.ABI_VERSION == 5
