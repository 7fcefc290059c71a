"""Host side of option "score_native" (include/dmpfold_hip.h): a prediction scored against a native structure on the GPU.

The library compares the model's C-alpha trace with a native trace that the caller places, one row per alignment column,
in the score block behind the confidences.  This module makes that block from a PDB file - parsing, a global sequence
alignment of the query against the native chain - and takes it apart again.  Nothing here touches the GPU.

The scores are TM-score, GDT_TS / GDT_HA, Kabsch RMSD and lDDT-C-alpha as include/dmpfold_hip.h defines them: the
TM-score program's KIND of search over superpositions, not its bits - any superposition gives a lower bound of the true
maximum, and nobody has compared the values with that program's.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

AA3 = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split()
AA1 = "ARNDCQEGHILKMFPSTWYV"
_THREE_TO_ONE = dict(zip(AA3, AA1))
_THREE_TO_ONE["MSE"] = "M"           # selenomethionine, as structure files of expressed proteins carry it

SCORE_HEADER = 24                    # floats between the native trace and the per-residue arrays
SCORE_NAMES = ("n_pairs", "rmsd", "tm", "gdt_ts", "gdt_ha", "lddt")
COUNT_CUTOFFS = (0.5, 1.0, 2.0, 4.0, 8.0)


def score_floats(L):
    """Floats of the score block of a prediction of length L."""
    return 5 * int(L) + SCORE_HEADER


ALIGN_HEADER = 24                    # floats between m and the per-residue arrays of the align block
ALIGN_NAMES = ("n_ali", "rmsd_ali", "tm_model", "tm_struct", "d0_model", "d0_struct", "seed_offset", "seeds")


def align_floats(L, m):
    """Floats of the align block of a prediction of length L aligned with a structure of m rows."""
    return 1 + ALIGN_HEADER + 2 * int(L) + 3 * int(m)


def conf_floats(L, distmap=False, score=False, align_m=None):
    """Floats the `d_conf` buffer of a prediction of length L must hold: the confidences, the L*L + 3 floats of option
    "emit_distmap", the 5L + 24 floats of option "score_native" and, with `align_m` (the structure's rows; not None), the
    25 + 2L + 3m floats of option "align_structure", in this order."""
    L = int(L)
    return (L + (L * L + 3 if distmap else 0) + (score_floats(L) if score else 0)
            + (align_floats(L, align_m) if align_m is not None else 0))


def align_offset(L, distmap=False, score=False):
    """Where the align block begins in the `d_conf` buffer (A0 of include/dmpfold_hip.h)."""
    return conf_floats(L, distmap, score)


def score_offset(L, distmap=False):
    """Where the score block begins in the `d_conf` buffer (S0 of include/dmpfold_hip.h)."""
    return conf_floats(L, distmap, False)


def distmap_floats(L, on=True):
    """Floats the `d_conf` buffer of a prediction of length L must hold: L, or L + L*L + 3 with option "emit_distmap"."""
    return conf_floats(L, on)


class Outputs(namedtuple("Outputs", "coords confs distmap info score_block align_block", defaults=(None, None, None, None))):
    """What a prediction gives: coords (L, 5, 3), and the parts of its `d_conf` buffer as views of the one allocation -
    confs (L,), with "emit_distmap" distmap (L, L) and info (3,) = [best_pass, passes_run, map_rms], with "score_native"
    score_block (5L + 24,), with "align_structure" align_block (25 + 2L + 3m,) - None for what is absent."""
    __slots__ = ()

    @classmethod
    def of(cls, public, distmap, score, align=False):
        """The inverse of `public` for a caller that knows which options were on."""
        public = tuple(public)
        at = 4 if distmap else 2
        return cls(*public[:2], *(public[2:4] if distmap else (None, None)), public[at] if score else None,
                   public[at + (1 if score else 0)] if align else None)

    def public(self, distmap=True, score=True, align=True):
        """The tuple the public calls return: (coords, confs), then (distmap, info) if present and wanted, then the score
        block if present and wanted, then the align block if present and wanted."""
        return ((self.coords, self.confs) + ((self.distmap, self.info) if distmap and self.distmap is not None else ())
                + ((self.score_block,) if score and self.score_block is not None else ())
                + ((self.align_block,) if align and self.align_block is not None else ()))


def split_conf_buffer(buf, L, emit=False, score=False, coords=None, align_m=None):
    """The parts of a `d_conf` buffer (a 1-D tensor or array of at least conf_floats(L, emit, score, align_m) floats) at the
    offsets of include/dmpfold_hip.h, as the views of an `Outputs` (`coords` is passed through)."""
    L = int(L)
    if buf.ndim != 1 or buf.shape[0] < conf_floats(L, emit, score, align_m):
        raise ValueError(f"a d_conf buffer of length {L} has {conf_floats(L, emit, score, align_m)} floats, got shape {tuple(buf.shape)}")
    s0 = score_offset(L, emit)
    a0 = align_offset(L, emit, score)
    return Outputs(coords, buf[:L], buf[L:L + L * L].reshape(L, L) if emit else None, buf[L + L * L:s0] if emit else None,
                   buf[s0:s0 + score_floats(L)] if score else None,
                   buf[a0:a0 + align_floats(L, align_m)] if align_m is not None else None)


def split_distmap_buffer(buf, L):
    """The three parts of an "emit_distmap" output buffer (a 1-D tensor or array of distmap_floats(L) floats), as views:
    confs (L,), distmap (L, L) and info (3,) = [best_pass, passes_run, map_rms] (include/dmpfold_hip.h)."""
    if buf.ndim != 1 or buf.shape[0] != distmap_floats(L):
        raise ValueError(f"an emit_distmap buffer of length {L} has {distmap_floats(L)} floats, got shape {tuple(buf.shape)}")
    return split_conf_buffer(buf, L, True)[1:4]


def read_native_ca(pdb, chain=None):
    """(ca float32 (n, 3), one-letter sequence) of a chain of a PDB file: ATOM records (and HETATM MSE) with atom name CA,
    fixed columns; the first model only; of alternate locations the first one met per residue.  `chain` None = the chain of
    the first such atom.  A residue name outside the twenty (and MSE) reads as 'X'."""
    xyz, seq, seen = [], [], set()
    with open(pdb, "r") as fh:
        for line in fh:
            rec = line[:6]
            if rec.startswith("ENDMDL"):
                break
            if not (rec == "ATOM  " or (rec == "HETATM" and line[17:20] == "MSE")) or line[12:16] != " CA ":
                continue
            if chain is None:
                chain = line[21]
            if line[21] != chain:
                continue
            key = line[22:27]                               # residue number + insertion code
            if key in seen:
                continue                                    # a further alternate location of the same residue
            seen.add(key)
            xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
            seq.append(_THREE_TO_ONE.get(line[17:20], "X"))
    return np.asarray(xyz, dtype=np.float32).reshape(-1, 3), "".join(seq)


def align_pairs(a, b, match=2, mismatch=-1, gap=-2):
    """Global (Needleman-Wunsch) alignment of two strings with a linear gap penalty; returns [(i, j)] of the aligned
    positions.  Scores and tie-breaking (diagonal, then a gap in `b`, then a gap in `a`) are those of
    tools/accuracy_3fgx.py:needleman_wunsch, so the pair list is the same; the table is filled a row at a time.

    Row i is max(diag, up) followed by the recurrence S[j] = max(T[j], S[j-1] + gap) along the row.  With
    U[j] = S[j] - gap*j that is a running maximum, U[j] = max(T[j] - gap*j, U[j-1]): one np.maximum.accumulate."""
    n, m = len(a), len(b)
    A = np.frombuffer(a.encode("latin-1"), dtype=np.uint8)
    B = np.frombuffer(b.encode("latin-1"), dtype=np.uint8)
    ramp = gap * np.arange(m + 1, dtype=np.int64)
    S = np.empty((n + 1, m + 1), dtype=np.int64)
    S[0] = ramp
    for i in range(1, n + 1):
        prev = S[i - 1]
        T = np.empty(m + 1, dtype=np.int64)
        T[0] = gap * i
        sub = np.where(B == A[i - 1], match, mismatch)
        T[1:] = np.maximum(prev[:-1] + sub, prev[1:] + gap)
        S[i] = np.maximum.accumulate(T - ramp) + ramp
    pairs, i, j = [], n, m
    while i > 0 and j > 0:
        if S[i, j] == S[i - 1, j - 1] + (match if a[i - 1] == b[j - 1] else mismatch):
            pairs.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        elif S[i, j] == S[i - 1, j] + gap:
            i -= 1
        else:
            j -= 1
    return pairs[::-1]


def native_rows(query, native_seq, native_ca):
    """The native trace as the library wants it: (rows float32 (L, 3), lnorm) - row i holds the native C-alpha the
    alignment pairs with query position i, NaN where there is none; lnorm = the native chain's length."""
    native_ca = np.asarray(native_ca, dtype=np.float32).reshape(-1, 3)
    if len(native_seq) != native_ca.shape[0]:
        raise ValueError(f"native sequence has {len(native_seq)} residues, its trace {native_ca.shape[0]}")
    rows = np.full((len(query), 3), np.nan, dtype=np.float32)
    for i, j in align_pairs(query, native_seq):
        rows[i] = native_ca[j]
    return rows, float(len(native_seq))


def native_from_pdb(query, pdb, chain=None):
    """`native_rows` of a PDB file's chain."""
    ca, seq = read_native_ca(pdb, chain)
    if ca.shape[0] == 0:
        raise ValueError(f"{pdb}: no C-alpha atoms" + (f" in chain {chain}" if chain else ""))
    return native_rows(query, seq, ca)


def as_native(native, L):
    """What the front ends accept as `native` -> (rows float32 (L, 3), lnorm float): an (L, 3) array (NaN rows allowed;
    lnorm 0 = the rows present) or a tuple (array, lnorm)."""
    lnorm = 0.0
    if isinstance(native, tuple):
        native, lnorm = native
    rows = np.ascontiguousarray(np.asarray(native, dtype=np.float32))
    if rows.shape != (int(L), 3):
        raise ValueError(f"native must be one row per alignment column, ({int(L)}, 3); got {rows.shape}")
    return rows, float(lnorm)


def pack_native(rows, lnorm, L):
    """The score block (float32 (5L + 24,)) with its two inputs filled in and NaN elsewhere."""
    rows, lnorm = as_native((rows, lnorm), L)
    block = np.full(score_floats(L), np.nan, dtype=np.float32)
    block[:3 * L] = rows.reshape(-1)
    block[3 * L] = lnorm
    return block


def empty_native(L):
    """A score block without any native residue (the library then reports n_pairs = 0 and NaN)."""
    return pack_native(np.full((int(L), 3), np.nan, dtype=np.float32), 0.0, L)


def unpack_scores(block, L):
    """A score block (5L + 24 floats, array or tensor) -> dict: n_pairs (int), rmsd, tm, gdt_ts, gdt_ha, lddt (float),
    counts (5 ints: rows within 0.5, 1, 2, 4, 8 A), R (3, 3) and t (3,) with native ~ R model + t, lddt_res (L,),
    deviation (L,), and the inputs back: lnorm, native (L, 3)."""
    L = int(L)
    b = np.asarray(block.detach().cpu().numpy() if hasattr(block, "detach") else block, dtype=np.float32)
    if b.ndim != 1 or b.shape[0] != score_floats(L):
        raise ValueError(f"a score block of length {L} has {score_floats(L)} floats, got shape {tuple(b.shape)}")
    h = b[3 * L:]
    out = {"n_pairs": int(h[1]) if h[1] == h[1] else 0}
    for k, name in enumerate(SCORE_NAMES[1:]):
        out[name] = float(h[2 + k])
    out["counts"] = [int(v) if v == v else 0 for v in h[7:12]]
    out["R"] = h[12:21].reshape(3, 3).copy()
    out["t"] = h[21:24].copy()
    out["lddt_res"] = b[3 * L + 24:4 * L + 24].copy()
    out["deviation"] = b[4 * L + 24:].copy()
    out["lnorm"] = float(h[0])
    out["native"] = b[:3 * L].reshape(L, 3).copy()
    return out


def scores_json(scores):
    """The scalar part of `unpack_scores` as a JSON-ready dict (what `dmpfold --native` prints and `dmpfold-batch --natives`
    writes); NaN becomes None."""
    def num(v):
        v = float(v)
        return v if v == v else None
    out = {"n_pairs": int(scores["n_pairs"]), "lnorm": num(scores["lnorm"])}
    for name in SCORE_NAMES[1:]:
        out[name] = num(scores[name])
    out["counts"] = [int(c) for c in scores["counts"]]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "align_structure" (include/dmpfold_hip.h): the model aligned with a structure of any length and sequence on the
# GPU - TM-align's KIND of search (gapless threadings, then superposition and dynamic programming in turn), not its
# bits: one family of initial alignments, one gap penalty, 16 refinements.  Any alignment gives a lower bound of the
# best TM-score; nobody has compared the values with that program's.
# ---------------------------------------------------------------------------------------------------------------------
def as_structure(ca):
    """What the front ends accept as `structure` -> float32 (m, 3), contiguous."""
    ca = np.ascontiguousarray(np.asarray(ca, dtype=np.float32))
    if ca.ndim != 2 or ca.shape[1] != 3:
        raise ValueError(f"structure must be a C-alpha trace (m, 3); got {ca.shape}")
    return ca


def pack_structure(ca, L, m_value=None):
    """The align block (float32 (25 + 2L + 3m,)) with its two inputs filled in - m in front, the trace at the end - and NaN
    in the out slots.  `m_value`: what to write as m instead of the trace's length (tests of the library's validation)."""
    ca = as_structure(ca)
    m, L = ca.shape[0], int(L)
    block = np.full(align_floats(L, m), np.nan, dtype=np.float32)
    block[0] = float(m if m_value is None else m_value)
    block[1 + ALIGN_HEADER + 2 * L:] = ca.reshape(-1)
    return block


def empty_structure(L):
    """An align block without a structure: m = 0, which the library answers with NaN in every out slot."""
    return pack_structure(np.zeros((0, 3), dtype=np.float32), L)


def unpack_alignment(block, L):
    """An align block (array or tensor) -> dict: n_ali (int), rmsd_ali, tm_model, tm_struct, d0_model, d0_struct (float),
    seed_offset, seeds (int), R (3, 3) and t (3,) with structure ~ R model + t, ali (L,) int - the structure's row aligned
    with model residue i, or -1 -, deviation (L,), and the inputs back: m, structure (m, 3).  A block the library answered
    with NaN (a bad m, a NaN coordinate, a fault) gives n_ali 0, NaN floats and ali all -1."""
    L = int(L)
    b = np.asarray(block.detach().cpu().numpy() if hasattr(block, "detach") else block, dtype=np.float32)
    m = (b.shape[0] - (1 + ALIGN_HEADER + 2 * L)) // 3 if b.ndim == 1 else -1
    if m < 0 or b.shape[0] != align_floats(L, m):
        raise ValueError(f"an align block of length {L} has 25 + 2L + 3m floats, got shape {tuple(b.shape)}")
    h = b[1:1 + ALIGN_HEADER]

    def whole(v):
        return int(v) if v == v else 0
    out = {"n_ali": whole(h[0]), "rmsd_ali": float(h[1]), "tm_model": float(h[2]), "tm_struct": float(h[3]),
           "R": h[4:13].reshape(3, 3).copy(), "t": h[13:16].copy(), "d0_model": float(h[16]), "d0_struct": float(h[17]),
           "seed_offset": whole(h[18]), "seeds": whole(h[19])}
    ali = b[1 + ALIGN_HEADER:1 + ALIGN_HEADER + L]
    out["ali"] = np.where(ali == ali, ali, -1.0).astype(np.int64)
    out["deviation"] = b[1 + ALIGN_HEADER + L:1 + ALIGN_HEADER + 2 * L].copy()
    out["m"] = float(b[0])
    out["structure"] = b[1 + ALIGN_HEADER + 2 * L:].reshape(m, 3).copy()
    return out


def alignment_json(al):
    """`unpack_alignment` as a JSON-ready dict (what `dmpfold --compare` prints and `dmpfold-batch --structures` writes):
    the header fields, R, t and ali; NaN becomes None."""
    def num(v):
        v = float(v)
        return v if v == v else None
    out = {"m": num(al["m"])}
    for name in ALIGN_NAMES:
        out[name] = int(al[name]) if name in ("n_ali", "seed_offset", "seeds") else num(al[name])
    out["R"] = [[num(v) for v in row] for row in np.asarray(al["R"])]
    out["t"] = [num(v) for v in np.asarray(al["t"])]
    out["ali"] = [int(v) for v in al["ali"]]
    return out
