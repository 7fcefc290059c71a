"""Host side of option "score_native" (include/dmpfold_hip.h): a prediction scored against a native structure on the GPU.

The library compares the model's C-alpha trace with a native trace that the caller places, one row per alignment column,
in the score block behind the confidences.  This module makes that block from a PDB file - parsing, a global sequence
alignment of the query against the native chain - and takes it apart again.  Nothing here touches the GPU.

`Layout` is the one Python statement of where each block lies in that buffer (the twin of conf_layout() in csrc/common.h);
conf_floats, score_offset, mapscore_offset, align_offset, search_offset and split_conf_buffer are views of it.

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


def _num(v):
    """A float for JSON: NaN becomes None."""
    v = float(v)
    return v if v == v else None


def _whole(v):
    """A count the library wrote as a float: NaN (a block it answered with NaN) reads as 0."""
    return int(v) if v == v else 0


def _host(block):
    """A block (array, or tensor on any device) as a float32 array on the host."""
    return np.asarray(block.detach().cpu().numpy() if hasattr(block, "detach") else block, dtype=np.float32)


def score_floats(L):
    """Floats of the score block of a prediction of length L."""
    return 5 * int(L) + SCORE_HEADER


ALIGN_HEADER = 24                    # floats between m and the per-residue arrays of the align block
ALIGN_NAMES = ("n_ali", "rmsd_ali", "tm_model", "tm_struct", "d0_model", "d0_struct", "seed_offset", "seeds")


def align_floats(L, m):
    """Floats of the align block of a prediction of length L aligned with a structure of m rows."""
    return 1 + ALIGN_HEADER + 2 * int(L) + 3 * int(m)


MAPSCORE_HEADER = 64                 # floats in front of the per-residue array of the map-score block


def mapscore_floats(L):
    """Floats of the map-score block (option "score_map") of a prediction of length L."""
    return MAPSCORE_HEADER + int(L)


PASS_HEADER = 16                     # floats in front of the rows of the pass block
PASS_ROW = 8                         # floats of a row
PASS_MAX = 128                       # the context's max_passes: later passes have no recorded trace
PASS_COLUMNS = ("conf_mean", "delta", "tm", "gdt_ts", "gdt_ha", "rmsd", "lddt")
PASS_FIELDS = ("rows", "best_pass", "tm_pass", "lddt_pass", "regret_tm", "regret_lddt")


def pass_rows(iterations):
    """R of the pass block of a prediction asked for `iterations` recycling passes: min(iterations + 1, 128)."""
    return min(max(int(iterations), 0) + 1, PASS_MAX)


def pass_floats(R):
    """Floats of the pass block (option "score_passes") of R rows."""
    return PASS_HEADER + PASS_ROW * int(R)


SS_HEADER = 32                       # floats in front of the per-residue arrays of the SS block
SS_ARRAYS = 8                        # per-residue arrays of L floats behind it
SS_CODES = "-STIGBEH"                # code 0 .. 7 of a residue -> its letter
SS_THREE = "CCCHHEEH"                # ... -> its three-state letter: helix (H, G, I), strand (E, B), coil (the rest)


def ss_floats(L):
    """Floats of the SS block (option "assign_ss") of a prediction of length L."""
    return SS_HEADER + SS_ARRAYS * int(L)


EXPOSURE_HEADER = 32                 # floats in front of the per-residue arrays of the exposure block
EXPOSURE_ARRAYS = 16                 # per-residue arrays of L floats behind it: eight of the model, eight of the native
EXPOSURE_POINTS = 256                # sphere points per atom
EXPOSURE_ATOMS = ("N", "CA", "C", "O", "CB")
EXPOSURE_RADII = (3.05, 3.27, 3.16, 2.80, 3.20)     # atom radius + the 1.4 A probe (Kabsch & Sander 1983)
HYDROPHOBIC = "AVILMFWC"


def exposure_floats(L):
    """Floats of the exposure block (option "exposure") of a prediction of length L."""
    return EXPOSURE_HEADER + EXPOSURE_ARRAYS * int(L)


DOMAINS_HEADER = 32                  # floats in front of the labels of the domain block: sixteen of the model, sixteen of the native
DOMAINS_MAX = 16                     # rows of a leg's table: four levels of bisection
DOMAINS_ROW = 8                      # floats of a row
DOMAINS_FIELDS = ("domains", "contacts", "tau_milli", "min_size", "min_segment", "discontinuous", "depth", "unexamined")
DOMAINS_COLUMNS = ("size", "segments", "first", "contacts", "contacts_out", "cut_ext", "cut_den", "level")


def domains_floats(L):
    """Floats of the domain block (option "domains") of a prediction of length L."""
    return DOMAINS_HEADER + 2 * int(L) + 2 * DOMAINS_MAX * DOMAINS_ROW


class Layout(namedtuple("Layout", "L distmap score score_map align_m search max_L passes ss exposure",
                        defaults=(False, False, False, None, None, None, None, False, False))):
    """Where everything lies in the `d_conf` buffer of a prediction of length L: the Python twin of ConfLayout / conf_layout()
    / search_base() of csrc/common.h, in the order of include/dmpfold_hip.h.  Made from what decides it - `distmap`, `score`,
    `score_map`, `ss`, `exposure`, `domains`: options "emit_distmap", "score_native", "score_map", "assign_ss", "exposure",
    "domains" on (`domains` is an attribute beside the ten fields, which callers unpack by position); `align_m`:
    the m the align block holds (None = "align_structure" off); `search`: (K, M) of option "search_structures" (None = off);
    `max_L`: the context's, for the rule of B0 (None: whatever the align block's writer allocated, i.e. any whole m >= 0
    counts); `passes`: the rows R of the pass block of option "score_passes" (None = off).  The confidences, the map and its
    info lie in front; behind them the blocks of BLOCKS that are on, each where the one in front of it ends:

      [0, L) confidences | L: map (L*L), info (3) | score_off (S0): score block (5L + 24) | mapscore_off (M0): map-score block
      (64 + L) | pass_off (T0): pass block (16 + 8R) | ss_off (U0): SS block (32 + 8L) | exposure_off (X0): exposure block (32 + 16L) |
      domains_off (D0): domain block (32 + 2L + 256) | domain_search_off: domain-search block ((400 + 2L) K, with `search_domains`) | domain_score_off: domain-score block (1040 + 4L, with `score_domains`) | align_off (A0): align block (25 + 2L + 3m) | align_end | search_off (B0): search block (26K + 2LK + 3M)

    and `total` is the floats the buffer must hold.  `search_domains` (option "search_domains" on; an attribute beside the
    fields, like `domains`) puts the domain-search block, sized from the K of `search`, between the domain block and the
    align block; `score_domains` (option "score_domains" on; an attribute likewise) puts the domain-score block behind that, in
    front of the align block; `flex` (option "flex" on; an attribute likewise) puts the flex block (48 + 20L, at `flex_off`)
    behind that, in front of the align block; `msa_report` (option "msa_report": 0, 1 or 2; an attribute likewise) puts the
    report block (128 + 8L, with 2 + L*L, at `msa_report_off`) behind that, in front of the align block."""

    def __new__(cls, L, distmap=False, score=False, score_map=False, align_m=None, search=None, max_L=None, passes=None,
                ss=False, exposure=False, domains=False, search_domains=False, score_domains=False, flex=False, msa_report=0):
        self = super().__new__(cls, int(L), bool(distmap), bool(score), bool(score_map), align_m,
                               None if search is None else (int(search[0]), int(search[1])), max_L,
                               None if passes is None else int(passes), bool(ss), bool(exposure))
        self.domains = bool(domains)
        self.search_domains = bool(search_domains)
        self.score_domains = bool(score_domains)
        self.flex = bool(flex)
        self.msa_report = int(msa_report)
        return self

    domains = False                  # (of a Layout made by `_make`)
    search_domains = False
    score_domains = False
    flex = False
    msa_report = 0

    def _replace(self, **changes):
        domains = changes.pop("domains", self.domains)
        search_domains = changes.pop("search_domains", self.search_domains)
        score_domains = changes.pop("score_domains", self.score_domains)
        flex = changes.pop("flex", self.flex)
        msa_report = changes.pop("msa_report", self.msa_report)
        new = super()._replace(**changes)
        new.flex = bool(flex)
        new.msa_report = int(msa_report)
        new.domains = bool(domains)
        new.search_domains = bool(search_domains)
        new.score_domains = bool(score_domains)
        return new

    def floats(self, row):
        """The floats a row of BLOCKS takes in this buffer: 0 where its block is off."""
        if row is DOMAIN_SEARCH:
            return domain_search_floats(self.L, self.search[0]) if self.search_domains and self.search is not None else 0
        if row is DOMAIN_SCORES:
            return domain_score_floats(self.L) if self.score_domains else 0
        if row is FLEX:
            return flex_floats(self.L) if self.flex else 0
        if row is MSA_REPORT:
            return msa_report_floats(self.L, self.msa_report == 2) if self.msa_report else 0
        value = getattr(self, row.arg)
        return 0 if value is None or value is False else row.floats(self.L, value)

    def _walk(self):
        """(row, where its block begins) of every block up to the align block, then (None, where that ends): one running sum.
        A block's size is asked for only when the walk goes on behind it (an align_m that is no number raises ValueError there)."""
        at = self.score_off
        for row in BLOCKS[:-1]:
            yield row, at
            at += self.floats(row)
            if row.key == "domains" and self.floats(DOMAIN_SEARCH):      # (no row of BLOCKS: see DOMAIN_SEARCH)
                yield DOMAIN_SEARCH, at
                at += self.floats(DOMAIN_SEARCH)
            if row.key == "domains" and self.floats(DOMAIN_SCORES):      # (likewise: see DOMAIN_SCORES)
                yield DOMAIN_SCORES, at
                at += self.floats(DOMAIN_SCORES)
            if row.key == "domains" and self.floats(FLEX):               # (likewise: see FLEX)
                yield FLEX, at
                at += self.floats(FLEX)
            if row.key == "domains" and self.floats(MSA_REPORT):         # (likewise: see MSA_REPORT)
                yield MSA_REPORT, at
                at += self.floats(MSA_REPORT)
        yield None, at

    def _begin(self, key):
        return next(at for row, at in self._walk() if row is None or row.key == key)

    info_off = property(lambda s: s.L + (s.L * s.L if s.distmap else 0))
    score_off = property(lambda s: s.info_off + (3 if s.distmap else 0))                                    # S0
    mapscore_off = property(lambda s: s._begin("score_map"))                                                # M0
    pass_off = property(lambda s: s._begin("passes"))                                                       # T0
    ss_off = property(lambda s: s._begin("ss"))                                                             # U0
    exposure_off = property(lambda s: s._begin("exposure"))                                                 # X0
    domains_off = property(lambda s: s._begin("domains"))                                                   # D0
    domain_search_off = property(lambda s: s.domains_off + s.floats(BLOCK["domains"]))
    domain_score_off = property(lambda s: s.domain_search_off + s.floats(DOMAIN_SEARCH))
    flex_off = property(lambda s: s.domain_score_off + s.floats(DOMAIN_SCORES))
    msa_report_off = property(lambda s: s.flex_off + s.floats(FLEX))                                        # Q0
    align_off = property(lambda s: s._begin("align"))                                                       # A0
    # the end of the align block as its writer allocated it ...
    align_end = property(lambda s: s._begin(None))
    # ... and B0, its end as the library counts it: 3m of it only if m is an integer in [3, max_L]
    search_off = property(lambda s: s.align_end if s.align_m is None or s.max_L is None
                          else s.align_off + align_floats(s.L, align_m_rule(s.align_m, s.max_L)))
    search_end = property(lambda s: s.search_off + s.floats(BLOCK["search"]))
    # the search block may begin inside what the align block's writer allocated: the buffer holds the larger of the two
    total = property(lambda s: s.align_end if s.search is None else max(s.align_end, s.search_end))

    def split(self, buf, coords=None):
        """The parts of a `d_conf` buffer (a 1-D tensor or array of at least `total` floats) as the views of an `Outputs`
        (`coords` is passed through)."""
        L = self.L
        if buf.ndim != 1 or buf.shape[0] < self.total:
            raise ValueError(f"a d_conf buffer of length {L} has {self.total} floats, got shape {tuple(buf.shape)}")
        marks = list(self._walk())
        parts = {row.field: buf[at:end] for (row, at), (_, end) in zip(marks, marks[1:]) if end > at}
        if self.distmap:
            parts.update(distmap=buf[L:self.info_off].reshape(L, L), info=buf[self.info_off:self.score_off])
        if self.search is not None:
            parts["search_block"] = buf[self.search_off:self.search_end]
        return Outputs(coords, buf[:L], **parts)

    def _view(self, key, buf):
        at, floats = self._begin(key), self.floats(BLOCK[key])
        return buf[at:at + floats] if floats else None

    def ss_block(self, buf):
        """The SS block of a `d_conf` buffer as a view (32 + 8L floats), None with `ss` off."""
        return self._view("ss", buf)

    def exposure_block(self, buf):
        """The exposure block of a `d_conf` buffer as a view (32 + 16L floats), None with `exposure` off."""
        return self._view("exposure", buf)

    def domains_block(self, buf):
        """The domain block of a `d_conf` buffer as a view (32 + 2L + 256 floats), None with `domains` off."""
        return self._view("domains", buf)

    def domain_search_block(self, buf):
        """The domain-search block of a `d_conf` buffer as a view ((400 + 2L) K floats), None with `search_domains` off."""
        floats = self.floats(DOMAIN_SEARCH)
        return buf[self.domain_search_off:self.domain_search_off + floats] if floats else None

    def domain_score_block(self, buf):
        """The domain-score block of a `d_conf` buffer as a view (1040 + 4L floats), None with `score_domains` off."""
        floats = self.floats(DOMAIN_SCORES)
        return buf[self.domain_score_off:self.domain_score_off + floats] if floats else None

    def flex_block(self, buf):
        """The flex block of a `d_conf` buffer as a view (48 + 20L floats), None with `flex` off."""
        floats = self.floats(FLEX)
        return buf[self.flex_off:self.flex_off + floats] if floats else None

    def msa_report_block(self, buf):
        """The report block of a `d_conf` buffer as a view (128 + 8L floats, + L*L with `msa_report` 2), None with it off."""
        floats = self.floats(MSA_REPORT)
        return buf[self.msa_report_off:self.msa_report_off + floats] if floats else None


# The positional functions that tests, tools and outside callers use: each one view of a `Layout`.
def conf_floats(L, distmap=False, score=False, align_m=None, score_map=False):
    """Floats the `d_conf` buffer of a prediction of length L must hold: the confidences, the L*L + 3 floats of option
    "emit_distmap", the 5L + 24 floats of option "score_native", the 64 + L floats of option "score_map" and, with `align_m`
    (the structure's rows; not None), the 25 + 2L + 3m floats of option "align_structure", in this order."""
    return Layout(L, distmap, score, score_map, align_m).total


def align_offset(L, distmap=False, score=False, score_map=False):
    """Where the align block begins in the `d_conf` buffer (A0 of include/dmpfold_hip.h)."""
    return Layout(L, distmap, score, score_map).align_off


def mapscore_offset(L, distmap=True, score=True):
    """Where the map-score block begins in the `d_conf` buffer (M0 of include/dmpfold_hip.h): the end of the score block."""
    return Layout(L, distmap, score).mapscore_off


def score_offset(L, distmap=False):
    """Where the score block begins in the `d_conf` buffer (S0 of include/dmpfold_hip.h)."""
    return Layout(L, distmap).score_off


def distmap_floats(L, on=True):
    """Floats the `d_conf` buffer of a prediction of length L must hold: L, or L + L*L + 3 with option "emit_distmap"."""
    return Layout(L, on).total


class Outputs(namedtuple("Outputs", "coords confs distmap info score_block align_block search_block map_block pass_block ss_block "
                         "exposure_block", defaults=(None,) * 9)):
    """What a prediction gives: coords (L, 5, 3), and the parts of its `d_conf` buffer as views of the one allocation -
    confs (L,), with "emit_distmap" distmap (L, L) and info (3,) = [best_pass, passes_run, map_rms], with "score_native"
    score_block (5L + 24,), with "align_structure" align_block (25 + 2L + 3m,), with "search_structures" search_block
    (26K + 2LK + 3M,), with "score_map" map_block (64 + L,), with "score_passes" pass_block (16 + 8R,), with "assign_ss"
    ss_block (32 + 8L,), with "exposure" exposure_block (32 + 16L,) - None for what is absent.  The blocks stand in the
    order they are handed out in (HANDOUT), not the buffer's (BLOCKS, at the end of this module).  With "domains"
    `domains_block` (32 + 2L + 256,) is an attribute beside the eleven fields, which callers unpack by position; it is handed
    out behind them all."""
    __hash__ = tuple.__hash__
    domains_block = None
    domain_search_block = None       # with "search_domains": (400 + 2L) K floats; an attribute too, and never handed out by `public`
    domain_score_block = None        # with "score_domains": 1040 + 4L floats; likewise
    flex_block = None                # with "flex": 48 + 20L floats; likewise
    msa_report_block = None          # with "msa_report": 128 + 8L (+ L*L) floats; likewise

    def __new__(cls, *parts, domains_block=None, domain_search_block=None, domain_score_block=None, flex_block=None,
                msa_report_block=None, **named):
        self = super().__new__(cls, *parts, **named)
        self.flex_block = flex_block
        self.msa_report_block = msa_report_block
        self.domains_block = domains_block
        self.domain_search_block = domain_search_block
        self.domain_score_block = domain_score_block
        return self

    def _replace(self, **changes):
        domains_block = changes.pop("domains_block", self.domains_block)
        domain_search_block = changes.pop("domain_search_block", self.domain_search_block)
        domain_score_block = changes.pop("domain_score_block", self.domain_score_block)
        flex_block = changes.pop("flex_block", self.flex_block)
        msa_report_block = changes.pop("msa_report_block", self.msa_report_block)
        new = super()._replace(**changes)
        new.flex_block = flex_block
        new.msa_report_block = msa_report_block
        new.domains_block = domains_block
        new.domain_search_block = domain_search_block
        new.domain_score_block = domain_score_block
        return new

    def __eq__(self, other):        # (a part is an array or a tensor, whose == is elementwise: parts are the same by identity)
        return isinstance(other, tuple) and len(self) == len(other) and all(
            a is b or (not hasattr(a, "shape") and not hasattr(b, "shape") and a == b) for a, b in zip(self, other))

    def __ne__(self, other):
        return not self == other

    @classmethod
    def of(cls, public, distmap, score, align=False, search=False, score_map=False, passes=False, ss=False, exposure=False,
           domains=False):
        """The inverse of `public` for a caller that knows which options were on (the keywords stand in HANDOUT's order)."""
        rest = iter(public)
        parts = [next(rest) if on else None
                 for on in (True, True, distmap, distmap, score, align, search, score_map, passes, ss, exposure)]
        return cls(*parts, domains_block=next(rest) if domains else None)

    def public(self, distmap=True, score=True, align=True, search=True, score_map=True, blocks=True, passes=True, ss=True,
               exposure=True, domains=True):
        """The tuple the public calls return: (coords, confs), then (distmap, info) if present and wanted, then the score
        block, the align block, the search block and - though they lie behind the score block in the buffer - the map-score
        block, the pass block, the SS block, the exposure block and, last of all, the domain block, each if present and wanted.
        `blocks=False`: none of the blocks, whatever else is said - what a call of an `Engine` returns, `public(distmap, blocks=False)`."""
        wanted = (score, align, search, score_map, passes, ss, exposure)
        return (self[:2] + (self[2:4] if distmap and self.distmap is not None else ())
                + tuple(block for block, want in zip(self[4:] + (self.domains_block,), wanted + (domains,))
                        if blocks and want and block is not None))


# the blocks, by field, in the order `public` hands them out and `of` takes them
HANDOUT = Outputs._fields[4:] + ("domains_block",)


def split_conf_buffer(buf, L, emit=False, score=False, coords=None, align_m=None, search=None, score_map=False):
    """The parts of a `d_conf` buffer (a 1-D tensor or array of at least conf_floats(L, emit, score, align_m, score_map)
    floats) at the offsets of include/dmpfold_hip.h, as the views of an `Outputs` (`coords` is passed through).  `search`:
    (K, M, max_L) of option "search_structures" - the search block then lies at search_offset(L, emit, score, align_m, max_L,
    score_map)."""
    return Layout(L, emit, score, score_map, align_m, search and search[:2], search and search[2]).split(buf, coords)


def split_distmap_buffer(buf, L):
    """The three parts of an "emit_distmap" output buffer (a 1-D tensor or array of distmap_floats(L) floats), as views:
    confs (L,), distmap (L, L) and info (3,) = [best_pass, passes_run, map_rms] (include/dmpfold_hip.h)."""
    if buf.ndim != 1 or buf.shape[0] != distmap_floats(L):
        raise ValueError(f"an emit_distmap buffer of length {L} has {distmap_floats(L)} floats, got shape {tuple(buf.shape)}")
    return Layout(L, True).split(buf)[1:4]


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
    b = _host(block)
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
    out = {"n_pairs": int(scores["n_pairs"]), "lnorm": _num(scores["lnorm"])}
    for name in SCORE_NAMES[1:]:
        out[name] = _num(scores[name])
    out["counts"] = [int(c) for c in scores["counts"]]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "score_map" (include/dmpfold_hip.h): the predicted distance map scored against the same native - contact precision
# of the top L, L/2 and L/5 predictions per sequence-separation class, the contacts at the 8 A threshold, and the distance
# agreement of the map itself (lDDT of the map, per residue and global; mean absolute error, RMSE, bias).  The library
# returns integer counts; the ratios are formed here.  THE REFERENCE HAS NO SUCH QUANTITY.
# ---------------------------------------------------------------------------------------------------------------------
MAP_CLASSES = ("short", "medium", "long", "medium_long")       # separations 6-11, 12-23, >= 24, >= 12
MAP_LISTS = ("L", "L2", "L5")                                  # the top ln, ln / 2, ln / 5 of a class
MAP_NAMES = ("map_lddt", "map_mae", "map_rmse", "map_bias")


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def unpack_map_scores(block, L):
    """A map-score block (64 + L floats, array or tensor) -> dict: n, ln, pairs (ordered pairs within 15 A), map_lddt,
    map_mae, map_rmse, map_bias, map_lddt_res (L,), and classes: {short, medium, long, medium_long} -> dict of the counts
    candidates, native_contacts, tp, predicted (at the 8 A threshold), hits and taken (3 ints each: the lists L, L/2, L/5) and
    the ratios formed from them: precision (3 floats, hits / taken), precision_8A (tp / predicted), recall_8A (tp /
    native_contacts), f1_8A - NaN where the denominator is 0.  A block the library answered with NaN (a latched fault) gives
    zero counts and NaN floats."""
    L = int(L)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != mapscore_floats(L):
        raise ValueError(f"a map-score block of length {L} has {mapscore_floats(L)} floats, got shape {tuple(b.shape)}")
    out = {"n": _whole(b[0]), "ln": float(b[1]), "pairs": _whole(b[50])}
    for k, name in enumerate(MAP_NAMES):
        out[name] = float(b[51 + k])
    out["map_lddt_res"] = b[MAPSCORE_HEADER:].copy()
    out["classes"] = {}
    for c, cname in enumerate(MAP_CLASSES):
        s = b[2 + 12 * c:14 + 12 * c]
        cl = {"candidates": _whole(s[0]), "native_contacts": _whole(s[1]), "hits": [_whole(v) for v in s[2:5]],
              "taken": [_whole(v) for v in s[5:8]], "tp": _whole(s[8]), "predicted": _whole(s[9])}
        cl["precision"] = [_ratio(h, t) for h, t in zip(cl["hits"], cl["taken"])]
        p, r = _ratio(cl["tp"], cl["predicted"]), _ratio(cl["tp"], cl["native_contacts"])
        cl["precision_8A"], cl["recall_8A"] = p, r
        cl["f1_8A"] = _ratio(2 * cl["tp"], cl["predicted"] + cl["native_contacts"])
        out["classes"][cname] = cl
    return out


def map_scores_json(ms):
    """`unpack_map_scores` without the per-residue array as a JSON-ready dict (the value of "map" in what `dmpfold --native
    --score-map` prints and `dmpfold-batch --natives --score-map` writes); NaN becomes None."""
    out = {"n": int(ms["n"]), "ln": _num(ms["ln"]), "pairs": int(ms["pairs"])}
    for name in MAP_NAMES:
        out[name] = _num(ms[name])
    for cname in MAP_CLASSES:
        cl = ms["classes"][cname]
        out[cname] = {k: ([int(v) for v in cl[k]] if isinstance(cl[k], list) else int(cl[k]))
                      for k in ("candidates", "native_contacts", "hits", "taken", "tp", "predicted")}
        out[cname]["precision"] = dict(zip(MAP_LISTS, (_num(v) for v in cl["precision"])))
        for k in ("precision_8A", "recall_8A", "f1_8A"):
            out[cname][k] = _num(cl[k])
    return out


def map_scores_flat(js):
    """The scalar figures of `map_scores_json` by name - map_lddt, map_mae, map_rmse, map_bias and <class>_<list> for the
    twelve list precisions - for tables, means and medians."""
    out = {name: js.get(name) for name in MAP_NAMES}
    for cname in MAP_CLASSES:
        for lname in MAP_LISTS:
            out[f"{cname}_{lname}"] = js[cname]["precision"][lname]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "score_passes" (include/dmpfold_hip.h): every recycling pass's trace scored against the same native, with the
# number the best-of rule compared (conf_mean) and the convergence measure (delta) beside the scores.  Row p's scores are
# exactly what "score_native" gives for ca_pass[p]; its delta is exactly what "recycle_tol_mA" compares.
# ---------------------------------------------------------------------------------------------------------------------
def _pass_index(v):
    """A pass index the library wrote as a float -> int, None for NaN."""
    return int(v) if v == v else None


def unpack_pass_scores(block, R):
    """A pass block (16 + 8R floats, array or tensor) -> dict: R, rows (int: the rows that hold a pass), best_pass, tm_pass,
    lddt_pass (int, or None where the library wrote NaN), regret_tm, regret_lddt (float) and one float32 array (R,) per
    column: conf_mean, delta, tm, gdt_ts, gdt_ha, rmsd, lddt - NaN at and beyond `rows`.  A block the library answered with
    NaN (a latched fault) gives rows 0 and None / NaN elsewhere."""
    R = int(R)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != pass_floats(R):
        raise ValueError(f"a pass block of {R} rows has {pass_floats(R)} floats, got shape {tuple(b.shape)}")
    out = {"R": R, "rows": _whole(b[0]), "best_pass": _pass_index(b[1]), "tm_pass": _pass_index(b[2]),
           "lddt_pass": _pass_index(b[3]), "regret_tm": float(b[4]), "regret_lddt": float(b[5])}
    table = b[PASS_HEADER:].reshape(R, PASS_ROW)
    for k, name in enumerate(PASS_COLUMNS):
        out[name] = table[:, k].copy()
    return out


def _num_inf(v):
    """A float for JSON: NaN becomes None, an infinity the string "inf" / "-inf" (pass 0's delta)."""
    v = float(v)
    if v != v:
        return None
    return v if abs(v) != float("inf") else ("inf" if v > 0 else "-inf")


def _from_json(v):
    return float("nan") if v is None else float(v)


def pass_scores_json(ps):
    """`unpack_pass_scores` as a JSON-ready dict (the value of "passes" in what `dmpfold --native --score-passes` prints and
    `dmpfold-batch --natives --score-passes` writes): the header fields and one list per column; NaN becomes None, pass 0's
    delta the string "inf"."""
    out = {"R": int(ps["R"]), "rows": int(ps["rows"])}
    for name in PASS_FIELDS[1:4]:
        out[name] = None if ps[name] is None else int(ps[name])
    for name in PASS_FIELDS[4:]:
        out[name] = _num(ps[name])
    for name in PASS_COLUMNS:
        out[name] = [_num_inf(v) for v in ps[name]]
    return out


def pass_scores_from_json(js):
    """The inverse of `pass_scores_json`: the dict `unpack_pass_scores` gives."""
    out = {"R": int(js["R"]), "rows": int(js["rows"])}
    for name in PASS_FIELDS[1:4]:
        out[name] = None if js[name] is None else int(js[name])
    for name in PASS_FIELDS[4:]:
        out[name] = _from_json(js[name])
    for name in PASS_COLUMNS:
        out[name] = np.asarray([_from_json(v) for v in js[name]], dtype=np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "assign_ss" (include/dmpfold_hip.h): secondary structure of the final backbone from its hydrogen bonds, on the GPU.
# DSSP's KIND of assignment, not its bits: no two-best-partner rule, no bulges, no sheet labels, no chain breaks; nobody has
# compared the strings with that program's.  The library returns codes and integer counts; strings and ratios are formed here.
# ---------------------------------------------------------------------------------------------------------------------
def _letters(codes, table):
    return "".join(table[int(v)] if v == v and 0 <= v < len(table) else "?" for v in codes)


def _index(a):
    """Indices the library wrote as floats -> int64, -1 for NaN."""
    return np.where(a == a, a, -1.0).astype(np.int64)


def unpack_ss(block, L):
    """An SS block (32 + 8L floats, array or tensor) -> dict: ss8 (a string of L letters from "-STIGBEH"), ss3 (H, E, C),
    n_hb, counts ({letter: residues}), n_parallel, n_antiparallel (bridge pairs), helix, strand, coil (fractions of L), e_acc,
    p_acc, e_don, p_don (the lowest hydrogen-bond energy of each residue as acceptor / donor and its partner, -1 for none), bp1,
    bp2 (the two lowest-numbered bridge partners, -1 where absent), has_native; with a native also ss8_native, ss3_native,
    counts_native, q3_match, q8_match and q3, q8 (the matches over L).  A block the library answered with NaN (a latched fault)
    gives '?' in the strings, zero counts and -1 partners."""
    L = int(L)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != ss_floats(L):
        raise ValueError(f"an SS block of length {L} has {ss_floats(L)} floats, got shape {tuple(b.shape)}")
    arr = b[SS_HEADER:].reshape(SS_ARRAYS, L)
    out = {"ss8": _letters(arr[0], SS_CODES), "ss3": _letters(arr[0], SS_THREE), "n_hb": _whole(b[0]),
           "counts": {SS_CODES[k]: _whole(b[1 + k]) for k in range(8)}, "n_parallel": _whole(b[9]), "n_antiparallel": _whole(b[10])}
    three = {"helix": "HGI", "strand": "EB", "coil": "-ST"}
    for name, letters in three.items():
        out[name] = sum(out["counts"][c] for c in letters) / float(L)
    out["e_acc"], out["p_acc"] = arr[1].copy(), _index(arr[2])
    out["e_don"], out["p_don"] = arr[3].copy(), _index(arr[4])
    out["bp1"], out["bp2"] = _index(arr[5]), _index(arr[6])
    out["has_native"] = bool(_whole(b[11]))
    if out["has_native"]:
        out["ss8_native"], out["ss3_native"] = _letters(arr[7], SS_CODES), _letters(arr[7], SS_THREE)
        out["counts_native"] = {SS_CODES[k]: _whole(b[14 + k]) for k in range(8)}
        out["q3_match"], out["q8_match"] = _whole(b[12]), _whole(b[13])
        out["q3"], out["q8"] = out["q3_match"] / float(L), out["q8_match"] / float(L)
    return out


SS_JSON_KEYS = ("ss8", "ss3", "n_hb", "counts", "n_parallel", "n_antiparallel", "helix", "strand", "coil", "has_native",
                "ss8_native", "ss3_native", "counts_native", "q3_match", "q8_match", "q3", "q8")


def ss_json(ss, arrays=False):
    """`unpack_ss` as a JSON-ready dict (what `dmpfold --ss` prints and `dmpfold-batch --ss` writes): the strings, the
    counts and the fractions; with `arrays` also the per-residue energies and partners as lists (NaN becomes None)."""
    out = {k: ss[k] for k in SS_JSON_KEYS if k in ss}
    if arrays:
        for k in ("e_acc", "e_don"):
            out[k] = [_num(v) for v in ss[k]]
        for k in ("p_acc", "p_don", "bp1", "bp2"):
            out[k] = [int(v) for v in ss[k]]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "exposure" (include/dmpfold_hip.h): solvent exposure of the final backbone on the GPU - a Shrake-Rupley surface of
# the N, CA, C, O and CB atoms (256 points per atom, 1.4 A probe), the half-sphere exposure of every residue (Hamelryck
# 2005, the CB variant) and a CB contact number.  Shrake & Rupley's KIND of surface on a model WITHOUT SIDE CHAINS: not
# DSSP's ACC, no relative accessibility, and nobody has compared the figures with another program's.  The library returns
# integer counts; areas, fractions and correlations are formed here in float64.
# ---------------------------------------------------------------------------------------------------------------------
def exposure_points():
    """The 256 unit vectors of the sphere lattice, float32 (256, 3): a golden spiral formed in float64 and rounded once.
    csrc/exposure_points.h (tools/make_exposure_points.py) holds these bits."""
    k = np.arange(EXPOSURE_POINTS, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(EXPOSURE_POINTS)
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def _count(a):
    """Counts the library wrote as floats -> int64, NaN as 0."""
    return np.where(a == a, a, 0.0).astype(np.int64)


def _pearson(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ok = (x == x) & (y == y)
    if ok.sum() < 2:
        return float("nan")
    x, y = x[ok] - x[ok].mean(), y[ok] - y[ok].mean()
    d = np.sqrt((x * x).sum() * (y * y).sum())
    return float((x * y).sum() / d) if d > 0 else float("nan")


def _mean(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[v == v]
    return float(v.mean()) if v.size else float("nan")


def _exposure_leg(header, arr, L):
    """One entity's seven header floats and eight arrays -> its part of `unpack_exposure`."""
    n = _index(arr[:5].T)                                                    # (L, 5); -1: a glycine's CB (and NaN)
    radii = np.asarray(EXPOSURE_RADII, dtype=np.float64)
    area = 4.0 * np.pi * radii * radii * np.maximum(n, 0).astype(np.float64) / float(EXPOSURE_POINTS)
    cb = np.where(n[:, 4] >= 0, n[:, 4] / float(EXPOSURE_POINTS), np.nan)
    out = {"atoms": _whole(header[0]), "sums": [_whole(v) for v in header[1:6]], "buried_atoms": _whole(header[6]),
           "n": n, "hse_up": _count(arr[5]), "hse_down": _count(arr[6]), "cn10": _count(arr[7]),
           "area_atom": area, "area_res": area.sum(axis=1), "area": float(area.sum()), "cb_exposed": cb}
    for name in ("hse_up", "hse_down", "cn10"):
        out["mean_" + name] = float(out[name].mean()) if L else float("nan")
    return out


def unpack_exposure(block, L, seq=None):
    """An exposure block (32 + 16L floats, array or tensor) -> dict: points (256), atoms (the atoms present), sums (exposed
    points of the N, CA, C, O, CB atoms), buried_atoms (atoms without an exposed point), n (L, 5) int - exposed points per atom,
    -1 for a glycine's CB -, hse_up, hse_down, cn10 (L,) int, and formed here in float64: area_atom (L, 5) = 4 pi R^2 n / 256,
    area_res (L,), area, cb_exposed (L,) = n_CB / 256 (NaN for glycine), mean_hse_up, mean_hse_down, mean_cn10; has_native,
    and with a native the same under "native" plus r_area, r_hse_up, r_cn10 (Pearson r between model and native per residue).
    `seq` (the query as a string or as residue codes): also cb_hydrophobic, cb_other (the mean cb_exposed of A V I L M F W C and
    of the other non-glycine residues) and burial_ratio, their quotient.  A block the library answered with NaN (a latched
    fault) gives zero counts and -1 in n."""
    L = int(L)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != exposure_floats(L):
        raise ValueError(f"an exposure block of length {L} has {exposure_floats(L)} floats, got shape {tuple(b.shape)}")
    arr = b[EXPOSURE_HEADER:].reshape(EXPOSURE_ARRAYS, L)
    out = {"points": _whole(b[0])}
    out.update(_exposure_leg(b[1:8], arr[:8], L))
    out["has_native"] = bool(_whole(b[8]))
    if out["has_native"]:
        nat = _exposure_leg(b[9:16], arr[8:], L)
        out["native"] = nat
        out["r_area"] = _pearson(out["area_res"], nat["area_res"])
        out["r_hse_up"] = _pearson(out["hse_up"], nat["hse_up"])
        out["r_cn10"] = _pearson(out["cn10"], nat["cn10"])
    if seq is not None:
        letters = seq if isinstance(seq, str) else "".join(AA1[int(c)] if 0 <= int(c) < 20 else "X" for c in np.asarray(seq).reshape(-1)[:L])
        if len(letters) != L:
            raise ValueError(f"the sequence has {len(letters)} residues, the block {L}")
        hyd = np.asarray([c in HYDROPHOBIC for c in letters], dtype=bool)
        for leg in [out] + ([out["native"]] if out["has_native"] else []):
            present = leg["cb_exposed"] == leg["cb_exposed"]
            leg["cb_hydrophobic"], leg["cb_other"] = _mean(leg["cb_exposed"][hyd & present]), _mean(leg["cb_exposed"][~hyd & present])
            leg["burial_ratio"] = _ratio(leg["cb_hydrophobic"], leg["cb_other"]) if leg["cb_other"] == leg["cb_other"] else float("nan")
    return out


EXPOSURE_SCALARS = ("area", "mean_hse_up", "mean_hse_down", "mean_cn10", "cb_hydrophobic", "cb_other", "burial_ratio")


def exposure_json(ex, arrays=False):
    """`unpack_exposure` as a JSON-ready dict (what `dmpfold --exposure` prints and `dmpfold-batch --exposure` writes): the
    counts, the total area, the means and, with a native, the same under "native" and the three correlations; with `arrays`
    also n, hse_up, hse_down, cn10 and area_res as lists.  NaN becomes None."""
    def leg(d):
        js = {"atoms": int(d["atoms"]), "sums": [int(v) for v in d["sums"]], "buried_atoms": int(d["buried_atoms"])}
        js.update({k: _num(d[k]) for k in EXPOSURE_SCALARS if k in d})
        js["mean_cb_exposed"] = _num(_mean(d["cb_exposed"]))
        if arrays:
            js["n"] = [[int(v) for v in row] for row in d["n"]]
            for k in ("hse_up", "hse_down", "cn10"):
                js[k] = [int(v) for v in d[k]]
            js["area_res"] = [_num(v) for v in d["area_res"]]
        return js
    out = {"points": int(ex["points"])}
    out.update(leg(ex))
    out["has_native"] = bool(ex["has_native"])
    if ex["has_native"]:
        out["native"] = leg(ex["native"])
        for k in ("r_area", "r_hse_up", "r_cn10"):
            out[k] = _num(ex[k])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "domains" (include/dmpfold_hip.h): the final C-alpha trace split into structural domains on the GPU by recursive
# contact-density bisection.  The block holds integers only; radii of gyration, mean confidences and the overlap with the
# native's parse are formed here in float64.
# ---------------------------------------------------------------------------------------------------------------------
def _segments(labels, d):
    """[[first, last]] (inclusive) of the runs of residues with label d."""
    idx = np.flatnonzero(labels == d)
    if idx.size == 0:
        return []
    breaks = np.flatnonzero(np.diff(idx) > 1)
    return [[int(a), int(b)] for a, b in zip(idx[np.r_[0, breaks + 1]], idx[np.r_[breaks, idx.size - 1]])]


def _domains_leg(header, labels, table, ca=None, confs=None):
    """One leg's sixteen header floats, L labels and 16 x 8 table -> its part of `unpack_domains`."""
    out = {name: _whole(v) for name, v in zip(DOMAINS_FIELDS, header)}
    out["unexamined"] = bool(out["unexamined"])
    n = min(max(out["domains"], 0), DOMAINS_MAX)
    labels = _index(labels)
    out["labels"] = labels
    rows, splits = [], {}
    for d in range(n):
        row = {name: _whole(v) for name, v in zip(DOMAINS_COLUMNS, table[d])}
        row["segment_list"] = _segments(labels, d)
        row["q"] = row["cut_ext"] / row["cut_den"] if row["cut_den"] else None
        mine = labels == d
        if ca is not None:
            x = np.asarray(ca, dtype=np.float64).reshape(-1, 3)[mine]
            row["rg"] = float(np.sqrt(((x - x.mean(0)) ** 2).sum(1).mean())) if x.size else float("nan")
        if confs is not None:
            c = np.asarray(confs, dtype=np.float64).reshape(-1)[mine]
            row["mean_conf"] = float(c.mean()) if c.size else float("nan")
        rows.append(row)
        if row["cut_den"]:
            splits.setdefault((row["level"], row["cut_ext"], row["cut_den"]), row["q"])
    out["table"] = rows
    # q of every split that left a domain in the table: one per (level, ext, denominator), shallowest first
    out["splits"] = [{"level": level - 1, "ext": ext, "den": den, "q": q} for (level, ext, den), q in sorted(splits.items())]
    return out


def domains_overlap(a, b):
    """The share of residues whose labels agree when the domains of `a` are matched with those of `b` greedily by largest
    overlap (each domain matched at most once; ties to the lower labels)."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    ok = (a >= 0) & (b >= 0)
    if a.shape != b.shape or not ok.any():
        return float("nan")
    table = np.zeros((int(a[ok].max()) + 1, int(b[ok].max()) + 1), dtype=np.int64)
    np.add.at(table, (a[ok], b[ok]), 1)
    agree = 0
    while table.size and table.max() > 0:
        i, j = np.unravel_index(int(table.argmax()), table.shape)
        agree += int(table[i, j])
        table[i, :] = 0
        table[:, j] = 0
    return agree / float(a.shape[0])


def unpack_domains(block, L, coords=None, confs=None):
    """A domain block (32 + 2L + 256 floats, array or tensor) -> dict: domains, contacts, tau_milli, min_size, min_segment,
    discontinuous (domains of more than one segment), depth (the deepest level a domain lies at), unexamined (a final domain
    of level 4 was large enough to examine), labels (L,) int, table (per domain: size, segments, first, contacts,
    contacts_out, cut_ext, cut_den, level, segment_list [[first, last]], q of the cut that made it or None) and splits (level,
    ext, den, q of every split).  `coords` ((L, 5, 3) or the (L, 3) C-alpha trace) adds every domain's radius of gyration
    `rg`, `confs` its `mean_conf`, both in float64.  has_native, and with a native leg the same under "native" plus `overlap`
    (domains_overlap of the two labellings).  A block the library answered with NaN (a latched fault) gives zero counts."""
    L = int(L)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != domains_floats(L):
        raise ValueError(f"a domain block of length {L} has {domains_floats(L)} floats, got shape {tuple(b.shape)}")
    ca = None
    if coords is not None:
        ca = _host(coords)
        ca = ca.reshape(L, 5, 3)[:, 1] if ca.size == 15 * L else ca.reshape(L, 3)
    tables = b[DOMAINS_HEADER + 2 * L:].reshape(2, DOMAINS_MAX, DOMAINS_ROW)
    out = _domains_leg(b[:16], b[DOMAINS_HEADER:DOMAINS_HEADER + L], tables[0], ca, None if confs is None else _host(confs))
    out["has_native"] = _whole(b[16]) > 0
    if out["has_native"]:
        out["native"] = _domains_leg(b[16:32], b[DOMAINS_HEADER + L:DOMAINS_HEADER + 2 * L], tables[1])
        out["overlap"] = domains_overlap(out["labels"], out["native"]["labels"])
    return out


def domains_json(dom, arrays=False):
    """`unpack_domains` as a JSON-ready dict (what `dmpfold --domains` prints): the header, every domain's row with its
    segments and, where given, rg and mean_conf, the splits and, with a native, the same under "native" and the overlap; with
    `arrays` also the labels as a list.  NaN becomes None."""
    def leg(d):
        js = {k: (bool(d[k]) if k == "unexamined" else int(d[k])) for k in DOMAINS_FIELDS}
        js["table"] = [{k: (_num(v) if isinstance(v, float) else v) for k, v in row.items()} for row in d["table"]]
        js["splits"] = [dict(sp, q=_num(sp["q"])) for sp in d["splits"]]
        if arrays:
            js["labels"] = [int(v) for v in d["labels"]]
        return js
    out = leg(dom)
    out["has_native"] = bool(dom["has_native"])
    if dom["has_native"]:
        out["native"] = leg(dom["native"])
        out["overlap"] = _num(dom["overlap"])
    return out


def simulate_converge(conf_mean, delta, tol_angstrom):
    """What a run with the convergence stop at `tol_angstrom` (the `converge` of the front ends, option "recycle_tol_mA" =
    converge_to_mA of it) would have done, decided from a full-depth pass table alone -> (passes_run, best_pass).  The stop
    falls behind the first pass p >= 1 with float32(delta[p]) <= float32(tol_mA) * float32(1e-3), the library's comparison in
    its float32 arithmetic (false for NaN); without one, or with the tolerance 0 (off), every row ran.  best_pass is the
    strict '>' scan over conf_mean[0 .. passes_run - 1]: the earliest of equals stays.  Rows that hold no pass (NaN
    conf_mean at the table's end) do not count."""
    conf = np.asarray(conf_mean, dtype=np.float32).reshape(-1)
    delta = np.asarray(delta, dtype=np.float32).reshape(-1)
    n = conf.shape[0]
    while n > 0 and conf[n - 1] != conf[n - 1]:
        n -= 1
    tol_mA = tolerance_mA(tol_angstrom)
    tol = np.float32(tol_mA) * np.float32(1e-3)
    run = n
    if tol_mA > 0:
        for p in range(1, n):
            if delta[p] <= tol:
                run = p + 1
                break
    best = 0
    for p in range(1, run):
        if conf[p] > conf[best]:
            best = p
    return run, best


def tolerance_mA(tol_angstrom):
    """A tolerance in Angstrom as the whole milli-Angstrom option "recycle_tol_mA" takes (None and 0 = off)."""
    if tol_angstrom is None:
        return 0
    t = float(tol_angstrom)
    if not t >= 0.0:
        raise ValueError(f"a convergence tolerance must be >= 0 Angstrom, got {tol_angstrom}")
    return int(round(t * 1000.0))


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
    b = _host(block)
    m = (b.shape[0] - (1 + ALIGN_HEADER + 2 * L)) // 3 if b.ndim == 1 else -1
    if m < 0 or b.shape[0] != align_floats(L, m):
        raise ValueError(f"an align block of length {L} has 25 + 2L + 3m floats, got shape {tuple(b.shape)}")
    h = b[1:1 + ALIGN_HEADER]
    out = {"n_ali": _whole(h[0]), "rmsd_ali": float(h[1]), "tm_model": float(h[2]), "tm_struct": float(h[3]),
           "R": h[4:13].reshape(3, 3).copy(), "t": h[13:16].copy(), "d0_model": float(h[16]), "d0_struct": float(h[17]),
           "seed_offset": _whole(h[18]), "seeds": _whole(h[19])}
    ali = b[1 + ALIGN_HEADER:1 + ALIGN_HEADER + L]
    out["ali"] = np.where(ali == ali, ali, -1.0).astype(np.int64)
    out["deviation"] = b[1 + ALIGN_HEADER + L:1 + ALIGN_HEADER + 2 * L].copy()
    out["m"] = float(b[0])
    out["structure"] = b[1 + ALIGN_HEADER + 2 * L:].reshape(m, 3).copy()
    return out


def alignment_json(al):
    """`unpack_alignment` as a JSON-ready dict (what `dmpfold --compare` prints and `dmpfold-batch --structures` writes):
    the header fields, R, t and ali; NaN becomes None."""
    out = {"m": _num(al["m"])}
    for name in ALIGN_NAMES:
        out[name] = int(al[name]) if name in ("n_ali", "seed_offset", "seeds") else _num(al[name])
    out["R"] = [[_num(v) for v in row] for row in np.asarray(al["R"])]
    out["t"] = [_num(v) for v in np.asarray(al["t"])]
    out["ali"] = [int(v) for v in al["ali"]]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "search_structures" (include/dmpfold_hip.h): the model aligned with each of the K structures of a library in one
# prediction, and the ranking by tm_model.  Entry k's numbers are exactly what "align_structure" gives for that structure
# alone - the same kind of search, the same lower bound, not compared with TM-align.
# ---------------------------------------------------------------------------------------------------------------------
SEARCH_MAX = 4096                    # DMP_SEARCH_MAX


def search_floats(L, K, M):
    """Floats of the search block of a prediction of length L searching K entries of M rows in all."""
    L, K = int(L), int(K)
    return (2 + ALIGN_HEADER) * K + 2 * L * K + 3 * int(M)


def align_m_rule(m, max_L):
    """m' of the rule for B0: the align block's m if that is an integer in [3, max_L], else 0 (None: no align block)."""
    if m is None:
        return 0
    m = float(m)
    return int(m) if m == m and 3 <= m <= int(max_L) and m == int(m) else 0


def search_offset(L, distmap=False, score=False, align_m=None, max_L=None, score_map=False):
    """Where the search block begins in the `d_conf` buffer (B0 of include/dmpfold_hip.h): the end of what the other options
    give.  `align_m`: the m the align block holds (None = "align_structure" off); the library counts 3m of it only if it is
    an integer in [3, `max_L`] (`max_L` None: whatever the block's writer allocated, i.e. any whole m >= 0 counts)."""
    return Layout(L, distmap, score, score_map, align_m, None, max_L).search_off


class Library:
    """A fold library: names, lengths and one concatenated float32 C-alpha trace (M, 3), M = sum of the lengths.
    `refine` (option "search_refine"): 0 = every entry is refined; R = every entry is screened by its best gapless threading
    and only the R best by that are refined.  `domains` (option "search_domains"): the library is also searched with every
    domain of the model (the host layers then turn option "domains" on themselves)."""

    domains = False

    def __init__(self, names, lengths, ca, refine=0):
        self.names = [str(n) for n in names]
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.ca = np.ascontiguousarray(np.asarray(ca, dtype=np.float32).reshape(-1, 3))
        if len(self.names) != self.lengths.shape[0] or int(self.lengths.sum()) != self.ca.shape[0]:
            raise ValueError(f"library: {len(self.names)} names, {self.lengths.shape[0]} lengths summing to "
                             f"{int(self.lengths.sum())}, {self.ca.shape[0]} rows")
        if not 1 <= len(self.names) <= SEARCH_MAX:
            raise ValueError(f"library: {len(self.names)} entries; 1 to {SEARCH_MAX} can be searched")
        self._device = {}                # device -> the packed inputs there (they do not depend on L)
        self._refine = 0
        self.refine = refine

    @property
    def refine(self):
        return self._refine

    @refine.setter
    def refine(self, value):
        if isinstance(value, bool) or int(value) != value or not 0 <= int(value) <= SEARCH_MAX:
            raise ValueError(f"refine must be 0 or 1 .. {SEARCH_MAX}, got {value!r}")
        self._refine = int(value)

    def __len__(self):
        return len(self.names)

    @property
    def rows(self):
        return int(self.ca.shape[0])

    @property
    def max_m(self):
        return int(self.lengths.max())

    def entry(self, k):
        """Entry k's trace (m_k, 3)."""
        o = int(self.lengths[:k].sum())
        return self.ca[o:o + int(self.lengths[k])]

    def check(self, capacity):
        """Raises ValueError naming the first entry with fewer than 3 rows or more than `capacity`."""
        for name, m in zip(self.names, self.lengths):
            if m < 3 or m > int(capacity):
                raise ValueError(f"library entry {name}: {int(m)} C-alpha atoms; 3 to {int(capacity)} can be aligned")

    @classmethod
    def from_traces(cls, traces, names=None):
        traces = [as_structure(t) for t in traces]
        names = [f"entry{k}" for k in range(len(traces))] if names is None else names
        return cls(names, [t.shape[0] for t in traces], np.concatenate(traces) if traces else np.zeros((0, 3), np.float32))

    @classmethod
    def from_dir(cls, path):
        """Every *.pdb of a directory (first chain; read_native_ca), names = the stems, in sorted order."""
        import glob
        import os
        files = sorted(glob.glob(os.path.join(path, "*.pdb")))
        if not files:
            raise ValueError(f"{path}: no *.pdb files")
        return cls.from_traces([read_native_ca(f)[0] for f in files], [os.path.splitext(os.path.basename(f))[0] for f in files])

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls([str(n) for n in z["names"]], z["lengths"], z["ca"])

    @classmethod
    def open(cls, path, refine=0, domains=False):
        """A directory of PDB files or an .npz written by `save`; `refine`, `domains`: the library's `refine` and `domains`."""
        import os
        library = cls.from_dir(path) if os.path.isdir(path) else cls.load(path)
        library.refine = refine
        library.domains = bool(domains)
        return library

    def save(self, path):
        with open(path, "wb") as fh:
            np.savez(fh, names=np.asarray(self.names, dtype=np.str_), lengths=self.lengths, ca=self.ca)

    def device_inputs(self, device):
        """(lengths as float32 (K,), traces (3M,)) on `device`: uploaded once per device, kept on the library."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.lengths.astype(np.float32)).to(device),
                                 torch.from_numpy(self.ca.reshape(-1)).to(device))
        return self._device[key]

    def fill_block(self, block, L):
        """The inputs of a search block on the GPU (a tensor of search_floats(L, K, M)) filled device to device, NaN elsewhere."""
        lens, ca = self.device_inputs(block.device)
        K = len(self)
        block[:K].copy_(lens)
        block[K:block.shape[0] - ca.shape[0]].fill_(float("nan"))
        block[block.shape[0] - ca.shape[0]:].copy_(ca)


def pack_library(library, L, lengths=None):
    """The search block (float32 (26K + 2LK + 3M,)) with its inputs filled in - the lengths in front, the traces at the end -
    and NaN in the out slots.  `lengths`: what to write as the m_k instead (tests of the library's validation)."""
    K, L = len(library), int(L)
    block = np.full(search_floats(L, K, library.rows), np.nan, dtype=np.float32)
    block[:K] = library.lengths if lengths is None else np.asarray(lengths, dtype=np.float32)
    block[block.shape[0] - 3 * library.rows:] = library.ca.reshape(-1)
    return block


def unpack_search(block, L, lengths, refine=0):
    """A search block (array or tensor) of a library with these `lengths` -> dict: hits, a list of K dicts in the shape
    `unpack_alignment` gives (m, structure and all), and rank (K,) int - the entries by falling tm_model, ties to the lower
    index, NaN last.  A block the library answered with NaN in rank (a latched fault) gives rank 0 .. K-1.
    `refine`: the "search_refine" the prediction ran with; with 0 < refine < K the dict also has refined (K,) bool - the
    entries whose numbers are a refined alignment's (header offset 21 == 0), not the screen's gapless one."""
    L = int(L)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    K, M = lengths.shape[0], int(lengths.sum())
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != search_floats(L, K, M):
        raise ValueError(f"a search block of length {L}, {K} entries, {M} rows has {search_floats(L, K, M)} floats, got shape {tuple(b.shape)}")
    hdr, res, tr = 2 * K, (2 + ALIGN_HEADER) * K, (2 + ALIGN_HEADER) * K + 2 * L * K
    hits, o = [], 0
    for k in range(K):
        m = int(lengths[k])
        one = np.concatenate([b[k:k + 1], b[hdr + ALIGN_HEADER * k:hdr + ALIGN_HEADER * (k + 1)], b[res + 2 * L * k:res + 2 * L * (k + 1)],
                              b[tr + 3 * o:tr + 3 * (o + m)]])
        hits.append(unpack_alignment(one, L))
        o += m
    rank = b[K:2 * K]
    out = {"hits": hits, "rank": rank.astype(np.int64) if np.all(rank == rank) else np.arange(K, dtype=np.int64)}
    if 0 < int(refine) < K:
        out["refined"] = b[hdr + 20:hdr + ALIGN_HEADER * K:ALIGN_HEADER] == 0
    return out


def host_rank(tm):
    """The ranking rule on the host: by falling value, ties to the lower index, NaN last in index order."""
    tm = np.asarray(tm, dtype=np.float32)
    return np.asarray(sorted(range(len(tm)), key=lambda k: (tm[k] != tm[k], -float(tm[k]) if tm[k] == tm[k] else 0.0, k)), dtype=np.int64)


def hits_json(search, names, top=10, refine=0):
    """`unpack_search` as a JSON-ready dict (what `dmpfold --search` prints and `dmpfold-batch --library` writes): the best
    `top` entries in rank order, each with name, tm_model, tm_struct, rmsd_ali, n_ali, R, t; NaN becomes None.  `refine`: as
    for `unpack_search`; where that gave `refined`, the dict has "refine" and every hit "refined"."""
    out = []
    refined = search.get("refined") if 0 < int(refine) < len(names) else None
    for k in [int(k) for k in search["rank"][:max(int(top), 0)]]:
        h = search["hits"][k]
        out.append({"name": str(names[k]), "index": k, "tm_model": _num(h["tm_model"]), "tm_struct": _num(h["tm_struct"]),
                    "rmsd_ali": _num(h["rmsd_ali"]), "n_ali": int(h["n_ali"]),
                    "R": [[_num(v) for v in row] for row in np.asarray(h["R"])], "t": [_num(v) for v in np.asarray(h["t"])]})
        if refined is not None:
            out[-1]["refined"] = bool(refined[k])
    return {"entries": len(names), "hits": out} if refined is None else {"entries": len(names), "refine": int(refine), "hits": out}


# ---------------------------------------------------------------------------------------------------------------------
# option "search_domains" (include/dmpfold_hip.h): the library searched with every domain of the model.  Pair (d, k) is what
# "align_structure" gives for the domain's gathered trace and entry k, ali and deviation scattered back to the domain's residues;
# the same kind of search, the same lower bound per pair, not compared with TM-align.
# ---------------------------------------------------------------------------------------------------------------------
def domain_search_floats(L, K):
    """Floats of the domain-search block of a prediction of length L searching K entries: rank [16][K], 16 K headers of 24
    floats, K x (ali [L], deviation [L]) - all of it out."""
    L, K = int(L), int(K)
    return DOMAINS_MAX * K * (1 + ALIGN_HEADER) + 2 * L * K


def domain_search_offset(L, distmap=False, score=False, score_map=False, passes=None, ss=False, exposure=False):
    """Where the domain-search block begins in the `d_conf` buffer: the end of the domain block."""
    return Layout(L, distmap, score, score_map, passes=passes, ss=ss, exposure=exposure, domains=True).domain_search_off


def pack_domain_search(L, K, rank=None, headers=None, ali=None, deviation=None):
    """A domain-search block (float32) from its parts, NaN where a part is None: rank (16, K), headers (16, K, 24), ali (K, L),
    deviation (K, L) - the inverse of the raw views of `unpack_domain_search` (tests, restatements)."""
    L, K = int(L), int(K)
    block = np.full(domain_search_floats(L, K), np.nan, dtype=np.float32)
    r = DOMAINS_MAX * K
    if rank is not None:
        block[:r] = np.asarray(rank, dtype=np.float32).reshape(r)
    if headers is not None:
        block[r:r * (1 + ALIGN_HEADER)] = np.asarray(headers, dtype=np.float32).reshape(r * ALIGN_HEADER)
    res = block[r * (1 + ALIGN_HEADER):].reshape(K, 2, L)
    if ali is not None:
        res[:, 0] = np.asarray(ali, dtype=np.float32).reshape(K, L)
    if deviation is not None:
        res[:, 1] = np.asarray(deviation, dtype=np.float32).reshape(K, L)
    return block


def unpack_domain_search(block, L, K, refine=0):
    """A domain-search block (array or tensor) of a search of K entries -> dict: domains (D: the rows of `rank` that are no
    NaN; 0 for a block the library answered with NaN - a bad m_k, a latched fault), rank (D, K) int - per domain the entries by
    falling tm_model, the pair's TM-score normalised by the domain's size, ties to the lower index, NaN last -, hits (per
    domain a list of K dicts: n_ali, rmsd_ali, tm_model, tm_struct, R, t, d0_model, d0_struct, seed_offset, seeds), ali (K, L)
    int - the row of entry k aligned with residue i under the alignment of i's own domain, or -1 - and deviation (K, L); the
    raw views `headers` (16, K, 24) and `rank_raw` (16, K).  `refine`: the "search_refine" the prediction ran with; with 0 <
    refine < K also refined (D, K) bool."""
    L, K = int(L), int(K)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != domain_search_floats(L, K):
        raise ValueError(f"a domain-search block of length {L}, {K} entries has {domain_search_floats(L, K)} floats, got shape {tuple(b.shape)}")
    r = DOMAINS_MAX * K
    rank_raw = b[:r].reshape(DOMAINS_MAX, K)
    headers = b[r:r * (1 + ALIGN_HEADER)].reshape(DOMAINS_MAX, K, ALIGN_HEADER)
    res = b[r * (1 + ALIGN_HEADER):].reshape(K, 2, L)
    whole = np.all(rank_raw == rank_raw, axis=1)
    D = int(whole.sum()) if np.all(whole[:int(whole.sum())]) else 0
    hits = []
    for d in range(D):
        row = []
        for k in range(K):
            h = headers[d, k]
            row.append({"n_ali": _whole(h[0]), "rmsd_ali": float(h[1]), "tm_model": float(h[2]), "tm_struct": float(h[3]),
                        "R": h[4:13].reshape(3, 3).copy(), "t": h[13:16].copy(), "d0_model": float(h[16]), "d0_struct": float(h[17]),
                        "seed_offset": _whole(h[18]), "seeds": _whole(h[19])})
        hits.append(row)
    ali = res[:, 0]
    out = {"domains": D, "rank": rank_raw[:D].astype(np.int64), "hits": hits, "ali": np.where(ali == ali, ali, -1.0).astype(np.int64),
           "deviation": res[:, 1].copy(), "headers": headers.copy(), "rank_raw": rank_raw.copy()}
    if 0 < int(refine) < K:
        out["refined"] = headers[:D, :, 20] == 0
    return out


def domain_hits_json(ds, names, domains=None, top=10, refine=0):
    """`unpack_domain_search` as a JSON-ready dict (the key "domain_hits" of `dmpfold --search ... --search-domains` and of
    `dmpfold-batch`): per domain its number and - with `domains`, the dict of `unpack_domains` of the same prediction - its size
    and segment list, then its best `top` entries in rank order, each with name, index, tm_domain (normalised by the domain's
    size), tm_struct, rmsd_ali, n_ali, R, t and, where `unpack_domain_search` gave `refined`, refined; NaN becomes None."""
    refined = ds.get("refined") if 0 < int(refine) < len(names) else None
    out = []
    for d in range(ds["domains"]):
        js = {"domain": d}
        if domains is not None and d < len(domains["table"]):
            js["size"] = int(domains["table"][d]["size"])
            js["segments"] = [list(seg) for seg in domains["table"][d]["segment_list"]]
        js["hits"] = []
        for k in [int(k) for k in ds["rank"][d][:max(int(top), 0)]]:
            h = ds["hits"][d][k]
            js["hits"].append({"name": str(names[k]), "index": k, "tm_domain": _num(h["tm_model"]), "tm_struct": _num(h["tm_struct"]),
                               "rmsd_ali": _num(h["rmsd_ali"]), "n_ali": int(h["n_ali"]),
                               "R": [[_num(v) for v in row] for row in np.asarray(h["R"])], "t": [_num(v) for v in np.asarray(h["t"])]})
            if refined is not None:
                js["hits"][-1]["refined"] = bool(refined[d][k])
        out.append(js)
    js = {"entries": len(names), "domains": out}
    if refined is not None:
        js["refine"] = int(refine)
    return js


# ---------------------------------------------------------------------------------------------------------------------
# option "score_domains" (include/dmpfold_hip.h): every domain of the model's labels (leg 0) and of the native's (leg 1) scored
# against the native on its own superposition.  Row (leg, d) is what "score_native" gives for a native masked to the domain, with
# lnorm 0; the library adds the integer counts of the pairs that leave the domain, and the ratios are formed here.
# THE TM-SCORE PROGRAM'S KIND OF SEARCH PER DOMAIN, A LOWER BOUND, NOT ITS BITS; the domains are "domains"' contact-density
# bisection, with no validation on real domains; nobody has compared the figures with an assessor's.
# ---------------------------------------------------------------------------------------------------------------------
DOMSCORE_HEADER = 16                 # floats in front of the two tables of the domain-score block
DOMSCORE_ROW = 32                    # floats of a row


def domain_score_floats(L):
    """Floats of the domain-score block (option "score_domains") of a prediction of length L: 16 + 2 x 16 x 32 + 4L."""
    return DOMSCORE_HEADER + 2 * DOMAINS_MAX * DOMSCORE_ROW + 4 * int(L)


def pack_domain_scores(L, header=None, table=None, res=None):
    """A domain-score block (float32) from its parts, NaN where a part is None: header (16,), table (2, 16, 32), res (4, L) - the
    inverse of the raw views of `unpack_domain_scores` (tests, restatements)."""
    L = int(L)
    block = np.full(domain_score_floats(L), np.nan, dtype=np.float32)
    at = DOMSCORE_HEADER + 2 * DOMAINS_MAX * DOMSCORE_ROW
    if header is not None:
        block[:DOMSCORE_HEADER] = np.asarray(header, dtype=np.float32).reshape(DOMSCORE_HEADER)
    if table is not None:
        block[DOMSCORE_HEADER:at] = np.asarray(table, dtype=np.float32).reshape(at - DOMSCORE_HEADER)
    if res is not None:
        block[at:] = np.asarray(res, dtype=np.float32).reshape(4 * L)
    return block


def _preserved_ratio(preserved, pairs):
    return preserved / (4.0 * pairs) if pairs else float("nan")


def unpack_domain_scores(block, L):
    """A domain-score block (1040 + 4L floats, array or tensor) -> dict: domains (of the model's leg), domains_native, present
    (rows with a native residue), legs - a list of two (one without the native's leg; none for a block the library answered
    with NaN) - and the raw views header (16,), table (2, 16, 32), res (4, L).  A leg: rows, per domain a dict with the names
    of `unpack_scores` (n_pairs, rmsd, tm, gdt_ts, gdt_ha, lddt, counts, R, t) and n, size, preserved, pairs, outer_preserved,
    outer_pairs; lddt_res (L,) and deviation (L,), each residue inside and under the superposition of its own domain;
    tm_domains, the size-weighted mean of the domains' tm; lddt_intra and lddt_inter = preserved / (4 pairs) from the integer
    counts summed over the domains, inside them and leaving them (NaN without a pair)."""
    L = int(L)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != domain_score_floats(L):
        raise ValueError(f"a domain-score block of length {L} has {domain_score_floats(L)} floats, got shape {tuple(b.shape)}")
    at = DOMSCORE_HEADER + 2 * DOMAINS_MAX * DOMSCORE_ROW
    header, table, res = b[:DOMSCORE_HEADER], b[DOMSCORE_HEADER:at].reshape(2, DOMAINS_MAX, DOMSCORE_ROW), b[at:].reshape(4, L)
    out = {"domains": _whole(header[0]), "domains_native": _whole(header[1]), "present": _whole(header[2]), "legs": [],
           "header": header.copy(), "table": table.copy(), "res": res.copy()}
    for leg, D in enumerate((out["domains"], out["domains_native"])):
        if not 0 < D <= DOMAINS_MAX:
            break
        rows = []
        for d in range(D):
            h = table[leg, d]
            row = {"n": _whole(h[0]), "n_pairs": _whole(h[1])}
            for k, name in enumerate(SCORE_NAMES[1:]):
                row[name] = float(h[2 + k])
            row["counts"] = [int(v) if v == v else 0 for v in h[7:12]]
            row["R"] = h[12:21].reshape(3, 3).copy()
            row["t"] = h[21:24].copy()
            for k, name in enumerate(("preserved", "pairs", "outer_preserved", "outer_pairs", "size")):
                row[name] = _whole(h[24 + k])
            rows.append(row)
        scored = [r for r in rows if r["tm"] == r["tm"]]
        weight = sum(r["size"] for r in scored)
        out["legs"].append({
            "rows": rows, "lddt_res": res[2 * leg].copy(), "deviation": res[2 * leg + 1].copy(),
            "tm_domains": sum(r["size"] * r["tm"] for r in scored) / weight if weight else float("nan"),
            "lddt_intra": _preserved_ratio(sum(r["preserved"] for r in rows), sum(r["pairs"] for r in rows)),
            "lddt_inter": _preserved_ratio(sum(r["outer_preserved"] for r in rows), sum(r["outer_pairs"] for r in rows))})
    return out


def domain_scores_json(ds, domains=None):
    """`unpack_domain_scores` as a JSON-ready dict (the key "domain_scores" of `dmpfold --native ... --score-domains` and of
    `dmpfold-batch`): per leg ("model", "native": whose labels) the three summary figures and every domain's row - with
    `domains`, the dict of `unpack_domains` of the same prediction, its size and segment list joined from there; NaN becomes
    None."""
    out = {"domains": int(ds["domains"]), "domains_native": int(ds["domains_native"]), "present": int(ds["present"])}
    for name, leg in zip(("model", "native"), ds["legs"]):
        parse = None if domains is None else domains if name == "model" else domains.get("native")
        rows = []
        for d, r in enumerate(leg["rows"]):
            js = {"domain": d, "size": int(r["size"]), "n": int(r["n"])}
            if parse is not None and d < len(parse["table"]):
                js["segments"] = [list(seg) for seg in parse["table"][d]["segment_list"]]
            for key in SCORE_NAMES[1:]:
                js[key] = _num(r[key])
            js["counts"] = [int(c) for c in r["counts"]]
            for key in ("preserved", "pairs", "outer_preserved", "outer_pairs"):
                js[key] = int(r[key])
            rows.append(js)
        out[name] = {"tm_domains": _num(leg["tm_domains"]), "lddt_intra": _num(leg["lddt_intra"]), "lddt_inter": _num(leg["lddt_inter"]),
                     "rows": rows}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# option "flex" (include/dmpfold_hip.h): the Gaussian network model of the final C-alpha trace and, with a whole native, of the
# native's - contacts, degrees, the eight lowest eigenpairs of the Kirchhoff matrix and the slow-mode fluctuation.  Hinges,
# collectivities, the correlations with the confidence and with the native and the agreement with the domain parse are
# formed here in float64.
# ---------------------------------------------------------------------------------------------------------------------
FLEX_HEADER = 16                     # floats in front of the two legs' headers of the flex block
FLEX_LEG = 16                        # floats of a leg's header
FLEX_MODES = 8                       # eigenpairs per leg
FLEX_FIELDS = ("contacts", "sigma", "components", "used")


def flex_floats(L):
    """Floats of the flex block (option "flex") of a prediction of length L: 16 + 2 x 16 + 2 x (2 + 8) L."""
    return FLEX_HEADER + 2 * FLEX_LEG + 2 * (2 + FLEX_MODES) * int(L)


def flex_cut_mA(cutoff):
    """A contact cutoff in Angstrom as option "flex_cut_mA" (4 .. 20 A); ValueError for anything else."""
    mA = int(round(float(cutoff) * 1000.0)) if cutoff == cutoff else -1
    if not 4000 <= mA <= 20000:
        raise ValueError(f"the flex cutoff must be 4 .. 20 Angstrom, got {cutoff!r}")
    return mA


def pack_flex(L, cut_mA=7300, legs=()):
    """A flex block from its parts (one dict per leg: contacts, sigma, components, used, eigenvalues (8,), degree (L,), msf (L,),
    modes (8, L); one leg = no native: zeros and NaN in its place, as the library writes them): the inverse of the raw views of
    `unpack_flex` (tests, restatements)."""
    L = int(L)
    b = np.zeros(flex_floats(L), dtype=np.float32)
    b[0], b[1], b[2] = L, cut_mA, 1.0 if len(legs) > 1 else 0.0
    res = FLEX_HEADER + 2 * FLEX_LEG
    b[res + (2 + FLEX_MODES) * L * len(legs):] = np.nan
    for e, leg in enumerate(legs):
        h = b[FLEX_HEADER + FLEX_LEG * e:FLEX_HEADER + FLEX_LEG * (e + 1)]
        h[:4] = [leg[k] for k in FLEX_FIELDS]
        h[8:] = np.asarray(leg["eigenvalues"], dtype=np.float64).astype(np.float32)
        a = b[res + (2 + FLEX_MODES) * L * e:res + (2 + FLEX_MODES) * L * (e + 1)].reshape(2 + FLEX_MODES, L)
        a[0], a[1], a[2:] = leg["degree"], leg["msf"], leg["modes"]
    return b


def _ranks(v):
    """Ranks 0 .. n - 1 of a vector, ties sharing their mean rank."""
    v = np.asarray(v, dtype=np.float64)
    order = np.argsort(v, kind="stable")
    r = np.empty(v.size, dtype=np.float64)
    r[order] = np.arange(v.size, dtype=np.float64)
    _, inverse, counts = np.unique(v, return_inverse=True, return_counts=True)
    sums = np.zeros(counts.size, dtype=np.float64)
    np.add.at(sums, inverse, r)
    return (sums / counts)[inverse]


def flex_hinges(mode):
    """The residues i where a mode changes sign between i and i + 1; the sign is that of the float, zero counts as positive."""
    neg = np.asarray(mode) < 0
    return [int(i) for i in np.flatnonzero(neg[1:] != neg[:-1])]


def flex_collectivity(mode):
    """exp(-sum u^2 ln u^2) / L of a mode, u^2 normalised to sum 1 (Bruschweiler 1995); 1 / L .. 1."""
    u2 = np.asarray(mode, dtype=np.float64) ** 2
    total = u2.sum()
    if not total > 0:
        return float("nan")
    u2 = u2[u2 > 0] / total
    return float(np.exp(-(u2 * np.log(u2)).sum()) / np.asarray(mode).size)


def flex_parse_sides(domains_leg):
    """The two sides of the first cut of a domain parse (one leg of `unpack_domains`) as a boolean vector over the residues, or
    None where the parse has one domain or the block does not tell: a domain of level 1 is one whole side of the first cut and
    every other domain lies on the other; a parse whose both halves were split again has no such domain."""
    if domains_leg is None or domains_leg.get("domains", 0) < 2:
        return None
    labels = np.asarray(domains_leg["labels"])
    for d, row in enumerate(domains_leg["table"]):
        if row["level"] == 1:
            return labels == d
    return None


def flex_parse_agreement(mode, sides):
    """The share of residues whose sign in `mode` (zero counts as positive) agrees with the side of the first cut they lie on, the
    better of the two assignments of signs to sides: 0.5 .. 1."""
    neg = np.asarray(mode) < 0
    same = float((neg == np.asarray(sides, dtype=bool)).mean())
    return max(same, 1.0 - same)


def flex_rmsip(a, b):
    """The root mean square inner product of two sets of modes (rows), the first n = min(rows) of each: sqrt(sum (a_i . b_j)^2 / n)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = min(a.shape[0], b.shape[0])
    if n == 0:
        return float("nan")
    return float(np.sqrt(((a[:n] @ b[:n].T) ** 2).sum() / n))


def _flex_leg(header, arr, confs=None, domains_leg=None):
    """One leg's sixteen header floats and ten arrays -> its part of `unpack_flex`."""
    out = {name: _whole(v) for name, v in zip(FLEX_FIELDS, header)}
    out["eigenvalues"] = np.asarray(header[8:16], dtype=np.float64)
    out["degree"], out["msf"], out["modes"] = _count(arr[0]), np.asarray(arr[1]), np.asarray(arr[2:])
    first = min(max(out["components"], 0), FLEX_MODES)
    live = out["modes"][first:] if out["used"] > 0 else out["modes"][:0]
    out["first_mode"] = first if out["used"] > 0 else None
    out["hinges"] = flex_hinges(live[0]) if len(live) else []
    out["collectivity"] = [flex_collectivity(m) for m in live]
    mean = _mean(out["msf"])
    out["msf_norm"] = np.asarray(out["msf"], dtype=np.float64) / mean if mean > 0 else np.full(out["msf"].shape, np.nan)
    if confs is not None:
        floppy = 1.0 - np.asarray(confs, dtype=np.float64).reshape(-1)
        out["r_conf"] = _pearson(out["msf"], floppy)
        ok = (out["msf"] == out["msf"]) & (floppy == floppy)
        out["rho_conf"] = _pearson(_ranks(np.asarray(out["msf"], dtype=np.float64)[ok]), _ranks(floppy[ok])) if ok.sum() >= 2 else float("nan")
    sides = flex_parse_sides(domains_leg)
    if sides is not None and len(live):
        out["parse_agreement"] = flex_parse_agreement(live[0], sides)
    return out


def unpack_flex(block, L, confs=None, domains=None):
    """A flex block (48 + 20L floats, array or tensor) -> dict: L, cutoff (Angstrom), has_native and, of the model's leg,
    contacts, sigma, components, used, eigenvalues (8,) ascending, degree (L,) int, msf (L,), modes (8, L) and, formed here in
    float64: first_mode (the index of the first non-zero mode, None where used = 0), hinges (flex_hinges of that mode),
    collectivity (flex_collectivity of every non-zero mode), msf_norm (msf with mean 1).  `confs` (the prediction's per-residue
    confidence) adds r_conf and rho_conf, Pearson's and Spearman's correlation of msf with 1 - confidence; `domains` (the dict
    of `unpack_domains` of the same prediction) adds parse_agreement (flex_parse_agreement of the first non-zero mode with
    flex_parse_sides of the leg's parse) where the parse has two domains or more.  With a native's leg the same under "native"
    (no r_conf), plus r_msf (Pearson r of the two legs' msf) and rmsip (flex_rmsip of the two legs' non-zero modes).  A block the
    library answered with NaN (a latched fault) gives zero counts."""
    L = int(L)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] != flex_floats(L):
        raise ValueError(f"a flex block of length {L} has {flex_floats(L)} floats, got shape {tuple(b.shape)}")
    res = FLEX_HEADER + 2 * FLEX_LEG
    arr = b[res:].reshape(2, 2 + FLEX_MODES, L)
    out = {"L": _whole(b[0]), "cutoff": float(b[1]) / 1000.0}
    out.update(_flex_leg(b[FLEX_HEADER:FLEX_HEADER + FLEX_LEG], arr[0], None if confs is None else _host(confs), domains))
    out["has_native"] = _whole(b[2]) > 0
    if out["has_native"]:
        nat_domains = domains.get("native") if domains is not None and domains.get("has_native") else None
        nat = _flex_leg(b[FLEX_HEADER + FLEX_LEG:res], arr[1], None, nat_domains)
        out["native"] = nat
        out["r_msf"] = _pearson(out["msf"], nat["msf"])
        out["rmsip"] = flex_rmsip(out["modes"][out["components"]:] if out["used"] > 0 else out["modes"][:0],
                                  nat["modes"][nat["components"]:] if nat["used"] > 0 else nat["modes"][:0])
    return out


FLEX_SCALARS = ("r_conf", "rho_conf", "parse_agreement")


def flex_json(fx, arrays=False):
    """`unpack_flex` as a JSON-ready dict (the key "flex" of `dmpfold --flex` and of `dmpfold-batch --flex`): the cutoff, per leg
    the counts, the eigenvalues, the hinges, the collectivities and the correlations that are there, with a native the same under
    "native" plus r_msf and rmsip; with `arrays` also degree, msf and the modes as lists.  NaN becomes None."""
    def leg(d):
        js = {k: int(d[k]) for k in FLEX_FIELDS}
        js["eigenvalues"] = [_num(v) for v in d["eigenvalues"]]
        js["first_mode"] = d["first_mode"]
        js["hinges"] = [int(i) for i in d["hinges"]]
        js["collectivity"] = [_num(v) for v in d["collectivity"]]
        js.update({k: _num(d[k]) for k in FLEX_SCALARS if k in d})
        if arrays:
            js["degree"] = [int(v) for v in d["degree"]]
            js["msf"] = [_num(v) for v in d["msf"]]
            js["modes"] = [[_num(v) for v in row] for row in d["modes"]]
        return js
    out = {"L": int(fx["L"]), "cutoff": _num(fx["cutoff"])}
    out.update(leg(fx))
    out["has_native"] = bool(fx["has_native"])
    if fx["has_native"]:
        out["native"] = leg(fx["native"])
        out["r_msf"], out["rmsip"] = _num(fx["r_msf"]), _num(fx["rmsip"])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The blocks behind the confidences, each stated once.  A row of BLOCKS: `key` - what the host calls the block (a keyword of
# Outputs.public and Outputs.of, of a Pipeline's set_<key>); `option` - the library option that turns it on; `field` - its view
# in an `Outputs`; `name` - what its unpacked form is called wherever it is handed on (a property of predict.Engine, a field of
# predict.Prediction, a keyword of batch.write_result); `arg` - the field of a `Layout` that holds what sizes it (None or False
# = the block is off); `shape` - its floats in words; `floats`(L, that value); `unpack`(block, L, library=, seq=) - the block as a
# dict, each taking of the keywords what it needs; `json`(that dict, top=) - its JSON form.
# BLOCKS stands in the BUFFER's order, conf_layout()'s in csrc/common.h; HANDOUT is the order in which Outputs.public hands the
# blocks out and an `Outputs` holds them.  A new tail option on the host is one row here, its unpacker and its place in HANDOUT.
# ---------------------------------------------------------------------------------------------------------------------
Block = namedtuple("Block", "key option field name arg shape floats unpack json")


def _of_length(unpack):
    """An unpacker of (block, L) as a row's `unpack`."""
    return lambda block, L, **_: unpack(block, L)


def _form(to_json):
    """A JSON form of the unpacked dict alone as a row's `json`."""
    return lambda unpacked, **_: to_json(unpacked)


def _hits_of(block, L, library):
    """The search block unpacked, with the library's `names` beside `hits` and - where `unpack_search` gave `refined` - its `refine`."""
    hits = dict(unpack_search(block, L, library.lengths, library.refine), names=list(library.names))
    if "refined" in hits:
        hits["refine"] = library.refine
    return hits


BLOCKS = (
    Block("score", "score_native", "score_block", "scores", "score", "5L + 24",
          lambda L, on: score_floats(L), _of_length(unpack_scores), _form(scores_json)),
    Block("score_map", "score_map", "map_block", "map_scores", "score_map", "64 + L",
          lambda L, on: mapscore_floats(L), _of_length(unpack_map_scores), _form(map_scores_json)),
    Block("passes", "score_passes", "pass_block", "pass_scores", "passes", "16 + 8R",
          lambda L, R: pass_floats(R), lambda block, L, **_: unpack_pass_scores(block, (block.shape[0] - PASS_HEADER) // PASS_ROW),
          _form(pass_scores_json)),
    Block("ss", "assign_ss", "ss_block", "ss", "ss", "32 + 8L",
          lambda L, on: ss_floats(L), _of_length(unpack_ss), _form(ss_json)),
    Block("exposure", "exposure", "exposure_block", "exposure", "exposure", "32 + 16L",
          lambda L, on: exposure_floats(L), lambda block, L, seq=None, **_: unpack_exposure(block, L, seq=seq), _form(exposure_json)),
    Block("domains", "domains", "domains_block", "domains", "domains", "32 + 2L + 256",
          lambda L, on: domains_floats(L),
          lambda block, L, coords=None, confs=None, **_: unpack_domains(block, L, coords=coords, confs=confs), _form(domains_json)),
    Block("align", "align_structure", "align_block", "alignment", "align_m", "25 + 2L + 3m",
          align_floats, _of_length(unpack_alignment), _form(alignment_json)),
    Block("search", "search_structures", "search_block", "hits", "search", "26K + 2LK + 3M",
          lambda L, KM: search_floats(L, *KM),
          lambda block, L, library=None, **_: _hits_of(block, L, library),
          lambda hits, top=10, **_: hits_json(hits, hits["names"], top, hits.get("refine", 0))),
)
BLOCK = {row.key: row for row in BLOCKS}
# The domain-search block of option "search_domains" has no row of BLOCKS - whose rows, and their order, callers and recorded
# tables know by position: it lies in the buffer between the domain block and the align block (Layout._walk), its view is an
# attribute of an `Outputs` that `public` never hands out, and predict.Engine has its two properties beside the rows'.
DOMAIN_SEARCH = Block("search_domains", "search_domains", "domain_search_block", "domain_hits", "search_domains", "(400 + 2L)K",
                      lambda L, K: domain_search_floats(L, K),
                      lambda block, L, library=None, **_: unpack_domain_search(block, L, len(library), library.refine),
                      lambda ds, names=(), domains=None, top=10, refine=0, **_: domain_hits_json(ds, names, domains, top, refine))
# The domain-score block of option "score_domains": likewise no row of BLOCKS; it lies behind the domain-search block, in front of
# the align block.
DOMAIN_SCORES = Block("score_domains", "score_domains", "domain_score_block", "domain_scores", "score_domains", "1040 + 4L",
                      lambda L, on: domain_score_floats(L),
                      lambda block, L, **_: unpack_domain_scores(block, L),
                      lambda ds, domains=None, **_: domain_scores_json(ds, domains))
# The flex block of option "flex": likewise no row of BLOCKS; it lies behind the domain-score block, in front of the align block.
FLEX = Block("flex", "flex", "flex_block", "flex", "flex", "48 + 20L",
             lambda L, on: flex_floats(L),
             lambda block, L, confs=None, domains=None, **_: unpack_flex(block, L, confs=confs, domains=domains),
             lambda fx, arrays=False, **_: flex_json(fx, arrays))


# ---------------------------------------------------------------------------------------------------------------------
# option "msa_report" (include/dmpfold_hip.h): how deep the alignment was (Neff at three thresholds, gaps, copies, histograms
# of identity, coverage and nearest neighbour), how conserved each column is, and the raw DCA contact map ranked against the
# native by "score_map"'s definition.  Neff / L, the medians, the precisions and the correlations with the confidence are
# formed here in float64.  A "gap" is a clamped code of 20: unknown residues and gaps merge, as the network sees them.
# ---------------------------------------------------------------------------------------------------------------------
MSA_HEADER = 128                     # floats in front of the per-column arrays of the report block
MSA_COLS = 8                         # per-column arrays
MSA_HIST = 20                        # bins of a histogram
MSA_COLUMNS = ("gaps", "neff_col", "entropy", "cons", "cons_freq", "query_freq", "dca_max", "dca_partner")
MSA_HISTS = ("hist_idq", "hist_cov", "hist_nn")
MSA_NEFF = ("neff_62", "neff_80", "neff_90")
MSA_CLASSES = MAP_CLASSES          # "score_map"'s classes


def msa_report_floats(L, dca_map=False):
    """Floats of the report block (option "msa_report") of a prediction of length L: 128 + 8L, with the map (value 2) + L*L."""
    L = int(L)
    return MSA_HEADER + MSA_COLS * L + (L * L if dca_map else 0)


def pack_msa_report(L, header, columns, dca_map=None):
    """A report block from its parts: `header` a dict with N, the three neff, gap_cells, copies, query_gaps, the three histograms
    (20 each), classes (four dicts of candidates, native_contacts, h (3,), t (3,); or None), n, ln, has_dca, has_native;
    `columns` (8, L); `dca_map` (L, L) or None - the inverse of the raw views of `unpack_msa_report` (tests, restatements)."""
    L = int(L)
    b = np.zeros(msa_report_floats(L, dca_map is not None), dtype=np.float32)
    b[0], b[1] = header["N"], L
    b[2:5] = [header[k] for k in MSA_NEFF]
    b[5], b[6], b[7] = header["gap_cells"], header["copies"], header["query_gaps"]
    for k, name in enumerate(MSA_HISTS):
        b[16 + MSA_HIST * k:16 + MSA_HIST * (k + 1)] = header[name]
    for c, cls in enumerate(header.get("classes") or ()):
        o = b[76 + 12 * c:88 + 12 * c]
        o[0], o[1], o[2:5], o[5:8] = cls["candidates"], cls["native_contacts"], cls["h"], cls["t"]
    b[124], b[125] = header.get("n", 0), header.get("ln", 0)
    b[126], b[127] = header["has_dca"], header["has_native"]
    b[MSA_HEADER:MSA_HEADER + MSA_COLS * L] = np.asarray(columns, dtype=np.float32).reshape(-1)
    if dca_map is not None:
        b[MSA_HEADER + MSA_COLS * L:] = np.asarray(dca_map, dtype=np.float32).reshape(-1)
    return b


def hist_median(hist):
    """The median of a 20-bin histogram of shares as the middle of the bin that holds the (count + 1) // 2-th row; NaN if empty."""
    h = np.asarray(hist, dtype=np.int64)
    total = int(h.sum())
    if total <= 0:
        return float("nan")
    b = int(np.searchsorted(np.cumsum(h), (total + 1) // 2))
    return (b + 0.5) / float(MSA_HIST)


def _spearman(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ok = (x == x) & (y == y)
    return _pearson(_ranks(x[ok]), _ranks(y[ok])) if ok.sum() >= 2 else float("nan")


def unpack_msa_report(block, L, confs=None, seq=None):
    """A report block (128 + 8L floats, or + L*L; array or tensor) -> dict: N, L, neff_62 / neff_80 / neff_90, gap_cells, copies,
    query_gaps, hist_idq / hist_cov / hist_nn (20 ints each), has_dca, has_native, the eight per-column arrays of MSA_COLUMNS
    (gaps, cons and dca_partner as ints, -1 for NaN), the raw `header` (128,) and `columns` (8, L) and, formed here in float64: neff_per_L and neff_per_sqrtL (of neff_80),
    gap_share, median_identity, median_coverage, median_nearest.  With has_native and has_dca: n, ln and `classes` - per class of
    MSA_CLASSES candidates, native_contacts, h, t, precision (h / t) and enrichment (precision over native_contacts /
    candidates) for L/1, L/2, L/5 (NaN where a denominator is 0).  `confs` (the per-residue confidence) adds Pearson's and
    Spearman's correlation of it with neff_col, entropy and dca_max as r_conf / rho_conf dicts; `seq` (the query as a string)
    adds cons_seq, the consensus as letters ('-' in an all-gap column).  With the map (value 2) `dca_map` (L, L).  A block the
    library answered with NaN (a latched fault) gives zero counts."""
    L = int(L)
    b = _host(block)
    if b.ndim != 1 or b.shape[0] not in (msa_report_floats(L), msa_report_floats(L, True)):
        raise ValueError(f"a report block of length {L} has {msa_report_floats(L)} or {msa_report_floats(L, True)} floats, got shape {tuple(b.shape)}")
    out = {"N": _whole(b[0]), "L": _whole(b[1])}
    out.update({name: float(b[2 + k]) for k, name in enumerate(MSA_NEFF)})
    out.update(gap_cells=_whole(b[5]), copies=_whole(b[6]), query_gaps=_whole(b[7]))
    for k, name in enumerate(MSA_HISTS):
        out[name] = _count(b[16 + MSA_HIST * k:16 + MSA_HIST * (k + 1)])
    out["has_dca"], out["has_native"] = _whole(b[126]) > 0, _whole(b[127]) > 0
    cols = b[MSA_HEADER:MSA_HEADER + MSA_COLS * L].reshape(MSA_COLS, L)
    out["header"], out["columns"] = b[:MSA_HEADER], cols                   # (the raw floats: the batch's npz arrays)
    for k, name in enumerate(MSA_COLUMNS):
        v = np.asarray(cols[k])
        out[name] = np.where(v == v, v, -1.0).astype(np.int64) if name in ("gaps", "cons", "dca_partner") else v
    out["neff_per_L"] = out["neff_80"] / L if L else float("nan")
    out["neff_per_sqrtL"] = out["neff_80"] / float(np.sqrt(L)) if L else float("nan")
    cells = out["N"] * L
    out["gap_share"] = out["gap_cells"] / cells if cells else float("nan")
    out["median_identity"], out["median_coverage"] = hist_median(out["hist_idq"]), hist_median(out["hist_cov"])
    out["median_nearest"] = hist_median(out["hist_nn"])
    if out["has_native"] and out["has_dca"]:
        out["n"], out["ln"] = _whole(b[124]), float(b[125])
        out["classes"] = {}
        for c, name in enumerate(MSA_CLASSES):
            o = b[76 + 12 * c:88 + 12 * c]
            cand, nat = _whole(o[0]), _whole(o[1])
            h, t = [_whole(v) for v in o[2:5]], [_whole(v) for v in o[5:8]]
            prec = [hh / tt if tt else float("nan") for hh, tt in zip(h, t)]
            base = nat / cand if cand else float("nan")
            out["classes"][name] = {"candidates": cand, "native_contacts": nat, "h": h, "t": t, "precision": prec,
                                    "enrichment": [p / base if base == base and base > 0 else float("nan") for p in prec]}
    if confs is not None:
        cf = _host(confs).reshape(-1)[:L]
        out["r_conf"] = {k: _pearson(cf, out[k]) for k in ("neff_col", "entropy", "dca_max")}
        out["rho_conf"] = {k: _spearman(cf, out[k]) for k in ("neff_col", "entropy", "dca_max")}
    if seq is not None:
        out["seq"] = str(seq)
        out["cons_seq"] = "".join(AA1[c] if 0 <= c < 20 else "-" for c in out["cons"])
    if b.shape[0] == msa_report_floats(L, True):
        out["dca_map"] = b[MSA_HEADER + MSA_COLS * L:].reshape(L, L)
    return out


def msa_report_json(rep, arrays=False):
    """`unpack_msa_report` as a JSON-ready dict (the key "msa" of `dmpfold --msa-report` and of `dmpfold-batch --msa-report`):
    the depth figures, the histograms, the flags, the classes and correlations that are there; with `arrays` also the eight
    per-column arrays as lists.  The map is never part of it (it goes to a .npy file).  NaN becomes None."""
    js = {"N": int(rep["N"]), "L": int(rep["L"])}
    js.update({k: _num(rep[k]) for k in MSA_NEFF + ("neff_per_L", "neff_per_sqrtL", "gap_share", "median_identity", "median_coverage",
                                                     "median_nearest")})
    js.update({k: int(rep[k]) for k in ("gap_cells", "copies", "query_gaps")})
    js.update({k: [int(v) for v in rep[k]] for k in MSA_HISTS})
    js["has_dca"], js["has_native"] = bool(rep["has_dca"]), bool(rep["has_native"])
    js["mean_entropy"], js["mean_neff_col"] = _num(_mean(rep["entropy"])), _num(_mean(rep["neff_col"]))
    if "classes" in rep:
        js["n"], js["ln"] = int(rep["n"]), _num(rep["ln"])
        js["classes"] = {name: {k: ([_num(x) for x in v] if isinstance(v, list) else int(v)) for k, v in cls.items()}
                         for name, cls in rep["classes"].items()}
    for k in ("r_conf", "rho_conf"):
        if k in rep:
            js[k] = {name: _num(v) for name, v in rep[k].items()}
    if "cons_seq" in rep:
        js["cons_seq"] = rep["cons_seq"]
    if arrays:
        for name in MSA_COLUMNS:
            js[name] = [(int(v) if v >= 0 else None) if name in ("gaps", "cons", "dca_partner") else _num(v) for v in rep[name]]
    return js


# The report block of option "msa_report": likewise no row of BLOCKS; it lies behind the flex block, in front of the align block.
MSA_REPORT = Block("msa_report", "msa_report", "msa_report_block", "msa_report", "msa_report", "128 + 8L (+ L*L)",
                   lambda L, value: msa_report_floats(L, value == 2),
                   lambda block, L, confs=None, seq=None, **_: unpack_msa_report(block, L, confs=confs, seq=seq),
                   lambda rep, arrays=False, **_: msa_report_json(rep, arrays))
