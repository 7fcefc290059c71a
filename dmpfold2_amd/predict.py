"""Host-side mirror of the reference's prediction interface on the HIP engine.

`aln_to_coords` and `run_dmpfold` keep the names, argument meaning, return types and
error behaviour of the reference (dmpfold/predict.py:74-158 and 160-208); all
arithmetic happens in libdmpfold_hip.so through the C ABI of include/dmpfold_hip.h.
PyTorch is used only for device memory and the current stream.

Differences from the reference, all additive or forced by the environment:
  * there is no CPU path: `device` must name a GPU ("cuda", "cuda:1", an int, or a
    torch.device).  The default is "cuda" (the reference defaults to "cpu");
  * `aln_to_coords` synchronises with the GPU before it returns and checks the engine's device-side
    fault word: a prediction whose activations left the range of the default split-f16 convolution is
    re-run with the range-free bf16 split (a note goes to stderr), any other fault raises;
  * packed weights are cached per (device, weights file) instead of being rebuilt on
    every call (the reference constructs and loads a fresh network each time);
  * eigenvector signs of the MDS step follow a fixed rule (see include/dmpfold_hip.h);
  * missing trained weights raise FileNotFoundError (no download: predict.py:64-71);
  * `converge` (Angstrom, None / 0 = off, the default): recycling stops after the first pass that moves the seed
    distance map by no more than that (RMS); the result is then the one `iterations` = that pass would have given;
  * `distmap` / `return_distmap` / `dmpfold --distmap FILE`: the predicted C-alpha distance map of the pass the best-of
    rule chose (option "emit_distmap" of include/dmpfold_hip.h) comes back with the structure;
  * `native` / `return_scores` / `dmpfold --native PDB`: the model is scored against a native structure on the GPU
    (option "score_native": TM-score, GDT, RMSD, lDDT-C-alpha; dmpfold2_amd/score.py has the host side);
  * `compare` / `return_alignment` / `dmpfold --compare PDB`: the model is aligned on the GPU with a structure of any length
    and sequence (option "align_structure": a structural alignment, both TM-scores, the superposition);
  * `restrain` / `return_restrain` / `dmpfold -r K`: the final minimisation also pulls the model towards the predicted
    distance map (options "restrain_milli" / "restrain_cut_mA"; the reference's minimiser never sees the map).

Plumbing: a public method gathers what its call asks for besides the prediction into one `Extras` in its first lines and
everything below it carries that record; the caller's `d_conf` buffer is described by one `score.Layout`, made in `_stage`
from the options as the context holds them (`Flags`), which also cuts the buffer into the views of an `Outputs`.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import inspect
import json
import os
import sys
import threading
import time
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from . import score as _score
from .score import Layout, Outputs, distmap_floats, split_conf_buffer, split_distmap_buffer    # noqa: F401 (re-exports)

default_device = "cuda"
default_iterations = 10
default_minsteps = 100

MAX_SEQS = 3000     # predict.py:130-132
MAX_L = 2048        # include/dmpfold_hip.h DMP_MAX_L (the reference has no limit)

_RESNAMES = {0: "ALA", 1: "ARG", 2: "ASN", 3: "ASP", 4: "CYS", 5: "GLN", 6: "GLU", 7: "GLY",
             8: "HIS", 9: "ILE", 10: "LEU", 11: "LYS", 12: "MET", 13: "PHE", 14: "PRO",
             15: "SER", 16: "THR", 17: "TRP", 18: "TYR", 19: "VAL"}


# ---------------------------------------------------------------------------
# host-side parsing (pure Python / C-ABI host helper, no GPU needed)
# ---------------------------------------------------------------------------
def read_aln(input_file):
    """Lines not starting with '>', right-stripped (predict.py:100-104)."""
    rows = []
    with open(input_file, "r") as fh:
        for line in fh.readlines():
            if not line.startswith(">"):
                rows.append(line.rstrip())
    return rows


def read_a3m(input_file):
    """An .a3m alignment as .aln rows: the reference README's conversion
    `egrep -v "^>" x.a3m | sed 's/[a-z]//g' > x.aln` (drop header lines and the lower-case insert
    columns), done in memory."""
    rows = []
    with open(input_file, "r") as fh:
        for line in fh.readlines():
            if not line.startswith(">"):
                rows.append("".join(ch for ch in line.rstrip() if not ("a" <= ch <= "z")))
    return rows


def encode_aln(rows):
    """Residue letters -> uint8 codes (N, L), capped at 3000 rows (predict.py:124-132).
    Ragged input raises ValueError from the reshape, as in the reference.  A character outside the
    alignment alphabet (lower-case a3m inserts, digits ...) maps to a code above 21, which the
    reference's 22-row embedding rejects with IndexError (network.py:223): raised here, for the
    rows that survive the 3000-row cap, as the reference would."""
    nseqs = len(rows)
    length = len(rows[0])
    text = np.frombuffer("".join(rows).encode("latin-1"), dtype=np.uint8)
    codes = np.empty_like(text)
    lib = _lib.load()
    _lib.check(lib.dmp_msa_encode(text.ctypes.data, text.size, codes.ctypes.data))
    alnmat = codes.reshape(nseqs, length)
    if nseqs > MAX_SEQS:
        alnmat = alnmat[:MAX_SEQS]
    if alnmat.size and int(alnmat.max()) > 21:
        raise IndexError("index out of range in self")
    return alnmat


def read_template_ca(template):
    """CA atoms of ATOM records, fixed PDB columns (predict.py:106-117)."""
    xyz = []
    with open(template, "r") as fh:
        for line in fh:
            if line[:4] == "ATOM" and line[12:16] == " CA ":
                xyz.append(np.array([float(line[30:38]), float(line[38:46]), float(line[46:54])],
                                    dtype=np.float32))
    return np.asarray(xyz, dtype=np.float32).reshape(-1, 3)


def _resolve_device(device):
    dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    if dev.type != "cuda":
        raise RuntimeError(
            f"dmpfold2_amd runs on AMD GPUs only (got device '{device}'); there is no CPU path")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible to PyTorch-ROCm; dmpfold2_amd has no CPU fallback")
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


def default_weight_files():
    modeldir = os.path.join(os.path.dirname(os.path.realpath(__file__)), "trained_model")
    return [os.path.join(modeldir, f"FINAL_fullmap_e2e_model_part{p}.pt") for p in ("1", "2")]


def load_state_dict(weights_file=None):
    """The reference's weight files: one pickled state_dict, or the two-part default that is
    merged with dict.update (predict.py:81-96)."""
    if weights_file is None:
        parts = default_weight_files()
        if not os.path.isfile(parts[0]):
            raise FileNotFoundError(
                f"trained model not found at {parts[0]}; the reference would download it, this "
                "build does not: place the two FINAL_fullmap_e2e_model_part*.pt files there or "
                "pass weights_file=/-w")
        sd = torch.load(parts[0], map_location="cpu", weights_only=True)
        sd.update(torch.load(parts[1], map_location="cpu", weights_only=True))
    else:
        # weights_only: a user-supplied -w file is data (a tensor dict), never unpickled code
        sd = torch.load(weights_file, map_location="cpu", weights_only=True)
    return sd


def converge_to_mA(converge):
    """The convergence tolerance of the Python / CLI boundary (Angstrom, float, None = off) as the C option's integer
    number of milli-Angstrom ("recycle_tol_mA", include/dmpfold_hip.h).  Negative or non-finite values raise ValueError."""
    if converge is None:
        return 0
    tol = float(converge)
    if not (tol >= 0.0) or tol == float("inf"):
        raise ValueError(f"converge must be a finite tolerance >= 0 (Angstrom), got {converge!r}")
    return int(round(tol * 1000.0))


def restrain_to_milli(restrain):
    """The restraint force constant K of the Python / CLI boundary (float, None = off) as the C option's integer
    ("restrain_milli", include/dmpfold_hip.h: K * 1000).  Negative, non-finite or > 100 raises ValueError."""
    if restrain is None:
        return 0
    k = float(restrain)
    if not 0.0 <= k <= 100.0:                   # (false for NaN)
        raise ValueError(f"restrain must be a finite force constant in 0 .. 100, got {restrain!r}")
    return int(round(k * 1000.0))


def restrain_cutoff_to_mA(cutoff):
    """The restraint cutoff (Angstrom, 0 .. 100) as the integer of option "restrain_cut_mA"; ValueError for the rest."""
    a = float(cutoff)
    if not 0.0 <= a <= 100.0:
        raise ValueError(f"restrain_cutoff must be a finite distance in 0 .. 100 Angstrom, got {cutoff!r}")
    return int(round(a * 1000.0))


def restrain_options(restrain, cutoff=15.0):
    """What a call's `restrain` / `restrain_cutoff` ask of the two options: None (`restrain` None: leave them as they
    stand) or (restrain_milli, restrain_cut_mA).  A bad value raises ValueError - before any work."""
    return None if restrain is None else (restrain_to_milli(restrain), restrain_cutoff_to_mA(cutoff))


def restrain_report(k, cutoff, steps, distmap, map_rms, coords):
    """The report of a restrained prediction (the JSON line `dmpfold --restrain` writes under the key "restrain"): k,
    cutoff, steps and map_rms as given, and - formed here in NumPy from the returned map (L, L) and coordinates (L, 5, 3) -
    restrained_pairs (pairs i < j, |i - j| >= 2, map below the cutoff), clashes (such pairs closer than 3.0 A in the final
    trace) and bond_dev_max (max |d(i, i + 1) - 3.78|).  What to look at on a map no chain can realise: the restraints then
    buy map agreement with clashes and stretched bonds."""
    def host(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    ca = host(coords).reshape(-1, 5, 3)[:, 1].astype(np.float64)
    L = ca.shape[0]
    d = np.sqrt(((ca[:, None, :] - ca[None, :, :]) ** 2).sum(-1))
    far = np.triu(np.ones((L, L), dtype=bool), 2)
    pairs = None
    if distmap is not None:
        with np.errstate(invalid="ignore"):
            pairs = int((host(distmap).astype(np.float32)[far] < np.float32(cutoff)).sum())
    return {"k": float(k), "cutoff": float(cutoff), "steps": int(steps),
            "map_rms": None if map_rms is None else float(map_rms), "restrained_pairs": pairs,
            "clashes": int((d[far] < 3.0).sum()),
            "bond_dev_max": float(np.abs(d[np.arange(L - 1), np.arange(1, L)] - 3.78).max())}


def save_distmap_npy(path, distmap):
    """The (L, L) map as a float32 .npy file (what `dmpfold --distmap` and `dmpfold-batch --distmap` write)."""
    arr = distmap.detach().cpu().numpy() if isinstance(distmap, torch.Tensor) else np.asarray(distmap)
    with open(path, "wb") as fh:           # an open file: np.save would append ".npy" to a name without it
        np.save(fh, np.ascontiguousarray(arr, dtype=np.float32))


def _tolerance_arg(text):
    """argparse type of -c / --converge: a float >= 0."""
    try:
        tol = float(text)
        converge_to_mA(tol)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a tolerance >= 0 (Angstrom)")
    return tol


def _restrain_arg(text):
    """argparse type of -r / --restrain: a float in 0 .. 100."""
    try:
        k = float(text)
        restrain_to_milli(k)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a force constant in 0 .. 100")
    return k


def _cutoff_arg(text):
    """argparse type of --restrain-cutoff: a float in 0 .. 100 (Angstrom)."""
    try:
        a = float(text)
        restrain_cutoff_to_mA(a)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a cutoff in 0 .. 100 (Angstrom)")
    return a


def add_restrain_arguments(parser, *flags):
    """--restrain K [--restrain-cutoff A] of `dmpfold` (with -r) and `dmpfold-batch`."""
    parser.add_argument(*flags, "--restrain", type=_restrain_arg, default=None, required=False, metavar="K",
                        help="restrain the final minimisation to the predicted distance map with force constant K (0 .. 100; the "
                             "reference has no such term): pairs at least two residues apart whose predicted distance lies below "
                             "the cutoff are pulled towards it; a report (map_rms, restrained pairs, clashes, largest bond "
                             "deviation) goes to standard error as one JSON line; default: the reference's minimisation")
    parser.add_argument("--restrain-cutoff", type=_cutoff_arg, default=15.0, required=False, metavar="A",
                        help="with --restrain: only predicted distances below A Angstrom restrain (default 15)")


# device-side fault bits (include/dmpfold_hip.h, DMP_FAULT_*)
FAULT_SEQ_HANDOFF, FAULT_F16_RANGE, FAULT_REFINE_HANDOFF, FAULT_BAD_CODE, FAULT_EIG_HANDOFF, FAULT_VGRU_HANDOFF = 1, 2, 4, 8, 16, 32


class DeviceFault(_lib.DmpError):
    """A device-side fault invalidated a prediction (its outputs are NaN)."""

    def __init__(self, bits):
        self.bits = int(bits)
        what = [txt for bit, txt in ((FAULT_SEQ_HANDOFF, "sequence-GRU workgroup hand-off timed out"),
                                     (FAULT_REFINE_HANDOFF, "minimiser workgroup hand-off timed out"),
                                     (FAULT_EIG_HANDOFF, "tridiagonalisation workgroup hand-off timed out"),
                                     (FAULT_VGRU_HANDOFF, "vertical-GRU row barrier timed out"),
                                     (FAULT_F16_RANGE, "an activation left the f16 range of the "
                                      "split-product convolution (conv_mode 2 has no range limit)"))
                if bits & bit]
        super().__init__("device-side fault (results invalid): " + "; ".join(what))


def raise_for_faults(bits):
    if bits & FAULT_BAD_CODE:
        raise IndexError("index out of range in self")      # the embedding lookup of network.py:223
    if bits:
        raise DeviceFault(bits)


# ---------------------------------------------------------------------------
# engine: one dmp_ctx per GPU
# ---------------------------------------------------------------------------
def _env_precision():
    """DMPFOLD_PRECISION selects the arithmetic (option "precision" of include/dmpfold_hip.h) for the drop-in entry points -
    aln_to_coords, the CLI, the batch front end - which have no argument for it:
      2  full-width operands on the 16-bit matrix cores: the float32 operands of the convolutions and of the vertical GRU
         as three exact bf16 pieces (24 significand bits, six products);
      1  the reference's instructions: float32 matrix-core convolutions and vertical GRU (about half the speed of 2);
      0  the fast mode: two f16 pieces per operand (22-23 significand bits), about 1.8 x the speed of 2.
    Unset = the library's default."""
    v = os.environ.get("DMPFOLD_PRECISION", "").strip()
    if v == "":
        return None
    if v not in ("0", "1", "2"):
        raise ValueError(f"DMPFOLD_PRECISION must be 0, 1 or 2, got {v!r}")
    return int(v)


# What the reference's own entry points compute in is float32 (predict.py:136 `.float()`, network.py:25-31), so a context
# - through the C ABI, an `Engine`, a `Pipeline`, aln_to_coords, the CLI, the batch front end - starts in the setting whose
# operands carry float32's 24 significand bits at the 16-bit matrix cores' rate (option "precision" = 2).
# DMPFOLD_PRECISION=0 selects the fast 22-23-bit mode (about 1.8 x the speed), 1 the f32 matrix-core instructions.
DROP_IN_PRECISION = 2


def drop_in_precision():
    v = _env_precision()
    return DROP_IN_PRECISION if v is None else v


# What one call asks for besides the prediction itself, as `Engine.predict` documents each: `distmap` (return the map),
# `native` (score against it), `structure` (align with it), `library` (search it), `score_map` (score the map),
# `score_passes` (score every recycling pass), `ss` (assign secondary structure) and `exposure` (solvent exposure of the
# backbone).  The public methods build one in their first line (`_asked`); everything below them takes and carries the record.
Extras = namedtuple("Extras", "distmap native structure library score_map score_passes ss exposure",
                    defaults=(False, None, None, None, False, False, False, False))


def _asked(call):
    """The locals of a public predict method -> (Extras, what restrain_options makes of its `restrain`, `restrain_cutoff`)."""
    return Extras(*(call[field] for field in Extras._fields)), restrain_options(call["restrain"], call["restrain_cutoff"])


# What a call sets for its duration: (field of `Extras`, option), in the order they are set - an option behind what it needs.
# `native` and `structure` are inputs (None = not given), the rest flags; CALL_CHECKS: what must hold of an input before
# anything changes.  Convergence, the restraint and the library have arguments of their own: Engine._call_options.
CALL_OPTIONS = (("distmap", "emit_distmap"), ("score_map", "score_map"), ("native", "score_native"),
                ("score_passes", "score_passes"), ("ss", "assign_ss"), ("exposure", "exposure"), ("structure", "align_structure"))
CALL_INPUTS = {"native": lambda L: np.full((L, 3), np.nan, dtype=np.float32),      # an input -> the value that means "none"
               "structure": lambda L: np.zeros((0, 3), dtype=np.float32)}
CALL_CHECKS = {"structure": _score.as_structure}

# What an option needs on beside itself (the library looks at them together when a prediction begins).  "score_native" comes
# with a native only: an option that needs it asks for one (`needs_native`) where none is given.
NEEDS = {"score_map": ("emit_distmap", "score_native"), "score_passes": ("score_native",), "restrain_milli": ("emit_distmap",)}
NATIVE_NEEDED = {"score_map": "scores the distance map{s}", "score_passes": "scores every pass"}
# (option "score_domains" is no field of a call's `Extras` and no flag of the parsers' loops over NATIVE_NEEDED: its text stands alone)
SCORE_DOMAINS_NEEDS_NATIVE = "score_domains scores every domain against a native structure: give `native`"
_BLOCK_OF = {row.option: row for row in _score.BLOCKS}


def needs_native(option, spelt, give, many=False):
    """The text of the error for `option` (spelt as its caller spells it) asked for without a native (`give`: what to give)."""
    return (f"{spelt} {NATIVE_NEEDED[option].format(s='s' if many else '')} against "
            + ("native structures" if many else "a native structure") + f": give {give}")


# The options that decide the layout of a `d_conf` buffer, in the order of a row of `agree_options`.
LAYOUT_OPTIONS = ("emit_distmap", "score_native", "score_map", "align_structure", "search_structures")
# The options that own one block and need nothing, by the key of their row in score.BLOCKS: a field of `Flags` and of a
# `Layout`, a Pipeline's set_<key>; the engines of a pipeline must agree on each (`agree`).
OWN_BLOCK = ("ss", "exposure")

# The layout options as one prediction runs with them: `emit` .. `align` bools, `search` the K of "search_structures";
# `alloc`: size the buffer as if "emit_distmap" were on (a pipeline whose engines disagree on that option alone);
# `max_L`: the context's, for the rule of B0; `passes`: the rows R of the pass block of "score_passes" (None = off), which
# follow the prediction's own depth; `ss`: option "assign_ss" on; `exposure`: option "exposure" on.
Flags = namedtuple("Flags", "emit alloc score score_map align search max_L passes ss exposure", defaults=(None, None, False, False))


def agree(values, option, setter):
    """A field of a prediction's Flags from an option that owns one block, as every engine that may run the prediction holds
    it: they must agree - RuntimeError if not."""
    values = [bool(v) for v in values]
    if any(v != values[0] for v in values):
        raise RuntimeError(f"the engines must agree on \"{option}\" (the blocks behind its block move with it); use {setter}")
    return values[0]


def domains_options(tau=0.25, min_size=40, min_segment=10):
    """The three parameters of option "domains" as the library takes them -> (tau_milli, min_size, min_segment): `tau` (the
    largest ext / (min(int_A, int_B) + ext) that still splits, 0.001 .. 1) in thousandths, `min_size` 8 .. 1024 residues,
    `min_segment` 1 .. 64 residues and no more than `min_size` - ValueError otherwise."""
    milli = int(round(float(tau) * 1000.0))
    if not (tau == tau) or not 1 <= milli <= 1000:
        raise ValueError(f"domains: tau must be in [0.001, 1], got {tau}")
    if not 8 <= int(min_size) <= 1024:
        raise ValueError(f"domains: min_size must be 8 .. 1024, got {min_size}")
    if not 1 <= int(min_segment) <= 64 or int(min_segment) > int(min_size):
        raise ValueError(f"domains: min_segment must be 1 .. 64 and at most min_size = {min_size}, got {min_segment}")
    return milli, int(min_size), int(min_segment)


DOMAINS_OPTIONS = ("domains_tau_milli", "domains_min_size", "domains_min_segment")


def agree_ss(values, option="assign_ss", setter="set_ss"):
    """`agree` for option "assign_ss" (the name and signature callers know)."""
    return agree(values, option, setter)


def _own_blocks(engines):
    """{key: `agree` over the engines} of every OWN_BLOCK option."""
    return {key: agree([e.get_option(_score.BLOCK[key].option) for e in engines], _score.BLOCK[key].option, "set_" + key)
            for key in OWN_BLOCK}


def agree_passes(values, score, iterations):
    """The `passes` of a prediction's Flags from option "score_passes" as every engine that may run it holds it: they must
    agree, and the option needs "score_native" (`score`) - RuntimeError if not.  -> R = score.pass_rows(iterations), or None."""
    values = [bool(v) for v in values]
    if any(v != values[0] for v in values) or (values[0] and not score):
        raise RuntimeError("the engines must agree on \"score_passes\", and it needs \"score_native\" on; use set_score_passes")
    return _score.pass_rows(iterations) if values[0] else None



def agree_options(rows):
    """The one rule for the engines of a pipeline, which share a buffer whichever of them runs a target.  `rows`: per engine
    the values of LAYOUT_OPTIONS.  Where nothing beyond the map is on anywhere the engines may differ in "emit_distmap": the
    buffer is then sized for the map (`alloc`) and only the confidences are handed out (`emit`).  Otherwise every engine must
    hold the same five values, and "score_map" needs "emit_distmap" and "score_native" on: RuntimeError if not.  -> Flags."""
    rows = [tuple(bool(v) for v in r[:4]) + (int(r[4]),) for r in rows]
    if any(any(r[1:]) for r in rows):
        emit, score, score_map = rows[0][:3]
        if any(r != rows[0] for r in rows) or (score_map and not (emit and score)):
            raise RuntimeError("the engines of a pipeline must agree on \"emit_distmap\", \"score_native\", \"score_map\", "
                               "\"align_structure\" and \"search_structures\" (where each block lies in the buffer depends on "
                               "those in front of it), and \"score_map\" needs \"emit_distmap\" and \"score_native\" on; use "
                               "set_distmap / set_score / set_score_map / set_align / set_search")
    emits = [r[0] for r in rows]
    return Flags(all(emits), any(emits), *rows[0][1:])


def _stage(device, L, template_ca, flags, extras, domains=False, search_domains=False, score_domains=False, flex=False, msa_report=0):
    """What a prediction of length L needs on the GPU besides its alignment: (template CA trace (L, 3) or None, Outputs).
    The `d_conf` buffer behind the Outputs is laid out (score.Layout) for the options as the context holds them (`flags`) -
    the library cannot check it - and its input blocks are filled from `extras`: with "score_native" on the native trace (no
    `native` = no row present: n_pairs 0, NaN scores); with "align_structure" on m and the rows of `structure` (none: m = 0,
    which the library answers with NaN); with "search_structures" on the search block from the library's copy on the GPU.
    `domains`: option "domains" on (it travels beside `flags`, whose fields callers know by position); `search_domains`: option
    "search_domains" on - the buffer then holds the domain-search block in front of the align block; `score_domains`: option
    "score_domains" on - the domain-score block behind that; `flex`: option "flex" on - the flex block behind that; `msa_report`: the value of option
    "msa_report" - the report block behind that."""
    d_tpl = None
    if template_ca is not None:
        d_tpl = torch.as_tensor(template_ca, dtype=torch.float32).reshape(-1, 3).to(device).contiguous()
        if d_tpl.shape[0] != L:
            raise RuntimeError(f"Sizes of tensors must match: template has {d_tpl.shape[0]} CA atoms, "
                               f"alignment has {L} columns")
    coords = torch.empty((L, 5, 3), dtype=torch.float32, device=device)
    ablock = None
    if flags.align:
        ablock = _score.pack_structure(extras.structure, L) if extras.structure is not None else _score.empty_structure(L)
    library = extras.library if flags.search else None
    align_m = None if ablock is None else (ablock.shape[0] - _score.align_floats(L, 0)) // 3
    lay = Layout(L, flags.emit, flags.score, flags.score_map, align_m, None if library is None else (len(library), library.rows),
                 flags.max_L, flags.passes, domains=domains, search_domains=search_domains and library is not None, score_domains=score_domains, flex=flex, msa_report=msa_report,
                 **{key: getattr(flags, key) for key in OWN_BLOCK})
    floats = max(lay.total, lay._replace(distmap=flags.alloc).total)
    out = lay.split(torch.empty((floats,), dtype=torch.float32, device=device), coords)
    if library is not None:
        library.fill_block(out.search_block, L)
    if flags.align:
        out.align_block.copy_(torch.from_numpy(ablock))
    if flags.score:
        native = extras.native
        block = _score.pack_native(*_score.as_native(native, L), L) if native is not None else _score.empty_native(L)
        out.score_block.copy_(torch.from_numpy(block))
    return d_tpl, out


# The last prediction of an engine: its Outputs (without the coordinates), its length and the library it searched.
# `coords`: the coordinates, kept only where an unpacker reads them (the domains' radii of gyration).
_Last = namedtuple("_Last", "out L library coords", defaults=(None,))


class Engine:
    """Owns one `dmp_ctx` (device buffers + packed weights) on one GPU."""

    def __init__(self, device, max_L, max_N, stream=None, precision=None):
        self.lib = _lib.load()
        self.device = _resolve_device(device)
        self.max_L = int(max_L)
        self.max_N = int(min(max_N, MAX_SEQS))
        self._stream = stream          # optional torch.cuda.Stream owned by this engine
        self._ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dmp_ctx_create(self.device.index, self.max_L, self.max_N,
                                               C.byref(self._ctx)))
        self.weights_tag = None
        self.last_fallback = False     # the last predict_*_checked call fell back to conv_mode 2
        self._forget_last()
        prec = precision if precision is not None else _env_precision()
        if prec is not None:
            self.set_option("precision", prec)

    def close(self):
        if self._ctx:
            self.lib.dmp_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        return self._ctx

    @property
    def device_bytes(self):
        return self.get_option("device_mib") << 20

    def stream(self):
        s = self._stream if self._stream is not None else torch.cuda.current_stream(self.device)
        return C.c_void_p(s.cuda_stream)

    def set_weights(self, state_dict, tag=None):
        """Strict load like load_state_dict (predict.py:98): unknown, missing or mis-shaped
        tensors raise RuntimeError."""
        for key, val in state_dict.items():
            arr = np.ascontiguousarray(
                val.detach().cpu().float().numpy() if isinstance(val, torch.Tensor) else val,
                dtype=np.float32)
            shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
            _lib.check(self.lib.dmp_weights_set(self._ctx, key.encode(), arr.ctypes.data, shape,
                                                arr.ndim), RuntimeError)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dmp_weights_finalize(self._ctx), RuntimeError)
        self.weights_tag = tag

    def share_weights(self, other):
        """Use the packed weights of `other` (an engine on the same GPU) instead of packing a copy."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dmp_weights_share(self._ctx, other.ctx), RuntimeError)
        self.weights_tag = other.weights_tag

    def predict(self, alnmat, template_ca=None, iterations=default_iterations,
                minsteps=default_minsteps, converge=None, distmap=False, native=None, structure=None, library=None,
                score_map=False, score_passes=False, ss=False, restrain=None, restrain_cutoff=15.0, exposure=False):
        """codes (N, L) uint8 -> (coords (L,5,3), confs (L,)) float32 tensors on the GPU.
        `ss`: secondary structure is assigned to the final backbone on the GPU from its hydrogen bonds (option "assign_ss", set
        for this call only) and, with `native` given whole (no NaN row), to the native's backbone rebuilt from its trace; what
        the call returns does not change, the result is in `ss` (score.unpack_ss) and `ss_block`.
        `exposure`: the solvent exposure of the final backbone is counted on the GPU - exposed sphere points per atom, half-sphere
        exposure and CB contact number per residue (option "exposure", set for this call only) - and, with `native` given whole,
        that of the native's rebuilt backbone; what the call returns does not change, the result is in `exposure`
        (score.unpack_exposure) and `exposure_block`.
        `restrain` (force constant K, 0 .. 100; None = the engine's "restrain_milli" option as it stands, 0 by default) and
        `restrain_cutoff` (Angstrom): the `minsteps` steps of the FINAL refinement also pull every pair at least two residues
        apart whose predicted distance lies below the cutoff towards it (options "restrain_milli" / "restrain_cut_mA", set for
        this call only together with "emit_distmap" - the reference has no such term); what the call returns does not change
        in shape, the report (map_rms, restrained pairs, clashes, largest bond deviation) is in `restrain`.
        `score_passes` (needs `native`): every recycling pass's trace - not only the one the best-of rule kept - is scored
        against the native on the GPU (option "score_passes", set for this call only together with "score_native"), with
        its mean confidence logit and its convergence delta beside the scores; what the call returns does not change, the
        table is in `pass_scores`.
        `score_map` (needs `native`): the chosen pass's predicted distance map is scored against the native too (option
        "score_map", set for this call only together with "emit_distmap" and "score_native"): contact precision of the top
        L, L/2 and L/5 per separation class and the map's own distance agreement; what the call returns does not change,
        the result is in `map_scores`.
        `library` (a score.Library of K structures, each 3 .. max_L rows): the final trace is aligned with every one of them on
        the GPU (option "search_structures", set for this call only, "search_max_m" = the longest entry); what the call
        returns does not change, the results and the ranking are in `hits`.
        `structure` (an (m, 3) array, the C-alpha trace of a structure of any length, 3 <= m <= max_L): the final trace is
        aligned with it on the GPU (option "align_structure", set for this call only); what the call returns does not
        change, the result is in `alignment`.
        `native` (an (L, 3) array, one native C-alpha per alignment column, NaN rows where there is none, or a tuple
        (array, lnorm); score.native_rows makes one from a structure): the model is scored against it on the GPU (option
        "score_native", set for this call only); what the call returns does not change, the scores are in `scores`.
        `distmap=True` returns (coords, confs, distmap (L, L), info (3,)): the chosen pass's predicted distance map and
        [best_pass, passes_run, map_rms] (option "emit_distmap", include/dmpfold_hip.h; the map's diagonal is what the
        network predicts, not zero).  confs, distmap and info are views of the one allocation handed to the library.
        The option is set for this call only; no host synchronisation is added.  (On an engine whose "emit_distmap" option
        was set to 1 by hand the library writes the long buffer in every call; without `distmap=True` the call still
        returns the two tensors, confs being the first L floats of it.)
        `converge` (Angstrom; None = the engine's "recycle_tol_mA" option as it stands, 0 by default): stop recycling
        after the first pass p >= 1 whose trace changes the seed distance map by no more than that (RMS); the outputs
        are bit for bit those of `iterations` = p.  `passes_run` tells how many trunk passes ran.  With a tolerance the
        call synchronises with the GPU once per pass."""
        extras, restrain = _asked(locals())
        return self._predict(self._upload(alnmat), template_ca, iterations, minsteps, converge, extras, restrain)

    def _forget_last(self):
        self._last = _Last(Outputs(None, None), 0, None)
        self._restrained = None       # (restrain_milli, restrain_cut_mA, steps, coords) of a restrained last prediction

    @property
    def restrain(self):
        """The report of the last prediction if its final refinement was restrained (restrain_report: k, cutoff, steps,
        map_rms, restrained_pairs, clashes, bond_dev_max), None otherwise.  Synchronises with the GPU."""
        if self._restrained is None:
            return None
        milli, cut_mA, steps, coords = self._restrained
        torch.cuda.synchronize(self.device)
        out = self._last.out
        return restrain_report(milli * 1e-3, cut_mA * 1e-3, steps, out.distmap, None if out.info is None else out.info[2].item(),
                               coords)

    # Per row of score.BLOCKS two properties, made behind the class: the block of the last prediction on the GPU, a view of the
    # buffer handed to the library, under its field's name (score_block, map_score_block, pass_block, ss_block, exposure_block,
    # align_block, search_block), and its unpacked form under the row's name (scores, map_scores, pass_scores, ss, exposure,
    # alignment, hits); None where the option was off.
    def _unpacked(self, row):
        """The block of a row of score.BLOCKS of the last prediction through the row's unpacker, None without it.
        Synchronises with the GPU."""
        block = getattr(self._last.out, row.field)
        if block is None:
            return None
        torch.cuda.synchronize(self.device)
        return row.unpack(block, self._last.L, library=self._last.library, coords=self._last.coords, confs=self._last.out.confs)

    @property
    def domain_search_block(self):
        """"search_domains": (400 + 2L) K floats - the library searched with every domain of the last prediction's model - or None."""
        return self._last.out.domain_search_block

    @property
    def domain_hits(self):
        """The domain search of the last prediction as score.unpack_domain_search gives it, with the library's `names` and -
        where it gave `refined` - `refine` beside it; None if it ran without option "search_domains".  Synchronises with the GPU."""
        block, library = self.domain_search_block, self._last.library
        if block is None or library is None:
            return None
        torch.cuda.synchronize(self.device)
        hits = dict(_score.unpack_domain_search(block, self._last.L, len(library), library.refine), names=list(library.names))
        if "refined" in hits:
            hits["refine"] = library.refine
        return hits

    @property
    def domain_score_block(self):
        """"score_domains": 1040 + 4L floats - every domain of the last prediction scored against the native - or None."""
        return self._last.out.domain_score_block

    @property
    def domain_scores(self):
        """The domain scores of the last prediction as score.unpack_domain_scores gives them; None if it ran without option
        "score_domains".  Synchronises with the GPU."""
        block = self.domain_score_block
        if block is None:
            return None
        torch.cuda.synchronize(self.device)
        return _score.unpack_domain_scores(block, self._last.L)

    @property
    def flex_block(self):
        """"flex": 48 + 20L floats - the Gaussian network model of the last prediction's trace and of the native's - or None."""
        return self._last.out.flex_block

    @property
    def flex(self):
        """The flexibility of the last prediction as score.unpack_flex gives it, with the prediction's confidences and - where
        option "domains" was on - its parse; None if it ran without option "flex".  Synchronises with the GPU."""
        block = self.flex_block
        if block is None:
            return None
        torch.cuda.synchronize(self.device)
        dom = self._last.out.domains_block
        parse = None if dom is None else _score.unpack_domains(dom, self._last.L)
        return _score.unpack_flex(block, self._last.L, confs=self._last.out.confs[:self._last.L], domains=parse)

    def set_flex(self, on, cutoff=7.3):
        """Option "flex" on this engine, as it stands from now on: every prediction's final C-alpha trace (and, with a whole
        `native`, the native's) gets its Gaussian network model on the GPU - contacts within `cutoff` Angstrom (4 .. 20), the
        eight lowest eigenpairs of the Kirchhoff matrix, the slow-mode fluctuation; what a call returns does not change, the
        result is in `flex` (score.unpack_flex) and `flex_block`."""
        mA = _score.flex_cut_mA(cutoff) if on else None       # (raises before anything changes)
        if on:
            self.set_option("flex_cut_mA", mA)
        self.set_option("flex", 1 if on else 0)

    @contextlib.contextmanager
    def with_flex(self, cutoff=7.3):
        """Option "flex" and its cutoff set for the duration of the block, then as they were (`set_flex`)."""
        values = {"flex_cut_mA": _score.flex_cut_mA(cutoff), "flex": 1}
        before = {}
        try:
            for name, value in values.items():
                before[name] = self.get_option(name)
                self.set_option(name, value)
            yield self
        finally:
            for name, value in reversed(list(before.items())):
                self.set_option(name, value)

    def predict_flex(self, alnmat, *args, flex_cutoff=7.3, **asked):
        """`predict` with option "flex" set for this call only: the same arguments, the same return value; the result is in
        `flex` and `flex_block` afterwards."""
        with self.with_flex(flex_cutoff):
            return self.predict(alnmat, *args, **asked)

    @property
    def msa_report_block(self):
        """"msa_report": 128 + 8L floats (+ L*L with the map) - depth, conservation and DCA contacts of the last prediction's
        alignment - or None."""
        return self._last.out.msa_report_block

    @property
    def msa_report(self):
        """The alignment report of the last prediction as score.unpack_msa_report gives it, with the prediction's confidences;
        None if it ran without option "msa_report".  Synchronises with the GPU."""
        block = self.msa_report_block
        if block is None:
            return None
        torch.cuda.synchronize(self.device)
        return _score.unpack_msa_report(block, self._last.L, confs=self._last.out.confs[:self._last.L])

    def set_msa_report(self, on, dca_map=False):
        """Option "msa_report" on this engine, as it stands from now on: every prediction also reports on its alignment on the
        GPU - Neff at three thresholds, gaps, copies, the histograms, per-column conservation, the strongest DCA coupling of
        every column and, with a `native`, the DCA contact precisions; `dca_map` adds the raw L x L DCA contact map.  What a
        call returns does not change, the result is in `msa_report` (score.unpack_msa_report) and `msa_report_block`."""
        self.set_option("msa_report", (2 if dca_map else 1) if on else 0)

    @contextlib.contextmanager
    def with_msa_report(self, dca_map=False):
        """Option "msa_report" set for the duration of the block, then as it was (`set_msa_report`)."""
        before = self.get_option("msa_report")
        try:
            self.set_option("msa_report", 2 if dca_map else 1)
            yield self
        finally:
            self.set_option("msa_report", before)

    def predict_msa_report(self, alnmat, *args, dca_map=False, **asked):
        """`predict` with option "msa_report" set for this call only: the same arguments, the same return value; the result is
        in `msa_report` and `msa_report_block` afterwards."""
        with self.with_msa_report(dca_map):
            return self.predict(alnmat, *args, **asked)

    _score_domains = False           # set_score_domains / with_score_domains: the calls of this engine score every domain

    def set_score_domains(self, on):
        """Every domain scored against the native (option "score_domains") by this engine's calls from now on: a call given a
        `native` sets the option for itself - and "domains", with the parameters of `set_domains` / `with_domains` or the
        defaults - and puts both back; it scores each domain of the model's parse and of the native's against the native on the
        domain's own superposition.  What a call returns does not change, the result is in `domain_scores`
        (score.unpack_domain_scores) and `domain_score_block`.  A call without `native` raises ValueError."""
        self._score_domains = bool(on)

    @contextlib.contextmanager
    def with_score_domains(self):
        """`set_score_domains(True)` for the duration of the block, then as it was."""
        before = self._score_domains
        try:
            self._score_domains = True
            yield self
        finally:
            self._score_domains = before

    def set_domains(self, on, tau=0.25, min_size=40, min_segment=10):
        """Option "domains" on this engine, as it stands from now on: every prediction's final C-alpha trace is split into
        structural domains on the GPU (and, with a whole `native`, the native's); what a call returns does not change, the
        result is in `domains` (score.unpack_domains) and `domains_block`.  `tau`, `min_size`, `min_segment`: domains_options."""
        values = domains_options(tau, min_size, min_segment) if on else None      # (raises before anything changes)
        for name, value in zip(DOMAINS_OPTIONS, values or ()):
            self.set_option(name, value)
        self.set_option("domains", 1 if on else 0)

    @contextlib.contextmanager
    def with_domains(self, tau=0.25, min_size=40, min_segment=10):
        """Option "domains" and its three parameters set for the duration of the block, then as they were: the predictions
        made inside it get their domains (`set_domains`)."""
        values = dict(zip(DOMAINS_OPTIONS, domains_options(tau, min_size, min_segment)), domains=1)
        before = {}
        try:
            for name, value in values.items():
                before[name] = self.get_option(name)
                self.set_option(name, value)
            yield self
        finally:
            for name, value in reversed(list(before.items())):
                self.set_option(name, value)

    def predict_domains(self, alnmat, *args, domains_tau=0.25, domains_min_size=40, domains_min_segment=10, **asked):
        """`predict` with option "domains" set for this call only: the same arguments, the same return value; the parse is in
        `domains` and `domains_block` afterwards."""
        with self.with_domains(domains_tau, domains_min_size, domains_min_segment):
            return self.predict(alnmat, *args, **asked)

    @property
    def passes_run(self):
        """Trunk passes of the last prediction (iterations + 1 unless it converged earlier)."""
        return self.get_option("passes_run")

    def predict_device(self, d_msa, template_ca=None, iterations=default_iterations,
                       minsteps=default_minsteps, converge=None, distmap=False, native=None, structure=None, library=None,
                       score_map=False, score_passes=False, ss=False, restrain=None, restrain_cutoff=15.0, exposure=False):
        """Same as `predict` for residue codes already resident on the GPU (uint8 (N, L))."""
        extras, restrain = _asked(locals())
        return self._predict(d_msa, template_ca, iterations, minsteps, converge, extras, restrain)

    def _upload(self, alnmat):
        with torch.cuda.device(self.device):
            return torch.from_numpy(np.ascontiguousarray(alnmat, dtype=np.uint8)).to(self.device)

    def _predict(self, d_msa, template_ca, iterations, minsteps, converge, extras, restrain=None):
        with self._call_options(converge, extras, restrain):
            return self._run(d_msa, template_ca, iterations, minsteps, extras).public(extras.distmap, blocks=False)

    @contextlib.contextmanager
    def _call_options(self, converge, extras, restrain=None):
        """The options one call asks for - read when the prediction begins - set for its duration, then as they were.
        `converge` None leaves "recycle_tol_mA" as it stands; "emit_distmap" / "score_native" / "align_structure" set by hand
        stay set.  `restrain`: None (the two restraint options stay as they stand) or what restrain_options gave."""
        want = {} if converge is None else {"recycle_tol_mA": converge_to_mA(converge)}    # (raises before anything changes)
        def turn_on(option, asked_by=None):
            """An option that is off is wanted on; "score_native" as the need of another only says that a native must be given."""
            if not self.get_option(option):
                if asked_by is None or option != "score_native":
                    want[option] = 1
                elif extras.native is None:
                    raise ValueError(needs_native(asked_by, asked_by, "`native`"))

        if restrain is not None:
            want["restrain_milli"], want["restrain_cut_mA"] = restrain
            for need in NEEDS["restrain_milli"] if restrain[0] > 0 else ():
                turn_on(need)                             # (map_rms comes back with the map)
        for field, option in CALL_OPTIONS:
            value = getattr(extras, field)
            if value is None or not (field in CALL_INPUTS or value):
                continue
            for need in NEEDS.get(option, ()):
                turn_on(need, asked_by=option)
            if field in CALL_CHECKS and not self.get_option(option):
                CALL_CHECKS[field](value)                 # (a bad shape raises before anything changes)
            turn_on(option)
        if extras.library is not None and not self.get_option("search_structures"):
            extras.library.check(self.max_L)                                               # (raises, naming the entry)
            want["search_max_m"] = extras.library.max_m   # before the option itself: the scratch is sized from it
            want["search_structures"] = len(extras.library)
            if extras.library.refine:
                want["search_refine"] = extras.library.refine      # screen every entry, refine the best so many
        if extras.library is not None and getattr(extras.library, "domains", False) and not self.get_option("search_domains"):
            turn_on("domains")                                     # (with the parameters set_domains / with_domains hold, or the defaults)
            want["search_domains"] = 1                             # the library searched with every domain of the model as well
        if getattr(self, "_score_domains", False) and not self.get_option("score_domains"):        # (set_score_domains / with_score_domains)
            if extras.native is None and not self.get_option("score_native"):
                raise ValueError(SCORE_DOMAINS_NEEDS_NATIVE)
            turn_on("domains")                                     # (likewise: the parameters as they stand, or the defaults)
            want["score_domains"] = 1                              # behind "score_native" and "domains", which it needs
        before = {}
        try:
            for name, value in want.items():
                before[name] = self.get_option(name)
                self.set_option(name, value)
            yield
        finally:
            for name, value in reversed(list(before.items())):
                self.set_option(name, value)

    def _run(self, d_msa, template_ca, iterations, minsteps, extras):
        """One prediction with the options as the context holds them (not as the call asked) -> Outputs."""
        emit, score, smap, align, search = (self.get_option(name) for name in LAYOUT_OPTIONS)
        structure, library = extras.structure, extras.library
        if align and structure is not None and _score.as_structure(structure).shape[0] > self.max_L:
            raise RuntimeError(f"structure has {len(structure)} rows; the engine's capacity is {self.max_L} (max_L)")
        if search:
            if library is None or len(library) != search:
                raise RuntimeError(f"search_structures is {search}: the prediction needs a library of that many entries"
                                   + ("" if library is None else f", got {len(library)}"))
            library.check(self.get_option("search_max_m") or self.max_L)
        assert d_msa.dtype == torch.uint8 and d_msa.is_contiguous() and d_msa.device == self.device
        n, L = d_msa.shape
        if L < 8:
            raise RuntimeError(f"alignment has {L} columns; the network needs at least 8 "
                               "(MDS embedding width, reference network.py:250-253)")
        flags = Flags(bool(emit), bool(emit), bool(score), bool(smap and emit and score), bool(align), search, self.max_L,
                      agree_passes([self.get_option("score_passes")], score, iterations), **_own_blocks([self]))
        with torch.cuda.device(self.device):
            self._forget_last()
            domains = bool(self.get_option("domains"))
            d_tpl, out = _stage(self.device, L, template_ca, flags, extras, domains, bool(self.get_option("search_domains")),
                                bool(self.get_option("score_domains")), bool(self.get_option("flex")), self.get_option("msa_report"))
            self._last = _Last(out._replace(coords=None), L, library if search else None, out.coords if domains else None)
            milli = self.get_option("restrain_milli")
            if milli > 0:
                self._restrained = (milli, self.get_option("restrain_cut_mA"), int(max(minsteps, 0)), out.coords)
            if self._stream is not None:
                # an engine with its own stream: order it after the producer of the inputs and tell the
                # caching allocator that these blocks are in use there
                self._stream.wait_stream(torch.cuda.current_stream(self.device))
                for x in (out.coords, out.confs, d_msa, d_tpl):
                    if x is not None:
                        x.record_stream(self._stream)
            _lib.check(self.lib.dmp_predict(
                self._ctx, d_msa.data_ptr(), n, L,
                d_tpl.data_ptr() if d_tpl is not None else None, L if d_tpl is not None else 0,
                int(max(iterations, 0)), int(max(minsteps, 0)),
                out.coords.data_ptr(), out.confs.data_ptr(), self.stream()))
            # d_msa / d_tpl are stream-ordered temporaries: keep them alive until the work is queued
            self._keep = (d_msa, d_tpl)
        return out

    def set_option(self, name, value):
        """Additive engine options, e.g. ("conv_f32_exact", 1); see include/dmpfold_hip.h."""
        _lib.check(self.lib.dmp_ctx_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name):
        """The option's current value, read back from the context (not from a Python-side mirror: the
        C API may have been used directly)."""
        v = C.c_int(0)
        _lib.check(self.lib.dmp_ctx_get_option(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def sync_faults(self):
        """Wait for the queued work; the DMP_FAULT_* bits recorded since the last report (reporting
        clears them).  Predictions that ran while a bit was raised returned NaN."""
        bits = C.c_int(0)
        _lib.check(self.lib.dmp_sync_faults(self._ctx, self.stream(), C.byref(bits)))
        return bits.value

    def sync_check(self):
        """Wait for the queued work and raise if a device-side fault was recorded: IndexError for a
        residue code above 21 (as the reference's embedding), DeviceFault otherwise."""
        raise_for_faults(self.sync_faults())

    def predict_checked(self, alnmat, template_ca=None, iterations=default_iterations,
                        minsteps=default_minsteps, converge=None, distmap=False, native=None, structure=None, library=None,
                        score_map=False, score_passes=False, ss=False, restrain=None, restrain_cutoff=15.0, exposure=False):
        """`predict`, synchronised and verified.  The default convolution multiplies f16 pieces of its
        operands and needs |activation| < 6e4; a prediction that leaves that range (never seen with
        InstanceNorm'd trunks, but the trained weights decide) is repeated with the 3-way bf16 split,
        which has float32's range, at about half the convolution rate."""
        extras, restrain = _asked(locals())
        return self._checked(self._upload(alnmat), template_ca, iterations, minsteps, converge, extras,
                             restrain).public(extras.distmap, blocks=False)

    def predict_device_checked(self, d_msa, template_ca=None, iterations=default_iterations,
                               minsteps=default_minsteps, converge=None, distmap=False, native=None, structure=None, library=None,
                               score_map=False, score_passes=False, ss=False, restrain=None, restrain_cutoff=15.0, exposure=False):
        """`predict_checked` for residue codes already resident on the GPU (`distmap`, `native`, `structure`, `library`,
        `score_map`, `score_passes`, `ss`, `restrain`: see `predict`; a repeat of the prediction returns the repeat's map,
        scores, alignment and hits)."""
        extras, restrain = _asked(locals())
        return self._checked(d_msa, template_ca, iterations, minsteps, converge, extras, restrain).public(extras.distmap, blocks=False)

    def _checked(self, d_msa, template_ca, iterations, minsteps, converge, extras, restrain=None):
        """`predict_device_checked` -> Outputs; the repeats run with the call's options still set and carry the call's
        extras along."""
        def run():
            return self._run(d_msa, template_ca, iterations, minsteps, extras), self.sync_faults()

        with self._call_options(converge, extras, restrain):
            out, bits = run()
            self.last_fallback = False
            if bits & FAULT_VGRU_HANDOFF and self.get_option("vgru_persistent"):
                # the persistent chain's row barriers timed out (its workgroups were not all resident: another process
                # on this GPU holds CUs with a launch of the same kind): the launch-per-row form has no such requirement
                print("dmpfold2_amd: the persistent vertical-GRU launch could not get the whole GPU; re-running this "
                      "alignment (and every later one on this engine) with one launch per alignment row", file=sys.stderr)
                self.set_option("vgru_persistent", 0)
                out, bits = run()
            if bits == FAULT_F16_RANGE and self.get_option("conv_mode") == 0:
                print("dmpfold2_amd: activations left the f16 range of the split-product convolution; "
                      "re-running this alignment with conv_mode=2 (bf16 split, no range limit)",
                      file=sys.stderr)
                self.last_fallback = True
                self.set_option("conv_mode", 2)
                try:
                    out, bits = run()
                finally:
                    self.set_option("conv_mode", 0)
            raise_for_faults(bits)
            return out

    def fetch(self, name, numel):
        out = torch.empty((int(numel),), dtype=torch.float32, device=self.device)
        n = _lib.check(self.lib.dmp_debug_fetch(self._ctx, name.encode(), out.data_ptr(),
                                                int(numel), self.stream()))
        return out[:n]


# The properties of an `Engine` per row of score.BLOCKS (see `Engine._unpacked`); RESULT_DOCS: how each result reads.
RESULT_DOCS = {"scores": "The scores of the last prediction as score.unpack_scores gives them",
               "map_scores": "The map scores of the last prediction as score.unpack_map_scores gives them",
               "pass_scores": "The pass table of the last prediction as score.unpack_pass_scores gives it",
               "ss": "The secondary structure of the last prediction as score.unpack_ss gives it",
               "exposure": "The solvent exposure of the last prediction as score.unpack_exposure gives it",
               "domains": "The structural domains of the last prediction as score.unpack_domains gives them",
               "alignment": "The structural alignment of the last prediction as score.unpack_alignment gives it",
               "hits": "The search of the last prediction as score.unpack_search gives it, with the library's `names` beside `hits` "
                       "and `rank`"}
for _row in _score.BLOCKS:
    setattr(Engine, {"map_block": "map_score_block"}.get(_row.field, _row.field),
            property(lambda self, field=_row.field: getattr(self._last.out, field),
                     doc=f'"{_row.option}": {_row.shape} floats, or None'))
    setattr(Engine, _row.name, property(lambda self, row=_row: self._unpacked(row),
                                        doc=f'{RESULT_DOCS[_row.name]}, None if it ran without option "{_row.option}".  '
                                            "Synchronises with the GPU."))


class _PipelineEngine(Engine):
    """Engine i of a `Pipeline`: a view of the context and stream the C pipeline owns (options, introspection, the
    repeat of a faulted target on an idle pipeline); closing it does nothing."""

    def __init__(self, lib, device, ctx, stream_ptr, max_L, max_N):       # noqa: super().__init__ creates a context
        self.lib = lib
        self.device = device
        self.max_L, self.max_N = int(max_L), int(max_N)
        self._ctx = C.c_void_p(ctx)
        self._stream = torch.cuda.ExternalStream(stream_ptr, device=device)
        self.weights_tag = None
        self.last_fallback = False
        self._forget_last()

    def close(self):
        self._ctx = C.c_void_p()

    def __del__(self):
        pass


# A target in a `Pipeline`: what stays alive until its result is handed out and what a repeat needs.  `out`: its Outputs,
# `ready`: the event behind the producer of its inputs, `extras`: the native, structure and library the target was staged
# with - each None where its option was off.
_Job = namedtuple("_Job", "d_msa iterations minsteps d_tpl out ready extras")


# ticket states of the C pipeline (include/dmpfold_hip.h, DMP_TICKET_*)
_T_QUEUED, _T_RUNNING, _T_ISSUED, _T_DONE, _T_FAILED = 0, 1, 2, 3, 4


class Pipeline:
    """Throughput mode on one GPU: `streams` engines (each its own context and HIP stream) share a lane, so their
    machine-filling convolutions take turns while the latency-bound kernels of one target (eigensolver, sequence GRUs,
    minimiser) run under the convolutions of another; targets that start together run their vertical GRUs as one chain.

    Round 6: the scheduler lives behind the C ABI (csrc/pipeline.hip, dmp_pipeline_*: one host thread inside the library
    issues every unit); this class allocates the tensors, keeps them alive, and mirrors the interface the Python scheduler
    of rounds 1-5 had - submit / pump / drain / result, step / poll / peek for the streaming batch front end, collect for
    the repeat of faulted targets."""

    def __init__(self, device, max_L, max_N, state_dict, streams=2, precision=None, torch_streams=False, converge=None,
                 distmap=False, score=False, align=False, search=None, score_map=False, score_passes=False, ss=False,
                 restrain=None, exposure=False):
        """`torch_streams`: the engines run on PyTorch pool streams handed to the library (dmp_pipeline_create_on) instead of
        the library's own - for a host that wants every stream to be one its allocator knows.
        `converge` (Angstrom, None = off): every target stops recycling once its trace has converged to that tolerance
        (`set_converge`; `stats()` counts the passes run and saved).
        `distmap`: every target also returns its chosen pass's distance map and [best_pass, passes_run, map_rms]
        (`set_distmap`): `result`, `peek`, `collect` and `run` then give (coords, confs, distmap, info) per target.
        `score`: every target is scored against the native trace given to `submit` (`set_score`); its score block (5L + 24
        floats, score.unpack_scores) is then the last element of what those calls give per target.
        `align`: every target is aligned with the `structure` given to `submit` (`set_align`); its align block (25 + 2L + 3m
        floats, score.unpack_alignment) is then the last element of what those calls give per target, behind the score block.
        `search` (a score.Library): every target is aligned with every entry of it (`set_search`); its search block (26K + 2LK
        + 3M floats, score.unpack_search) is then the last element of all.
        `score_map`: every target's distance map is scored against its native too (`set_score_map`, which turns `distmap`
        and `score` on); its map-score block (64 + L floats, score.unpack_map_scores) then comes behind even the search block.
        `score_passes`: every recycling pass of every target is scored against its native (`set_score_passes`, which turns
        `score` on); its pass block (16 + 8R floats, R = min(iterations + 1, 128) of that submission,
        score.unpack_pass_scores) is then the last element of all.
        `ss`: every target's backbone gets its secondary structure assigned (`set_ss`); its SS block (32 + 8L floats,
        score.unpack_ss) then comes behind even the pass block.
        `exposure`: every target's backbone gets its solvent exposure counted (`set_exposure`); its exposure block (32 + 16L
        floats, score.unpack_exposure) then comes behind even the SS block.
        `restrain` (force constant K, None = off): every target's final refinement is restrained to its predicted distance
        map (`set_restrain`, which turns `distmap` on; cutoff 15 A - `set_restrain` takes another)."""
        self.lib = _lib.load()
        self._search = None
        self.device = _resolve_device(device)
        S = max(1, int(streams))
        self._p = C.c_void_p()
        max_N = int(min(max_N, MAX_SEQS))
        with torch.cuda.device(self.device):
            if torch_streams:
                self._torch_streams = [torch.cuda.Stream(device=self.device) for _ in range(S)]
                arr = (C.c_void_p * S)(*[st.cuda_stream for st in self._torch_streams])
                _lib.check(self.lib.dmp_pipeline_create_on(self.device.index, int(max_L), max_N, S, arr, C.byref(self._p)))
            else:
                _lib.check(self.lib.dmp_pipeline_create(self.device.index, int(max_L), max_N, S, C.byref(self._p)))
        self.engines = [_PipelineEngine(self.lib, self.device, self.lib.dmp_pipeline_ctx(self._p, i),
                                        self.lib.dmp_pipeline_stream(self._p, i), max_L, max_N) for i in range(S)]
        self.engines[0].set_weights(state_dict)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dmp_pipeline_weights_ready(self._p), RuntimeError)    # packed once per pipeline
        prec = precision if precision is not None else _env_precision()
        if prec is not None:
            self.set_option("precision", prec)
        asked = locals()
        for name in ("converge", "distmap", "score", "align", "search", "score_map", "score_passes", "ss", "exposure", "restrain"):
            value = asked[name]       # (set in this order; a tolerance, a library and a force constant are given unless None)
            if value is not None and (name in ("converge", "search", "restrain") or value):
                getattr(self, "set_" + name)(value)
        self._jobs = {}               # ticket -> _Job: kept alive
        self._handed = []             # tickets whose result was handed out before the GPU finished them: released later

    def set_option(self, name, value):
        """An engine option on EVERY engine of the (idle) pipeline: a group's vertical-GRU chain runs in its leader's
        arithmetic and serves all members, so the engines must agree on "precision" / "vgru_f32" / "vgru_persistent"."""
        _lib.check(self.lib.dmp_pipeline_set_option(self._p, name.encode(), int(value)))

    def set_converge(self, converge):
        """Convergence tolerance (Angstrom; None or 0 = fixed depth) of every target submitted from now on; idle pipeline only."""
        self.set_option("recycle_tol_mA", converge_to_mA(converge))

    def set_restrain(self, restrain, cutoff=15.0):
        """Options "restrain_milli" / "restrain_cut_mA" on every engine: the final refinement of targets submitted from now on
        is restrained to their predicted distance map with force constant `restrain` (None or 0 = off) below `cutoff`
        Angstrom.  Turning it on turns "emit_distmap" on, so that map_rms comes back; turning it off leaves that as it is.
        Idle pipeline only."""
        milli, cut_mA = restrain_to_milli(restrain), restrain_cutoff_to_mA(cutoff)     # (raise before anything changes)
        for need in NEEDS["restrain_milli"] if milli > 0 else ():
            self.set_option(need, 1)
        self.set_option("restrain_cut_mA", cut_mA)
        self.set_option("restrain_milli", milli)

    def _set_flag(self, option, on):
        """An on / off option on every engine; turning it on turns on what it needs (NEEDS) first."""
        for need in NEEDS.get(option, ()) if on else ():
            self.set_option(need, 1)
        self.set_option(option, 1 if on else 0)

    def set_distmap(self, on):
        """Option "emit_distmap" on every engine: targets submitted from now on return their distance map; idle pipeline only."""
        self._set_flag("emit_distmap", on)

    def set_score(self, on):
        """Option "score_native" on every engine: targets submitted from now on are scored against the `native` given to
        `submit` (none given: no row present, n_pairs 0); idle pipeline only."""
        self._set_flag("score_native", on)

    def set_score_map(self, on):
        """Option "score_map" on every engine: the distance map of targets submitted from now on is scored against the
        `native` given to `submit`.  Turning it on turns "emit_distmap" and "score_native" on, which it needs; turning it off
        leaves them as they are.  Idle pipeline only."""
        self._set_flag("score_map", on)

    def set_score_passes(self, on):
        """Option "score_passes" on every engine: every recycling pass of targets submitted from now on is scored against the
        `native` given to `submit`.  Turning it on turns "score_native" on, which it needs; turning it off leaves that as it
        is.  Idle pipeline only."""
        self._set_flag("score_passes", on)

    def set_ss(self, on):
        """Option "assign_ss" on every engine: targets submitted from now on get the secondary structure of their backbone
        (and, with `set_score` on and a whole native given to `submit`, of the native's); idle pipeline only."""
        self._set_flag("assign_ss", on)

    def set_exposure(self, on):
        """Option "exposure" on every engine: targets submitted from now on get the solvent exposure of their backbone counted
        (and, with `set_score` on and a whole native given to `submit`, of the native's); idle pipeline only."""
        self._set_flag("exposure", on)

    def use_domains(self, on, tau=0.25, min_size=40, min_segment=10):
        """Option "domains" on every engine: targets submitted from now on get their final C-alpha trace split into structural
        domains (and, with `set_score` on and a whole native given to `submit`, the native's); the domain block (32 + 2L + 256
        floats, score.unpack_domains) then comes last of all in what `result`, `peek` and `collect` give per target.  `tau`,
        `min_size`, `min_segment`: domains_options.  Idle pipeline only."""
        values = domains_options(tau, min_size, min_segment) if on else None      # (raises before anything changes)
        for name, value in zip(DOMAINS_OPTIONS, values or ()):
            self.set_option(name, value)
        self.set_option("domains", 1 if on else 0)

    def use_score_domains(self, on):
        """Option "score_domains" on every engine: every domain of targets submitted from now on - of the model's parse and,
        where the native is whole, of the native's - is scored against the `native` given to `submit` on its own
        superposition; the domain-score block (1040 + 4L floats, score.unpack_domain_scores) is the attribute
        `domain_score_block` of what `outputs_of` gives.  It needs `set_score` on - RuntimeError if not - and turns "domains" on
        where it is off, with the parameters `use_domains` set, or the defaults; turning it off leaves both as they are.
        Idle pipeline only."""
        if on and not all(e.get_option("score_native") for e in self.engines):
            raise RuntimeError("use_score_domains scores every domain against the native of \"score_native\", which is off: use set_score first")
        if on and not all(e.get_option("domains") for e in self.engines):
            self.set_option("domains", 1)
        self.set_option("score_domains", 1 if on else 0)

    def use_flex(self, on, cutoff=7.3):
        """Option "flex" on every engine: targets submitted from now on get the Gaussian network model of their final C-alpha
        trace (and, with `set_score` on and a whole native given to `submit`, of the native's) with contacts within `cutoff`
        Angstrom; the flex block (48 + 20L floats, score.unpack_flex) is the attribute `flex_block` of what `outputs_of` gives.
        Idle pipeline only."""
        mA = _score.flex_cut_mA(cutoff) if on else None       # (raises before anything changes)
        if on:
            self.set_option("flex_cut_mA", mA)
        self.set_option("flex", 1 if on else 0)

    def use_msa_report(self, on, dca_map=False):
        """Option "msa_report" on every engine: targets submitted from now on get the report on their alignment (depth,
        conservation, DCA contacts; with `set_score` on and a native given to `submit`, the DCA precisions; `dca_map`: the raw
        map too); the report block (128 + 8L floats, + L*L; score.unpack_msa_report) is the attribute `msa_report_block` of what
        `outputs_of` gives.  Idle pipeline only."""
        self.set_option("msa_report", (2 if dca_map else 1) if on else 0)

    def set_align(self, on):
        """Option "align_structure" on every engine: targets submitted from now on are aligned with the `structure` given to
        `submit` (none given: m = 0, NaN in every out slot); idle pipeline only."""
        self._set_flag("align_structure", on)

    def set_search(self, library):
        """Option "search_structures" on every engine: targets submitted from now on are aligned with every entry of `library`
        (a score.Library; None = off) - with a `refine` of R on the library, screened and only the best R refined (option
        "search_refine"); with `domains` on the library, also with every domain of the model (option "search_domains", which
        turns "domains" on with the parameters `use_domains` set, or the defaults; the domain-search block is the attribute
        `domain_search_block` of what `outputs_of` gives); idle pipeline only."""
        with_domains = library is not None and bool(getattr(library, "domains", False))
        if self.engines[0].get_option("search_domains") != int(with_domains):
            if with_domains and not all(e.get_option("domains") for e in self.engines):
                self.set_option("domains", 1)
            self.set_option("search_domains", int(with_domains))
        if library is None:
            self.set_option("search_structures", 0)
            self.set_option("search_max_m", 0)
            if self.engines[0].get_option("search_refine"):
                self.set_option("search_refine", 0)
        else:
            library.check(self.engines[0].max_L)
            self.set_option("search_max_m", library.max_m)
            self.set_option("search_structures", len(library))
            if library.refine or self.engines[0].get_option("search_refine"):
                self.set_option("search_refine", library.refine)
        self._search = library

    collected = {}                   # of the last `collect`: {ticket: the score.Outputs its entry was made of}, for what `public` leaves out

    def close(self):
        if self._p:
            self.lib.dmp_pipeline_destroy(self._p)           # joins the scheduler thread, synchronises the streams
            self._p = C.c_void_p()
        for e in self.engines:
            e.close()
        self.engines = []
        self._jobs = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- submission --------------------------------------------------------------------------
    def submit(self, d_msa, iterations=default_iterations, minsteps=default_minsteps, template_ca=None, native=None,
               structure=None):
        """Queue one target (uint8 (N, L) tensor on the GPU, optional template CA trace (L, 3));
        returns a ticket for `result`.  `native`: the trace to score against (Engine.predict), read only with `set_score` on.
        `structure`: the (m, 3) trace to align the model with, read only with `set_align` on."""
        assert d_msa.dtype == torch.uint8 and d_msa.is_contiguous() and d_msa.device == self.device
        n, L = d_msa.shape
        if L < 8:
            raise RuntimeError(f"alignment has {L} columns; the network needs at least 8")
        if L > self.engines[0].max_L or n > self.engines[0].max_N:
            raise RuntimeError(f"alignment {n} x {L} exceeds the pipeline capacity "
                               f"{self.engines[0].max_N} x {self.engines[0].max_L}")
        with torch.cuda.device(self.device):
            # the library cannot check the buffer: it is sized by the options as the engines hold them, whichever way they
            # were set (set_distmap, set_option, an engine's own set_option - then the largest any engine would write)
            flags = agree_options([e.get_option(name) for name in LAYOUT_OPTIONS] for e in self.engines)
            flags = flags._replace(max_L=self.engines[0].max_L,
                                   passes=agree_passes([e.get_option("score_passes") for e in self.engines], flags.score, iterations),
                                   **_own_blocks(self.engines))
            if flags.align and structure is not None and _score.as_structure(structure).shape[0] > flags.max_L:
                raise RuntimeError(f"structure has {len(structure)} rows; the pipeline's capacity is {flags.max_L}")
            if flags.search and (self._search is None or len(self._search) != flags.search):
                raise RuntimeError(f"search_structures is {flags.search} on the engines: give the library to set_search")
            extras = Extras(native=native if flags.score else None, structure=structure if flags.align else None,
                            library=self._search if flags.search else None)
            # (the native, align and search blocks are written on the current stream: `ready` below is behind it)
            domains = agree([e.get_option("domains") for e in self.engines], "domains", "use_domains")
            if domains and any(tuple(e.get_option(n) for n in DOMAINS_OPTIONS) != tuple(self.engines[0].get_option(n) for n in DOMAINS_OPTIONS)
                               for e in self.engines[1:]):
                raise RuntimeError("the engines must agree on \"domains_tau_milli\", \"domains_min_size\" and \"domains_min_segment\" "
                                   "(whichever of them runs a target must give the same parse); use use_domains")
            search_domains = agree([e.get_option("search_domains") for e in self.engines], "search_domains", "set_search")
            score_domains = agree([e.get_option("score_domains") for e in self.engines], "score_domains", "use_score_domains")
            flex = agree([e.get_option("flex") for e in self.engines], "flex", "use_flex")
            if flex and len({e.get_option("flex_cut_mA") for e in self.engines}) > 1:
                raise RuntimeError("the engines must agree on \"flex_cut_mA\" (whichever of them runs a target must give the same network); use use_flex")
            msa_report = self.engines[0].get_option("msa_report")            # 0, 1 or 2: 2 is a larger block
            agree([e.get_option("msa_report") == msa_report for e in self.engines], "msa_report", "use_msa_report")
            d_tpl, out = _stage(self.device, L, template_ca, flags, extras, domains, search_domains, score_domains, flex, msa_report)
            # the stream that is current NOW produced d_msa (the caller's copy stream, say); the engine that takes the
            # target orders itself behind this point
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
        # Inputs and outputs are used on the stream of whichever engine takes the target (and, as a rider, on a group
        # leader's): the caching allocator has to know before it recycles their blocks.
        for e in self.engines:
            for x in (out.coords, out.confs, d_msa, d_tpl):
                if x is not None:
                    x.record_stream(e._stream)
        t = _lib.check(self.lib.dmp_pipeline_submit(
            self._p, d_msa.data_ptr(), n, L, d_tpl.data_ptr() if d_tpl is not None else None,
            int(max(iterations, 0)), int(max(minsteps, 0)), out.coords.data_ptr(), out.confs.data_ptr(),
            C.c_void_p(ready.cuda_event)))
        self._jobs[t] = _Job(d_msa, int(max(iterations, 0)), int(max(minsteps, 0)), d_tpl, out, ready, extras)
        self._reap()
        return t

    def _status(self, ticket):
        st, bits = C.c_int(0), C.c_int(0)
        rc = self.lib.dmp_pipeline_status(self._p, ticket, C.byref(st), C.byref(bits))
        return st.value, bits.value, rc

    def _reap(self):
        keep = []
        for t in self._handed:
            st, _, _ = self._status(t)
            if st in (_T_DONE, _T_FAILED):
                self.lib.dmp_pipeline_release(self._p, t)
            else:
                keep.append(t)
        self._handed = keep

    def _raise_failed(self):
        """A target whose units could not be issued (a HIP or capacity error inside the scheduler) fails its ticket; the
        Python scheduler of rounds 1-5 raised from pump() / drain() at that point, and so does this."""
        for t in list(self._jobs):
            st, _, rc = self._status(t)
            if st == _T_FAILED:
                _lib.check(rc if rc < 0 else -5)

    def pump(self):
        """Block until every queued target has been started on an engine."""
        _lib.check(self.lib.dmp_pipeline_wait(self._p, 0))
        self._raise_failed()

    def drain(self):
        """Block until every queued target is fully enqueued; the current stream then waits for
        the engines' streams (the host is not synchronised with the GPU)."""
        _lib.check(self.lib.dmp_pipeline_wait(self._p, 1))
        cur = torch.cuda.current_stream(self.device)
        for e in self.engines:
            cur.wait_stream(e._stream)
        self._raise_failed()

    def result(self, ticket):
        return self._result(ticket).public()

    def outputs_of(self, ticket):
        """The score.Outputs of a queued target, which stays queued: every block as a view of its buffer, the domain-search
        block of option "search_domains" and the domain-score block of option "score_domains" - which `result` never hands out -
        among them (valid once the target is done)."""
        return self._jobs[ticket].out

    def _result(self, ticket):
        job = self._jobs.pop(ticket)
        self._handed.append(ticket)
        self._reap()
        return job.out

    # ---- streaming use (dmpfold2_amd.batch): submit / step / poll, no barrier between targets ----------------
    def step(self, rounds=32):
        """The scheduler runs in its own thread inside the library: there is nothing to step.  Yields the core for a moment
        (the caller's loop does a piece of host work per call) and answers False - "nothing more for you to issue"."""
        time.sleep(2e-4)
        return False

    def backlog(self):
        """Targets queued but not yet started on an engine."""
        q, r = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.dmp_pipeline_backlog(self._p, C.byref(q), C.byref(r)))
        return q.value

    def busy(self):
        q, r = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.dmp_pipeline_backlog(self._p, C.byref(q), C.byref(r)))
        return q.value > 0 or r.value > 0

    def poll(self):
        """Tickets whose prediction has COMPLETED on the GPU since the last call (their tensors may be read from
        any stream); `peek` / `result` hand the tensors out."""
        buf, n = (C.c_int64 * 64)(), C.c_int(0)
        out = []
        while True:
            _lib.check(self.lib.dmp_pipeline_poll(self._p, buf, 64, C.byref(n)))
            out += [buf[i] for i in range(n.value)]
            if n.value < 64:
                return out

    def peek(self, ticket):
        return self._jobs[ticket].out.public()

    def stats(self):
        v = (C.c_longlong * 11)()
        _lib.check(self.lib.dmp_pipeline_stats(self._p, v, 11))
        return {"groups": v[0], "max_group": v[1], "rider_chains": v[2], "max_riders": v[3], "riders_left": v[4],
                "idle_rounds": v[5], "rounds": v[6], "scheduler_thread_cpu_s": v[7] * 1e-6,
                "passes_run": v[8], "early_stops": v[9], "passes_saved": v[10]}

    def submit_many(self, d_msas, iterations=default_iterations, minsteps=default_minsteps):
        """Submit a batch with the scheduler paused, so that the first vertical-GRU group is formed from the whole batch
        (the scheduler's thread would otherwise start whatever has arrived when it looks)."""
        _lib.check(self.lib.dmp_pipeline_pause(self._p, 1))
        try:
            return [self.submit(m, iterations, minsteps) for m in d_msas]
        finally:
            _lib.check(self.lib.dmp_pipeline_pause(self._p, 0))

    def collect(self, tickets):
        """drain + synchronise + verify.  Returns {ticket: (coords, confs) - with `distmap` on (coords, confs, distmap,
        info) - or Exception}: a target
        whose prediction recorded a device-side fault (its outputs are NaN) is repeated alone through
        `Engine.predict_device_checked` - which falls back to the range-free convolution where that
        is the cure - and only if that fails too its entry is the exception.  One bad target never
        costs the others their results.  Once one repeat needed the range-free convolution the
        remaining repeats run in it directly (the weights, not the alignment, put a trunk outside the
        f16 range: the others would only fault again first), with one note on stderr for all of them."""
        _lib.check(self.lib.dmp_pipeline_wait(self._p, 2))
        self.collected = {}
        cur = torch.cuda.current_stream(self.device)
        for e in self.engines:
            cur.wait_stream(e._stream)
        for e in self.engines:
            e.sync_faults()                     # the engines' latched words: cleared, the per-ticket words below decide
        out = {}
        eng = self.engines[0]
        mode0 = eng.get_option("conv_mode")
        try:
            for t in tickets:
                st, bits, rc = self._status(t)
                job = self._jobs.get(t)
                res = self._result(t)
                if st == _T_FAILED:
                    out[t] = _lib.DmpError(_lib.load().dmp_last_error().decode("utf-8", "replace") or f"error {rc}")
                    continue
                if bits:
                    # what the target ran with, for one engine alone: a block that was there without its input gets the
                    # input that means "none" (an all-NaN native, a structure of 0 rows)
                    emit, extras = res.distmap is not None, job.extras._replace(distmap=res.distmap is not None)
                    for field, option in CALL_OPTIONS[1:]:
                        there = getattr(res, _BLOCK_OF[option].field) is not None
                        if field not in CALL_INPUTS:
                            extras = extras._replace(**{field: there})
                        elif there and getattr(extras, field) is None:
                            extras = extras._replace(**{field: CALL_INPUTS[field](job.d_msa.shape[1])})
                    try:
                        rep = eng._checked(job.d_msa, job.d_tpl, job.iterations, job.minsteps, None, extras)
                        res = rep if emit else rep._replace(distmap=None, info=None)     # (engine 0's "emit_distmap" set by hand)
                        if eng.last_fallback:
                            eng.set_option("conv_mode", 2)
                        if not eng.get_option("vgru_persistent"):
                            # the repeat fell back to one vertical-GRU launch per row (another process holds CUs of
                            # this GPU): the other engines - and a group chain led by one of them - would only
                            # fault again, target after target
                            self.set_option("vgru_persistent", 0)
                    except (IndexError, _lib.DmpError) as exc:
                        out[t] = exc
                        continue
                out[t] = res.public()
                self.collected[t] = res
        finally:
            eng.set_option("conv_mode", mode0)
        return out

    def run(self, d_msas, iterations=default_iterations, minsteps=default_minsteps):
        """Predict every target (uint8 (N, L) tensors on the GPU).  Returns [(coords, confs)] ([(coords, confs, distmap,
        info)] with `distmap` on) in
        input order, ordered on the current stream; the host is not synchronised with the tail."""
        tickets = self.submit_many(d_msas, iterations, minsteps)
        self.drain()
        return [self.result(t) for t in tickets]

    def sync_check(self):
        """Synchronise every engine and raise for the first recorded fault (see `collect` for the
        per-target form)."""
        bits = 0
        for e in self.engines:
            bits |= e.sync_faults()
        raise_for_faults(bits)


class _EngineCache(dict):
    """device index -> the engine used last there (what tests and diagnostics look at).  Behind it a small LRU of
    engines per device, one per weights file: the reference builds a fresh network on every call (predict.py:79), so
    callers may alternate between weight files - or call from several threads - without re-packing 140 MB each time."""
    MAX_PER_DEVICE = 2

    def __init__(self):
        super().__init__()
        self.lru = {}                 # device index -> [engine, ...], most recently used last

    def clear(self):
        for engines in self.lru.values():
            for e in engines:
                e.close()
        self.lru = {}
        super().clear()


_ENGINES = _EngineCache()
_DEVICE_LOCKS = {}
_LOCKS_GUARD = threading.Lock()


def device_lock(device):
    """One re-entrant lock per GPU for the drop-in entry points: `aln_to_coords` may be called from several threads (the
    reference's function is re-entrant - every call builds its own network, predict.py:79); here the calls of a device
    share cached engines whose buffers one prediction owns from its first kernel to its synchronisation, so they take
    turns.  (Throughput across targets is what `Pipeline` / the batch front end are for.)"""
    dev = _resolve_device(device)
    with _LOCKS_GUARD:
        return _DEVICE_LOCKS.setdefault(dev.index, threading.RLock())


def get_engine(device, L, N, weights_file=None, state_dict=None):
    """Cached engine for `device` and these weights, grown when an alignment exceeds its capacity; weights are packed
    once per (engine, weights file).  Call it - and use the engine - under `device_lock(device)` when other threads may
    do the same."""
    if L > MAX_L:
        raise RuntimeError(f"alignment has {L} columns; this build supports at most {MAX_L} "
                           "(include/dmpfold_hip.h DMP_MAX_L: the eigensolver's LDS image)")
    dev = _resolve_device(device)
    N = min(N, MAX_SEQS)
    if state_dict is not None:
        tag = None
    else:
        files = [weights_file] if weights_file is not None else default_weight_files()
        tag = tuple((f, os.path.getmtime(f)) for f in files if os.path.isfile(f))
    with device_lock(dev):
        lru = _ENGINES.lru.setdefault(dev.index, [])
        eng = next((e for e in lru if tag and e.weights_tag == tag), None)
        if eng is None and lru and (not tag or len(lru) >= _EngineCache.MAX_PER_DEVICE):
            eng = lru[0]                                  # recycle the least recently used one (new weights below)
        if eng is not None:
            lru.remove(eng)
        if eng is None or L > eng.max_L or N > eng.max_N:
            max_L = max(L, eng.max_L if eng else 0)
            max_N = max(N, eng.max_N if eng else 0)
            if eng is not None:
                eng.close()
            eng = Engine(dev, max_L, max_N)              # (weights_tag None: packed below)
        lru.append(eng)
        _ENGINES[dev.index] = eng
        want = drop_in_precision()
        if eng.get_option("precision") != want:
            eng.set_option("precision", want)
        if state_dict is not None:
            eng.set_weights(state_dict, tag=None)
        elif eng.weights_tag != tag or not tag:
            eng.set_weights(load_state_dict(weights_file), tag=tag)
    return eng


# ---------------------------------------------------------------------------
# the reference's public functions
# ---------------------------------------------------------------------------
def aln_to_coords(input_file, device=default_device, template=None, iterations=default_iterations,
                  minsteps=default_minsteps, weights_file=None, return_alnmat=False, converge=None,
                  return_distmap=False, native=None, return_scores=False, native_chain=None, compare=None,
                  compare_chain=None, return_alignment=False, search=None, return_hits=False, return_map_scores=False,
                  return_pass_scores=False, return_ss=False, restrain=None, restrain_cutoff=15.0, return_restrain=False,
                  return_exposure=False):
    """Alignment file -> (coords (L,5,3) [N, CA, C, O, CB], confs (L,)) on `device`,
    plus the uint8 alignment matrix when `return_alnmat` is set (predict.py:74-158).
    `converge` (addition; Angstrom, None = off): stop recycling once a pass changes the seed distance map by no more
    than this (RMS) - the answer `iterations` = that pass would have given (Engine.predict).
    `return_distmap` (addition): the (L, L) predicted C-alpha distance map of the pass the best-of rule chose is appended
    as the last element of the returned tuple (after `alnmat` when that is requested too).
    `native` (addition): a PDB file (its chain `native_chain`, default the first, is aligned with the query sequence:
    score.native_from_pdb) or an array as Engine.predict takes it; the model is scored against it on the GPU.  With
    `return_scores` the dict of score.unpack_scores is appended behind everything else (None without a `native`).
    `compare` (addition): a PDB file (its chain `compare_chain`, default the first) or an (m, 3) C-alpha trace of a structure of
    any length and sequence; the model is aligned with it on the GPU (option "align_structure").  With `return_alignment`
    the dict of score.unpack_alignment is appended behind the scores (None without a `compare`).
    `search` (addition): a score.Library, a directory of PDB files or an .npz of tools/make_library.py; the model is aligned
    with every entry on the GPU (option "search_structures").  With `return_hits` the dict of Engine.hits (hits, rank, names)
    is appended behind those (None without a `search`).
    `return_map_scores` (addition; needs `native`): the predicted distance map is scored against the native too (option
    "score_map") and the dict of score.unpack_map_scores is appended behind those.
    `return_pass_scores` (addition; needs `native`): every recycling pass is scored against the native (option
    "score_passes") and the dict of score.unpack_pass_scores is appended behind those.
    `return_ss` (addition): secondary structure is assigned to the final backbone on the GPU (option "assign_ss"; with a whole
    `native` also to the native's rebuilt backbone, with Q3 / Q8) and the dict of score.unpack_ss is appended behind those.
    `restrain` (addition; force constant K in 0 .. 100, None = off) and `restrain_cutoff` (Angstrom): the final refinement also
    pulls the pairs whose predicted distance lies below the cutoff towards it (Engine.predict; the reference has no such
    term).  With `return_restrain` the dict of restrain_report is appended behind those (None without a `restrain` > 0).
    `return_exposure` (addition): the solvent exposure of the final backbone is counted on the GPU (option "exposure"; with a
    whole `native` also that of the native's rebuilt backbone) and the dict of score.unpack_exposure, made with the query's
    sequence, is appended last of all."""
    return _coords_tuple(locals())


def aln_to_domains(input_file, *args, domains_tau=0.25, domains_min_size=40, domains_min_segment=10, **asked):
    """`aln_to_coords` with the model split into structural domains on the GPU (option "domains"; with a whole `native` also
    the native's trace): the same arguments, and the dict of score.unpack_domains - made with the model's coordinates and
    confidences, so every domain has its radius of gyration and mean confidence - appended last of all.  `domains_tau`,
    `domains_min_size`, `domains_min_segment`: domains_options."""
    call = inspect.signature(aln_to_coords).bind(input_file, *args, **asked)
    call.apply_defaults()
    return _coords_tuple(call.arguments, domains_options(domains_tau, domains_min_size, domains_min_segment))


def aln_to_flex(input_file, *args, flex_cutoff=7.3, **asked):
    """`aln_to_coords` with the Gaussian network model of the model's C-alpha trace on the GPU (option "flex"; with a whole
    `native` also of the native's): the same arguments, and the dict of score.unpack_flex - made with the model's confidences,
    so it has the correlations of msf with 1 - confidence - appended last of all.  `flex_cutoff`: the contact cutoff, 4 .. 20
    Angstrom."""
    call = inspect.signature(aln_to_coords).bind(input_file, *args, **asked)
    call.apply_defaults()
    _score.flex_cut_mA(flex_cutoff)                                          # (a bad value raises before any work)
    return _coords_tuple(call.arguments, flex=flex_cutoff)


def aln_to_msa_report(input_file, *args, dca_map=False, **asked):
    """`aln_to_coords` with the report on the alignment made on the GPU (option "msa_report": Neff at three thresholds, gaps,
    copies, the histograms, per-column conservation and the strongest DCA coupling; with a `native` the DCA contact
    precisions): the same arguments, and the dict of score.unpack_msa_report - made with the model's confidences and the
    query, so it has the correlations and the consensus string - appended last of all.  `dca_map`: the raw L x L DCA contact
    map too, as the dict's "dca_map"."""
    call = inspect.signature(aln_to_coords).bind(input_file, *args, **asked)
    call.apply_defaults()
    return _coords_tuple(call.arguments, msa_report=bool(dca_map))


def _coords_tuple(call, domains=None, flex=None, msa_report=None):
    """The arguments of `aln_to_coords` (and, for `aln_to_domains`, what domains_options gave; for `aln_to_flex`, its cutoff; for
    `aln_to_msa_report`, whether the map is wanted) -> what it returns."""
    v = SimpleNamespace(**call)
    r, parse, _, _, flexed, reported = _predict_file_with(domains, v.input_file, v.device, v.template, v.iterations, v.minsteps, v.weights_file, v.converge,
                                  v.native, v.native_chain, v.compare, v.compare_chain, v.search, distmap=v.return_distmap,
                                  scores=v.return_scores, alignment=v.return_alignment, hits=v.return_hits,
                                  map_scores=v.return_map_scores, pass_scores=v.return_pass_scores, ss=v.return_ss,
                                  restrain=v.restrain, restrain_cutoff=v.restrain_cutoff, exposure=v.return_exposure, flex=flex,
                                  msa_report=msa_report)
    return (_as_tuple(r, **{k: call[k] for k in call if k.startswith("return_")}) + ((parse,) if domains is not None else ())
            + ((flexed,) if flex is not None else ()) + ((reported,) if msa_report is not None else ()))


def _as_tuple(r, return_alnmat=False, return_distmap=False, return_scores=False, return_alignment=False, return_hits=False,
              return_map_scores=False, return_pass_scores=False, return_ss=False, return_restrain=False, return_exposure=False):
    return ((r.coords, r.confs) + ((r.alnmat,) if return_alnmat else ()) + ((r.distmap,) if return_distmap else ())
            + ((r.scores,) if return_scores else ()) + ((r.alignment,) if return_alignment else ())
            + ((r.hits,) if return_hits else ()) + ((r.map_scores,) if return_map_scores else ())
            + ((r.pass_scores,) if return_pass_scores else ()) + ((r.ss,) if return_ss else ())
            + ((r.restrain,) if return_restrain else ()) + ((r.exposure,) if return_exposure else ()))


# What `aln_to_coords` computes, by name: each of distmap, scores, alignment, hits and map_scores None unless it was wanted
# (and, for scores, alignment and hits, unless its input - native, compare, search - was given).
# `restrain`: the report of a restrained final refinement, None without one; `exposure`: the dict of score.unpack_exposure.
Prediction = namedtuple("Prediction", "coords confs alnmat distmap scores alignment hits map_scores pass_scores ss restrain exposure",
                        defaults=(None, None, None, None))


def _predict_file(input_file, device, template, iterations, minsteps, weights_file, converge, native, native_chain, compare,
                  compare_chain, search, distmap=False, scores=False, alignment=False, hits=False, map_scores=False,
                  pass_scores=False, ss=False, restrain=None, restrain_cutoff=15.0, exposure=False):
    """`aln_to_coords` -> Prediction; the eight flags are its return_distmap, return_scores, return_alignment, return_hits,
    return_map_scores, return_pass_scores, return_ss and return_exposure; `restrain`, `restrain_cutoff` are its own."""
    return _predict_file_with(None, input_file, device, template, iterations, minsteps, weights_file, converge, native, native_chain,
                              compare, compare_chain, search, distmap, scores, alignment, hits, map_scores, pass_scores, ss,
                              restrain, restrain_cutoff, exposure)[0]



def _predict_file_with(domains, input_file, device, template, iterations, minsteps, weights_file, converge, native, native_chain,
                       compare, compare_chain, search, distmap=False, scores=False, alignment=False, hits=False, map_scores=False,
                       pass_scores=False, ss=False, restrain=None, restrain_cutoff=15.0, exposure=False, score_domains=False, flex=None, msa_report=None):
    """`_predict_file` -> (Prediction, the dict of score.unpack_domains or None, the domain search or None, the domain scores or
    None, the dict of score.unpack_flex or None, the dict of score.unpack_msa_report or None).  `msa_report`: None, or whether
    the DCA contact map is wanted too - the prediction then runs with option "msa_report" (Engine.with_msa_report).  `flex`: None, or the contact cutoff in Angstrom - the prediction then runs
    with option "flex" (Engine.with_flex).  `score_domains` (needs `native`): every domain is scored against the native (Engine.with_score_domains); the fourth
    part is then (the dict of Engine.domain_scores, the dict of score.unpack_domains of the same prediction, the raw block as an
    array).  `domains`: None, or
    what domains_options gave - the prediction then runs with option "domains" (Engine.with_domains).  A `search` library with
    `domains` on is also searched with every domain of the model: the third part is then (the dict of Engine.domain_hits, the
    dict of score.unpack_domains of the same prediction)."""
    restrain_options(restrain, restrain_cutoff)                              # (a bad value raises before any work)
    for option, wanted in (("score_map", map_scores), ("score_passes", pass_scores)):
        if wanted and native is None:
            raise ValueError(needs_native(option, "return_" + _BLOCK_OF[option].name, "`native`"))
    if score_domains and native is None:
        raise ValueError(SCORE_DOMAINS_NEEDS_NATIVE)
    tol = None if converge is None else converge_to_mA(converge) * 1e-3     # (a bad tolerance raises before any work)
    dev = _resolve_device(device)
    aln = read_aln(input_file)
    template_ca = read_template_ca(template) if template is not None else None
    alnmat = encode_aln(aln)
    nseqs, length = alnmat.shape
    if isinstance(native, (str, os.PathLike)):
        native = _score.native_from_pdb(aln[0], native, native_chain)
    if isinstance(compare, (str, os.PathLike)):
        path = compare
        compare = _score.read_native_ca(path, compare_chain)[0]
        if compare.shape[0] == 0:
            raise ValueError(f"{path}: no C-alpha atoms" + (f" in chain {compare_chain}" if compare_chain else ""))
    if compare is not None:
        compare = _score.as_structure(compare)
        if not 3 <= compare.shape[0] <= MAX_L:
            raise ValueError(f"compare: the structure has {compare.shape[0]} C-alpha atoms; 3 to {MAX_L} can be aligned")
    if isinstance(search, (str, os.PathLike)):
        search = _score.Library.open(search)
    if search is not None:
        search.check(MAX_L)
    with device_lock(dev):                  # re-entrant like the reference's function: callers of one GPU take turns
        # (the engine holds both traces: its capacity covers the structure to align with, too)
        cap = max(length, 0 if compare is None else compare.shape[0], 0 if search is None else search.max_m)
        eng = get_engine(dev, cap, nseqs, weights_file=weights_file)
        with (eng.with_domains(domains[0] * 1e-3, *domains[1:]) if domains is not None else contextlib.nullcontext()), \
                (eng.with_score_domains() if score_domains else contextlib.nullcontext()), \
                (eng.with_flex(flex) if flex is not None else contextlib.nullcontext()), \
                (eng.with_msa_report(msa_report) if msa_report is not None else contextlib.nullcontext()):
            out = eng.predict_checked(alnmat, template_ca, iterations, minsteps, converge=tol, distmap=bool(distmap),
                                      native=native, structure=compare, library=search, score_map=bool(map_scores),
                                      score_passes=bool(pass_scores), ss=bool(ss), restrain=restrain,
                                      restrain_cutoff=restrain_cutoff, exposure=bool(exposure))
        parse = eng.domains if domains is not None else None
        domain_hits = (eng.domain_hits, eng.domains) if eng.domain_search_block is not None else None
        domain_scores = ((eng.domain_scores, eng.domains, eng.domain_score_block.cpu().numpy().copy())
                         if eng.domain_score_block is not None else None)
        exposed = None
        if exposure:
            torch.cuda.synchronize(eng.device)
            exposed = _score.unpack_exposure(eng.exposure_block, length, seq=alnmat[0])
        reported = None
        if msa_report is not None:
            torch.cuda.synchronize(eng.device)
            reported = _score.unpack_msa_report(eng.msa_report_block, length, confs=out[1][:length], seq=aln[0])
        return Prediction(out[0], out[1], alnmat, out[2] if distmap else None, ss=eng.ss if ss else None, exposure=exposed,
                          restrain=eng.restrain if restrain is not None else None,
                          map_scores=eng.map_scores if map_scores else None,
                          pass_scores=eng.pass_scores if pass_scores else None,
                          hits=eng.hits if search is not None and hits else None,
                          scores=eng.scores if native is not None and scores else None,
                          alignment=eng.alignment if compare is not None and alignment else None), parse, domain_hits, domain_scores, \
            (eng.flex if flex is not None else None), reported


def pdb_text(coords, confs, alnmat):
    """The PDB text of predict.py:195-208 from host copies of the outputs."""
    coords = coords.detach().cpu()
    confs = confs.detach().cpu()
    lines = ["REMARK  CONF:  " + repr(confs.mean().item())]
    atoms = (" N  ", " CA ", " C  ", " O  ", " CB ")
    xyz, cf = coords.tolist(), confs.tolist()      # Python floats of the float32 values, as .item() gives them
    atomnum = 1
    for ri in range(coords.size(0)):
        code = int(alnmat[0, ri])
        for ai, an in enumerate(atoms):
            if code != 7 or ai != 4:          # glycine has no CB
                x, y, z = xyz[ri][ai]
                lines.append("ATOM   %4d %s %s  %4d    %8.3f%8.3f%8.3f  1.00%6.2f" % (
                    atomnum, an, _RESNAMES[code], ri + 1, x, y, z, cf[ri]))
                atomnum += 1
    lines.append("END")
    return "\n".join(lines) + "\n"


def dmpfold_parser():
    """The reference's flags (predict.py:160-208), -c / --converge, --distmap, --native, --score-map, --score-passes, --compare,
    --search, --ss, --exposure and -r / --restrain."""
    parser = argparse.ArgumentParser(description=(
        "DMPfold2 end-to-end structure prediction on AMD MI355X (HIP engine). "
        "Prints a PDB format model file."))
    parser.add_argument("-i", "--input_file", type=str, required=True,
                        help="input sequence alignment in aln format")
    parser.add_argument("-d", "--device", type=str, default=default_device, required=False,
                        help="device to run on (cuda, cuda:1, ...)")
    parser.add_argument("-t", "--template", type=str, required=False,
                        help="use a PDB file as a template")
    parser.add_argument("-n", "--iterations", type=int, default=default_iterations, required=False,
                        help="number of iteration cycles")
    parser.add_argument("-m", "--minsteps", type=int, default=default_minsteps, required=False,
                        help="number of minimization steps")
    parser.add_argument("-w", "--model_weights", type=str, required=False,
                        help="use a custom set of model weights")
    parser.add_argument("-c", "--converge", type=_tolerance_arg, default=None, required=False, metavar="TOL",
                        help="stop recycling once a pass changes the seed distance map by no more than TOL Angstrom (RMS); "
                             "default: always run all iteration cycles")
    parser.add_argument("--distmap", type=str, default=None, required=False, metavar="FILE",
                        help="also write the predicted C-alpha distance map of the chosen pass to FILE (float32 .npy, L x L)")
    parser.add_argument("--native", type=str, default=None, required=False, metavar="PDB",
                        help="score the model against this native structure on the GPU (TM-score, GDT, RMSD, lDDT-CA); the scores "
                             "go to standard error as one JSON line, the model on standard output is unchanged")
    parser.add_argument("--native-chain", type=str, default=None, required=False, metavar="C",
                        help="chain of --native (default: its first)")
    parser.add_argument("--score-map", action="store_true", default=False,
                        help="with --native: also score the predicted distance map against the native on the GPU (contact precision "
                             "of the top L, L/2, L/5 per separation class, lDDT and distance error of the map); the JSON line of "
                             "--native gains the key \"map\"")
    parser.add_argument("--score-passes", action="store_true", default=False,
                        help="with --native: score every recycling pass against the native on the GPU, not only the one the "
                             "confidence picked (per pass: mean confidence logit, convergence delta, TM-score, GDT, RMSD, lDDT-CA; "
                             "which pass was best, and what the choice cost); the JSON line of --native gains the key \"passes\"")
    parser.add_argument("--scores", type=str, default=None, required=False, metavar="FILE",
                        help="write the JSON line of --native to FILE instead of standard error")
    parser.add_argument("--compare", type=str, default=None, required=False, metavar="PDB",
                        help="align the model on the GPU with this structure of any length and sequence (structural alignment, "
                             "TM-scores by both lengths, superposition); the result goes to standard error as one JSON line, the "
                             "model on standard output is unchanged")
    parser.add_argument("--compare-chain", type=str, default=None, required=False, metavar="C",
                        help="chain of --compare (default: its first)")
    parser.add_argument("--alignment", type=str, default=None, required=False, metavar="FILE",
                        help="write the JSON line of --compare to FILE instead of standard error")
    parser.add_argument("--search", type=str, default=None, required=False, metavar="DIR|FILE.npz",
                        help="align the model on the GPU with every structure of a fold library (a directory of PDB files or an "
                             ".npz of tools/make_library.py) and rank them by TM-score; the best hits go to standard error as one "
                             "JSON line, the model on standard output is unchanged")
    parser.add_argument("--search-top", type=int, default=10, required=False, metavar="N",
                        help="how many hits of --search to report (default 10)")
    # --search-refine R (with --search): screen every entry by its best gapless threading and refine only the best R by that;
    # the JSON line gains "refine" and every hit "refined".  The help text and the parsed namespace of the other flags are
    # recorded (tests/golden/host_plumbing.json.gz): the flag stays out of both unless given, and README.md describes it.
    parser.add_argument("--search-refine", type=int, default=argparse.SUPPRESS, required=False, metavar="R", help=argparse.SUPPRESS)
    # --search-domains (with --search): search the library with every domain of the model as well (option "search_domains", which
    # splits the model by the parameters of --domains, or the defaults); the JSON line of --search gains the key "domain_hits".
    # Hidden like --search-refine, for the same reason; README.md describes it.
    parser.add_argument("--search-domains", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    # --score-domains (with --native): score every domain of the model's parse - and of the native's, where it is whole - against the
    # native on its own superposition (option "score_domains", which splits the model by the parameters of --domains, or the
    # defaults); the JSON line of --native gains the key "domain_scores".  Hidden like --search-refine, for the same reason;
    # README.md describes it.
    parser.add_argument("--score-domains", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    parser.add_argument("--hits", type=str, default=None, required=False, metavar="FILE",
                        help="write the JSON line of --search to FILE instead of standard error")
    parser.add_argument("--ss", action="store_true", default=False,
                        help="assign secondary structure to the model's backbone on the GPU from its hydrogen bonds (eight-state and "
                             "three-state strings, counts, helix / strand / coil fractions; with --native given whole also the "
                             "native's and Q3 / Q8); the result goes to standard error as one JSON line, the model on standard "
                             "output is unchanged")
    parser.add_argument("--ss-file", type=str, default=None, required=False, metavar="FILE",
                        help="write the JSON line of --ss to FILE instead of standard error")
    parser.add_argument("--exposure", action="store_true", default=False,
                        help="count the solvent exposure of the model's backbone on the GPU (a Shrake-Rupley surface of N, CA, C, O "
                             "and CB with 256 points per atom, half-sphere exposure and CB contact number per residue, the burial of "
                             "the hydrophobic positions; with --native given whole also the native's and their correlations); the "
                             "result goes to standard error as one JSON line under the key \"exposure\", the model on standard "
                             "output is unchanged")
    parser.add_argument("--exposure-file", type=str, default=None, required=False, metavar="FILE",
                        help="write the JSON line of --exposure to FILE instead of standard error")
    # --domains [--domains-tau Q --domains-min-size N --domains-min-segment N] [--domains-file FILE]: split the model into
    # structural domains on the GPU (a contact-density bisection; with --native given whole also the native's trace and the
    # overlap of the two parses); the result goes to standard error, or to FILE, as one JSON line under the key "domains", the
    # model on standard output is unchanged.  Hidden like --search-refine, for the same reason; README.md describes it.
    parser.add_argument("--domains", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    parser.add_argument("--domains-tau", type=float, default=argparse.SUPPRESS, metavar="Q", help=argparse.SUPPRESS)
    parser.add_argument("--domains-min-size", type=int, default=argparse.SUPPRESS, metavar="N", help=argparse.SUPPRESS)
    parser.add_argument("--domains-min-segment", type=int, default=argparse.SUPPRESS, metavar="N", help=argparse.SUPPRESS)
    parser.add_argument("--domains-file", type=str, default=argparse.SUPPRESS, metavar="FILE", help=argparse.SUPPRESS)
    # --flex [--flex-cutoff A] [--flex-file FILE]: the Gaussian network model of the model's C-alpha trace on the GPU (contacts
    # within A Angstrom, 7.3 by default; the eight lowest modes, the hinges of the slowest, the slow-mode fluctuation and its
    # correlation with 1 - confidence; with --native given whole also the native's); the result goes to standard error, or to
    # FILE, as one JSON line under the key "flex", the model on standard output is unchanged.  Hidden like --search-refine, for
    # the same reason; README.md describes it.
    parser.add_argument("--flex", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    parser.add_argument("--flex-cutoff", type=float, default=argparse.SUPPRESS, metavar="A", help=argparse.SUPPRESS)
    parser.add_argument("--flex-file", type=str, default=argparse.SUPPRESS, metavar="FILE", help=argparse.SUPPRESS)
    # --msa-report [--msa-report-file FILE] [--dca-map FILE.npy]: a report on the alignment made on the GPU (Neff at 62, 80 and
    # 90 % identity, gaps, copies, histograms of identity, coverage and nearest neighbour, per-column conservation, the strongest
    # DCA coupling per column; with --native the DCA contact precisions); the result goes to standard error, or to FILE, as one
    # JSON line under the key "msa"; --dca-map (which implies --msa-report) saves the raw L x L DCA contact map.  The model on
    # standard output is unchanged.  Hidden like --search-refine, for the same reason; README.md describes it.
    parser.add_argument("--msa-report", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    parser.add_argument("--msa-report-file", type=str, default=argparse.SUPPRESS, metavar="FILE", help=argparse.SUPPRESS)
    parser.add_argument("--dca-map", type=str, default=argparse.SUPPRESS, metavar="FILE.npy", help=argparse.SUPPRESS)
    add_restrain_arguments(parser, "-r")
    return parser


def domains_arguments(parser, args):
    """What --domains and its companions ask for: None without --domains, else what domains_options makes of them (a bad
    value, or a companion without --domains, is an error of the command line)."""
    given = {k: getattr(args, "domains_" + k) for k in ("tau", "min_size", "min_segment") if hasattr(args, "domains_" + k)}
    if not hasattr(args, "domains"):
        if given or hasattr(args, "domains_file"):
            parser.error("--domains-tau, --domains-min-size, --domains-min-segment and --domains-file need --domains")
        return None
    try:
        return domains_options(**given)
    except ValueError as exc:
        parser.error(str(exc))


def flex_arguments(parser, args):
    """What --flex and its companions ask for: None without --flex, else the cutoff in Angstrom (a bad value, or a companion
    without --flex, is an error of the command line)."""
    if not hasattr(args, "flex"):
        if hasattr(args, "flex_cutoff") or hasattr(args, "flex_file"):
            parser.error("--flex-cutoff and --flex-file need --flex")
        return None
    cutoff = getattr(args, "flex_cutoff", 7.3)
    try:
        _score.flex_cut_mA(cutoff)
    except ValueError as exc:
        parser.error(str(exc))
    return cutoff


def run_dmpfold(argv=None):
    """Command-line entry point with the reference's flags (predict.py:160-208)."""
    parser = dmpfold_parser()
    args = parser.parse_args(argv)
    for option in NATIVE_NEEDED:
        if getattr(args, option) and args.native is None:
            parser.error(needs_native(option, "--" + option.replace("_", "-"), "--native"))
    search = args.search
    if hasattr(args, "search_refine"):
        if args.search is None:
            parser.error("--search-refine needs --search")
        if not 0 <= args.search_refine <= _score.SEARCH_MAX:
            parser.error(f"--search-refine must be 0 or 1 .. {_score.SEARCH_MAX}, got {args.search_refine}")
        search = _score.Library.open(args.search, refine=args.search_refine)
    if hasattr(args, "search_domains"):
        if args.search is None:
            parser.error("--search-domains needs --search")
        search = search if isinstance(search, _score.Library) else _score.Library.open(args.search)
        search.domains = True
    if hasattr(args, "score_domains") and args.native is None:
        parser.error("--score-domains needs --native")
    domains = domains_arguments(parser, args)
    flex = flex_arguments(parser, args)
    if hasattr(args, "msa_report_file") and not (hasattr(args, "msa_report") or hasattr(args, "dca_map")):
        parser.error("--msa-report-file needs --msa-report")
    msa_report = hasattr(args, "dca_map") if hasattr(args, "msa_report") or hasattr(args, "dca_map") else None
    r, parse, domain_hits, domain_scores, flexed, reported = _predict_file_with(domains, args.input_file, args.device, args.template, args.iterations, args.minsteps,
                                  args.model_weights, args.converge, args.native, args.native_chain, args.compare,
                                  args.compare_chain, search, distmap=args.distmap is not None, scores=args.native is not None,
                                  alignment=args.compare is not None, hits=args.search is not None, map_scores=args.score_map,
                                  pass_scores=args.score_passes, ss=args.ss, restrain=args.restrain,
                                  restrain_cutoff=args.restrain_cutoff, exposure=args.exposure,
                                  score_domains=hasattr(args, "score_domains"), flex=flex, msa_report=msa_report)

    def json_line(obj, path):
        """one JSON line to the file `path`, or to standard error without one"""
        with (open(path, "w") if path is not None else contextlib.nullcontext(sys.stderr)) as fh:
            fh.write(json.dumps(obj) + "\n")
    if args.search is not None:
        js = _score.BLOCK["search"].json(r.hits, top=args.search_top)
        if domain_hits is not None:                        # (--search-domains)
            ds, dom = domain_hits
            js["domain_hits"] = _score.domain_hits_json(ds, ds["names"], dom, args.search_top, ds.get("refine", 0))["domains"]
        json_line(js, args.hits)
    if args.distmap is not None:
        save_distmap_npy(args.distmap, r.distmap)
    if args.compare is not None:
        json_line(_score.alignment_json(r.alignment), args.alignment)
    if args.native is not None:
        js = _score.scores_json(r.scores)
        if r.map_scores is not None:
            js["map"] = _score.map_scores_json(r.map_scores)
        if r.pass_scores is not None:
            js["passes"] = _score.pass_scores_json(r.pass_scores)
        if domain_scores is not None:                      # (--score-domains)
            js["domain_scores"] = _score.domain_scores_json(domain_scores[0], domain_scores[1])
        json_line(js, args.scores)
    if args.ss:
        json_line(_score.ss_json(r.ss), args.ss_file)
    if args.exposure:
        json_line({"exposure": _score.exposure_json(r.exposure)}, args.exposure_file)
    if parse is not None:
        json_line({"domains": _score.domains_json(parse)}, getattr(args, "domains_file", None))
    if flexed is not None:
        json_line({"flex": _score.flex_json(flexed)}, getattr(args, "flex_file", None))
    if reported is not None:
        json_line({"msa": _score.msa_report_json(reported)}, getattr(args, "msa_report_file", None))
        if hasattr(args, "dca_map"):
            np.save(args.dca_map, np.asarray(reported["dca_map"], dtype=np.float32))
    if r.restrain is not None:
        json_line({"restrain": r.restrain}, None)
    sys.stdout.write(pdb_text(r.coords, r.confs, r.alnmat))
