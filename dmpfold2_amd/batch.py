"""Batch front end: many independent alignments -> one PDB file each, sharded over the GPUs of a node.

    python -m dmpfold2_amd.batch -l targets.txt -o out_dir [-n 10] [-m 100] [-w weights.pt] [--streams 3]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m dmpfold2_amd.batch -l targets.txt -o out_dir

    python -m dmpfold2_amd.batch -i msa_dir more.aln other.a3m -o out_dir --format ca

`targets.txt` holds one alignment path per line (.aln, or .a3m converted as the reference's README
describes), optionally followed by a template PDB path; `-i` takes alignment files and directories
(every *.aln / *.a3m inside, sorted).  `--format`: `pdb` (default) = the text of the single-target CLI
(N, CA, C, O, CB records, confidence in the B-factor column and the REMARK line, predict.py:195-208),
`ca` = the same records for the CA atoms only, `npz` = coords (L,5,3), confs (L,), alnmat as arrays.  The
reference has no batch mode (its CLI takes one alignment, predict.py:160-208); this is the
"independent alignments shard embarrassingly" axis of SURVEY.md section 8e: every rank (one process
per GPU) takes the targets `shard.partition_targets` assigns to it (longest first), runs them through
a `Pipeline` (several targets in flight per GPU) and writes `<out_dir>/<alignment basename>.pdb` with
the text of the single-target CLI.  No collective on the data path; `torch.distributed` only sums the
target count and takes the maximum elapsed time for the summary line.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import hashlib
import os
import sys
import time

import numpy as np
import torch

from . import score as _score
from .score import Outputs
from . import shard
from .predict import (MAX_SEQS, Pipeline, domains_options, _tolerance_arg, drop_in_precision, default_iterations, default_minsteps, encode_aln, load_state_dict,
                      pdb_text, read_a3m, read_aln, read_template_ca, save_distmap_npy, add_restrain_arguments, restrain_cutoff_to_mA,
                      restrain_report, restrain_to_milli, needs_native, NATIVE_NEEDED)


class BatchFailures(RuntimeError):
    """Some targets of a shard failed; the PDB files of all the others were written."""

    def __init__(self, failed, n_done, elapsed, outputs):
        self.failed, self.n_done, self.elapsed, self.outputs = failed, n_done, elapsed, outputs
        super().__init__(f"{len(failed)} targets failed (the {len(outputs)} PDB files of the others "
                         "were written): " + ", ".join(f"{a} ({type(e).__name__}: {e})" for a, e in failed))


def read_target_list(path):
    """[(alignment path, template path or None)] from a text file (blank lines and # comments skipped)."""
    out = []
    with open(path) as fh:
        for line in fh:
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            parts = line.split()
            out.append((parts[0], parts[1] if len(parts) > 1 else None))
    return out


def expand_inputs(inputs):
    """Files and directories -> [(alignment path, None)]; a directory contributes its *.aln and *.a3m
    files in sorted order.  The reference README's workflow converts x.a3m to x.aln in the same
    directory: where a directory holds both, only x.aln is taken (both would be written to x.pdb)."""
    out = []
    for item in inputs:
        if os.path.isdir(item):
            names = sorted(f for f in os.listdir(item) if f.endswith((".aln", ".a3m")))
            have_aln = {f[:-4] for f in names if f.endswith(".aln")}
            out += [(os.path.join(item, f), None) for f in names
                    if f.endswith(".aln") or f[:-4] not in have_aln]
        else:
            out.append((item, None))
    return out


def check_output_stems(targets):
    """Two targets with the same basename would be written to the same <out_dir>/<stem> file (and, sharded,
    by two ranks at once): refuse the job before anything is predicted."""
    seen = {}
    for aln_path, _ in targets:
        stem = os.path.splitext(os.path.basename(aln_path))[0]
        if stem in seen and seen[stem] != aln_path:
            raise ValueError(f"targets {seen[stem]} and {aln_path} would both be written to {stem}.*: "
                             "rename one of them or run them into different output directories")
        seen[stem] = aln_path


def scan_target(aln_path):
    """(L, N) of an alignment WITHOUT parsing it: the length of its first sequence line and the number of lines that
    do not start with '>' (the rows the reference keeps, predict.py:100-104) - counted on the raw bytes, so a missing
    final newline or trailing blanks on the first line do not change the count (a size / line-length estimate came
    out one or more rows short for such files, and the engines were then built too small for their deepest
    target).  Every rank scans every target so that all ranks compute the same partition; only the owner of a target
    decodes and encodes it.  An unreadable file scans as (0, 0): its owner reports the error when it reads it."""
    a3m = aln_path.endswith(".a3m")
    lines = headers = size = 0
    head, last, prev_nl = b"", b"", True                  # prev_nl: the byte before this chunk was a newline (or none)
    try:
        with open(aln_path, "rb") as fh:
            while True:                                  # fixed-size chunks: a rank never holds a whole multi-GB a3m set
                chunk = fh.read(1 << 20)
                if not chunk:
                    break
                if len(head) < (1 << 16):
                    head += chunk[:(1 << 16) - len(head)]
                size += len(chunk)
                lines += chunk.count(b"\n")
                headers += chunk.count(b"\n>") + (1 if prev_nl and chunk.startswith(b">") and (size > len(chunk)) else 0)
                prev_nl = chunk.endswith(b"\n")
                last = chunk[-1:]
    except OSError:
        return 0, 0
    if not size:
        return 0, 0
    lines += 0 if last == b"\n" else 1
    headers += 1 if head.startswith(b">") else 0
    L = 0
    for raw in head.split(b"\n", 64):                    # the first sequence line is within the first few lines
        if not raw.startswith(b">"):
            L = sum(1 for ch in raw.rstrip() if not (a3m and 97 <= ch <= 122))
            break
    return L, max(1, lines - headers)


def plan_shard(targets, iterations, rank, world):
    """Indices of the targets rank `rank` of `world` owns, longest first.  Deterministic and identical on every
    rank (it depends only on the header scans), every target exactly once over the ranks."""
    costs = [shard.estimate_cost(L, N, iterations) for L, N in (scan_target(a) for a, _ in targets)]
    return shard.partition_targets(costs, world)[rank]


def ca_only_text(coords, confs, alnmat):
    """The CLI's PDB text reduced to its CA records (atom serial numbers renumbered 1..L)."""
    keep = [ln for ln in pdb_text(coords, confs, alnmat).split("\n") if not ln.startswith("ATOM") or ln[12:16] == " CA "]
    out, k = [], 0
    for ln in keep:
        if ln.startswith("ATOM"):
            k += 1
            ln = "ATOM   %4d" % k + ln[11:]
        out.append(ln)
    return "\n".join(out)


RESTRAIN_COUNTS = ("steps", "restrained_pairs", "clashes")      # the integers of predict.restrain_report


NESTED = {"score_map": "map", "passes": "passes"}       # the blocks whose JSON form goes inside the scores', and under which key


def results_json(results, top=10):
    """{name: JSON form} of the unpacked results given (each by the `name` of its row of score.BLOCKS), the map scores and the
    pass table inside the scores' under "map" and "passes" - and only there: without scores they are nowhere."""
    out = {row.name: row.json(results[row.name], top=top) for row in _score.BLOCKS
           if results.get(row.name) is not None and row.key not in NESTED}
    for key, inside in NESTED.items():
        if results.get(_score.BLOCK[key].name) is not None and "scores" in out:
            out["scores"][inside] = _score.BLOCK[key].json(results[_score.BLOCK[key].name])
    return out


def domain_hits_form(domain_hits, domains=None, top=10):
    """The JSON form of a target's domain search (the dict of Engine.domain_hits; `domains`: the dict of score.unpack_domains)."""
    return _score.domain_hits_json(domain_hits, domain_hits["names"], domains, top, domain_hits.get("refine", 0))


def write_result(out_dir, aln_path, coords, confs, alnmat, fmt="pdb", distmap=None, info=None, *, hits_top=10, restrain=None,
                 **results):
    """One target's output file; returns its path.  With `distmap` (L, L) and `info` = [best_pass, passes_run, map_rms]
    (--distmap): npz gains the arrays distmap, best_pass, passes_run and map_rms; pdb / ca get <stem>.distmap.npy beside
    the structure (float32, as `dmpfold --distmap` writes it).  With `scores` (the dict of score.unpack_scores, --natives):
    npz gains n_pairs, lnorm, rmsd, tm, gdt_ts, gdt_ha, lddt, counts, R, t, lddt_res and deviation; pdb / ca get
    <stem>.scores.json (the line `dmpfold --native` prints).  With `alignment` (the dict of score.unpack_alignment,
    --structures): npz gains the header fields of score.ALIGN_NAMES, ali, ali_R, ali_t and ali_deviation; pdb / ca get
    <stem>.alignment.json (the line `dmpfold --compare` prints).  With `hits` (the dict of Engine.hits: hits, rank, names;
    --library): npz gains hit_rank, hit_tm_model, hit_tm_struct (per entry, in the library's order) and hit_names; pdb / ca get
    <stem>.hits.json (the line `dmpfold --search` prints, the best `hits_top`).  With `map_scores` (the dict of
    score.unpack_map_scores, --natives --score-map; only beside `scores`): npz gains map_n, map_ln, map_pairs, map_lddt,
    map_mae, map_rmse, map_bias, map_lddt_res and map_counts (int32 (4, 10): per class short, medium, long, medium + long the
    candidates, native contacts, hits and taken of the lists L, L/2, L/5, true positives and predicted contacts at 8 A);
    <stem>.scores.json gains the key "map".  With `pass_scores` (the dict of score.unpack_pass_scores, --natives
    --score-passes; only beside `scores`): npz gains pass_rows, pass_best, pass_tm_best, pass_lddt_best (int32, -1 for none),
    pass_regret_tm, pass_regret_lddt and one float32 array (R,) per column, pass_conf_mean, pass_delta, pass_tm, pass_gdt_ts,
    pass_gdt_ha, pass_rmsd, pass_lddt; <stem>.scores.json gains the key "passes".  With `ss` (the dict of score.unpack_ss,
    --ss): npz gains ss8 (the string), ss_bp (int32 (L, 2): the two bridge partners), ss_e_acc, ss_e_don (float32 (L,)),
    ss_p_acc, ss_p_don (int32 (L,)) and, with a whole native, ss8_native, ss_q3 and ss_q8; pdb / ca get <stem>.ss.json (the
    line `dmpfold --ss` prints).  With `restrain` (the dict of predict.restrain_report, --restrain): npz gains the scalars
    restrain_k, restrain_cutoff, restrain_steps, restrain_map_rms, restrain_restrained_pairs, restrain_clashes and
    restrain_bond_dev_max; pdb / ca get <stem>.restrain.json (the line `dmpfold --restrain` prints).  With `exposure` (the dict of
    score.unpack_exposure, --exposure): npz gains exp_n (int32 (L, 5): exposed points of N, CA, C, O, CB, -1 for a glycine's CB),
    exp_hse_up, exp_hse_down, exp_cn10 (int32 (L,)) and exp_area (float64 (L,): the residue's accessible area in square
    Angstrom); pdb / ca get <stem>.exposure.json (the line `dmpfold --exposure` prints).  With `domains` (the dict of
    score.unpack_domains, --domains): npz gains dom_label (int32 (L,): every residue's domain) and dom_table (int32 (domains, 8):
    size, segments, lowest residue, contact pairs inside and to the rest, ext and denominator of the cut, level); pdb / ca get
    <stem>.domains.json (the line `dmpfold --domains` prints).  With `domain_hits` (the dict of Engine.domain_hits, --library
    --search-domains; beside `domains`): npz gains dom_hit_rank (int32 (D, K): per domain the entries by falling TM-score) and
    dom_hit_tm (float32 (D, K): pair (d, k)'s TM-score normalised by the domain's size, in the library's order); pdb / ca get
    <stem>.domain_hits.json (score.domain_hits_json, the best `hits_top` per domain).  With `domain_scores` (the dict of
    score.unpack_domain_scores, --natives --score-domains; only beside `scores`): npz gains dom_score_table (float32 (2, 16, 32):
    the two tables of the domain-score block) and dom_score_res (float32 (4, L): per leg the per-residue lDDT and deviation inside
    the residue's own domain); <stem>.scores.json gains the key "domain_scores" (score.domain_scores_json).  With `flex` (the dict
    of score.unpack_flex, --flex): npz gains flex_eig (float32 (8,): the model's eight lowest eigenvalues), flex_modes (float32
    (8, L)), flex_msf (float32 (L,)) and flex_degree (int32 (L,)); pdb / ca get <stem>.flex.json (the line `dmpfold --flex`
    prints).  With `msa_report` (the dict of score.unpack_msa_report, --msa-report): npz gains msa_header (float32 (128,)) and
    msa_columns (float32 (8, L)) and, with --dca-map, dca_map (float32 (L, L)); pdb / ca get <stem>.msa.json (the line `dmpfold
    --msa-report` prints) and <stem>.dca_map.npy."""
    msa_report = results.pop("msa_report", None)
    domain_hits = results.pop("domain_hits", None)
    domain_scores = results.pop("domain_scores", None)
    flex = results.pop("flex", None)
    unknown = set(results) - {row.name for row in _score.BLOCKS}
    if unknown:
        raise TypeError(f"write_result: no result is called {sorted(unknown)}")
    scores, map_scores, pass_scores, ss, exposure, domains, alignment, hits = (results.get(row.name) for row in _score.BLOCKS)
    stem = os.path.join(out_dir, os.path.splitext(os.path.basename(aln_path))[0])
    if fmt == "npz":
        path = stem + ".npz"
        extra = {}
        if distmap is not None:
            h_info = info.detach().cpu().numpy()
            extra = {"distmap": distmap.detach().cpu().numpy(), "best_pass": np.int32(h_info[0]),
                     "passes_run": np.int32(h_info[1]), "map_rms": np.float32(h_info[2])}
        if scores is not None:
            extra.update({"n_pairs": np.int32(scores["n_pairs"]), "lnorm": np.float32(scores["lnorm"]),
                          "counts": np.asarray(scores["counts"], dtype=np.int32)})
            extra.update({k: np.float32(scores[k]) for k in _score.SCORE_NAMES[1:]})
            extra.update({k: np.asarray(scores[k], dtype=np.float32) for k in ("R", "t", "lddt_res", "deviation")})
        if map_scores is not None:
            extra.update({"map_n": np.int32(map_scores["n"]), "map_ln": np.float32(map_scores["ln"]),
                          "map_pairs": np.int32(map_scores["pairs"]),
                          "map_lddt_res": np.asarray(map_scores["map_lddt_res"], dtype=np.float32),
                          "map_counts": np.asarray([[cl["candidates"], cl["native_contacts"]] + cl["hits"] + cl["taken"]
                                                    + [cl["tp"], cl["predicted"]]
                                                    for cl in (map_scores["classes"][c] for c in _score.MAP_CLASSES)], dtype=np.int32)})
            extra.update({k: np.float32(map_scores[k]) for k in _score.MAP_NAMES})
        if pass_scores is not None:
            extra.update({"pass_rows": np.int32(pass_scores["rows"]), "pass_regret_tm": np.float32(pass_scores["regret_tm"]),
                          "pass_regret_lddt": np.float32(pass_scores["regret_lddt"])})
            extra.update({"pass_" + k: np.int32(-1 if pass_scores[name] is None else pass_scores[name])
                          for k, name in (("best", "best_pass"), ("tm_best", "tm_pass"), ("lddt_best", "lddt_pass"))})
            extra.update({"pass_" + k: np.asarray(pass_scores[k], dtype=np.float32) for k in _score.PASS_COLUMNS})
        if ss is not None:
            extra.update({"ss8": np.asarray(ss["ss8"], dtype=np.str_), "ss_bp": np.stack([ss["bp1"], ss["bp2"]], axis=1).astype(np.int32),
                          "ss_e_acc": np.asarray(ss["e_acc"], dtype=np.float32), "ss_e_don": np.asarray(ss["e_don"], dtype=np.float32),
                          "ss_p_acc": np.asarray(ss["p_acc"], dtype=np.int32), "ss_p_don": np.asarray(ss["p_don"], dtype=np.int32)})
            if ss["has_native"]:
                extra.update({"ss8_native": np.asarray(ss["ss8_native"], dtype=np.str_), "ss_q3": np.float32(ss["q3"]),
                              "ss_q8": np.float32(ss["q8"])})
        if exposure is not None:
            extra.update({"exp_n": np.asarray(exposure["n"], dtype=np.int32), "exp_area": np.asarray(exposure["area_res"], dtype=np.float64)})
            extra.update({"exp_" + k: np.asarray(exposure[k], dtype=np.int32) for k in ("hse_up", "hse_down", "cn10")})
        if domains is not None:
            extra.update({"dom_label": np.asarray(domains["labels"], dtype=np.int32),
                          "dom_table": np.asarray([[row[k] for k in _score.DOMAINS_COLUMNS] for row in domains["table"]],
                                                  dtype=np.int32).reshape(-1, len(_score.DOMAINS_COLUMNS))})
        if restrain is not None:
            extra.update({"restrain_" + k: (np.int32 if k in RESTRAIN_COUNTS else np.float32)(v) for k, v in restrain.items()})
        if alignment is not None:
            extra.update({k: (np.int32 if k in ("n_ali", "seed_offset", "seeds") else np.float32)(alignment[k])
                          for k in _score.ALIGN_NAMES})
            extra.update({"ali": np.asarray(alignment["ali"], dtype=np.int32), "ali_R": np.asarray(alignment["R"], dtype=np.float32),
                          "ali_t": np.asarray(alignment["t"], dtype=np.float32),
                          "ali_deviation": np.asarray(alignment["deviation"], dtype=np.float32)})
        if hits is not None:
            extra.update({"hit_rank": np.asarray(hits["rank"], dtype=np.int32),
                          "hit_tm_model": np.asarray([h["tm_model"] for h in hits["hits"]], dtype=np.float32),
                          "hit_tm_struct": np.asarray([h["tm_struct"] for h in hits["hits"]], dtype=np.float32),
                          "hit_names": np.asarray(hits["names"], dtype=np.str_)})
            if "refined" in hits:                        # (--search-refine)
                extra["hit_refined"] = np.asarray(hits["refined"], dtype=np.bool_)
        if domain_hits is not None:
            D, K = domain_hits["domains"], len(domain_hits["names"])
            extra.update({"dom_hit_rank": np.asarray(domain_hits["rank"], dtype=np.int32).reshape(D, K),
                          "dom_hit_tm": np.asarray(domain_hits["headers"][:D, :, 2], dtype=np.float32).reshape(D, K)})
        if domain_scores is not None and scores is not None:
            extra.update({"dom_score_table": np.asarray(domain_scores["table"], dtype=np.float32),
                          "dom_score_res": np.asarray(domain_scores["res"], dtype=np.float32)})
        if flex is not None:
            extra.update({"flex_eig": np.asarray(flex["eigenvalues"], dtype=np.float32), "flex_modes": np.asarray(flex["modes"], dtype=np.float32),
                          "flex_msf": np.asarray(flex["msf"], dtype=np.float32), "flex_degree": np.asarray(flex["degree"], dtype=np.int32)})
        if msa_report is not None:
            extra.update({"msa_header": np.asarray(msa_report["header"], dtype=np.float32),
                          "msa_columns": np.asarray(msa_report["columns"], dtype=np.float32)})
            if "dca_map" in msa_report:
                extra["dca_map"] = np.asarray(msa_report["dca_map"], dtype=np.float32)
        np.savez_compressed(path, coords=coords.detach().cpu().numpy(), confs=confs.detach().cpu().numpy(),
                            alnmat=alnmat, **extra)
        return path
    if distmap is not None:
        save_distmap_npy(stem + ".distmap.npy", distmap)
    forms = results_json(results, hits_top)
    if domain_hits is not None:
        forms["domain_hits"] = domain_hits_form(domain_hits, domains, hits_top)
    if domain_scores is not None and "scores" in forms:
        forms["scores"]["domain_scores"] = _score.domain_scores_json(domain_scores, domains)
    for name, value in (("exposure", forms.get("exposure")), ("domains", forms.get("domains")), ("restrain", restrain),
                        ("flex", None if flex is None else _score.flex_json(flex))):
        if value is not None:
            forms[name] = {name: value}                  # (these lines carry their name)
    if msa_report is not None:
        forms["msa"] = {"msa": _score.msa_report_json(msa_report)}
        if "dca_map" in msa_report:
            np.save(stem + ".dca_map.npy", np.asarray(msa_report["dca_map"], dtype=np.float32))
    for name, form in forms.items():
        with open(f"{stem}.{name}.json", "w") as fh:
            fh.write(json.dumps(form) + "\n")
    path = stem + ".pdb"
    with open(path, "w") as fh:
        fh.write(pdb_text(coords, confs, alnmat) if fmt == "pdb" else ca_only_text(coords, confs, alnmat))
    return path


class _StaticQueue:
    """This rank's share of a static partition (shard.partition_targets on the header scans), longest first."""

    def __init__(self, indices):
        self._it = iter(indices)

    def take(self):
        return next(self._it, None)


class _SharedQueue:
    """One queue for all ranks: the targets in descending order of estimated cost, handed out by an atomic counter
    in the job's torch.distributed key-value store (host side; no collective, nothing on the data path).  A rank
    that finishes early simply keeps taking targets: no tail of idle GPUs behind a mis-estimated partition."""

    _calls = {}          # per process: how many queues were made over each target list (ranks call run_batch in step)

    def __init__(self, order, store, tag=""):
        # one counter per JOB: a second run_batch over the same store must not continue the first one's counter (it
        # would find it exhausted and silently predict nothing), so the key carries the target list's digest and the
        # number of earlier queues this process made over that list - the same on every rank of an SPMD job
        nth = _SharedQueue._calls.get(tag, 0)
        _SharedQueue._calls[tag] = nth + 1
        self._order, self._store, self._key = list(order), store, f"dmpfold_batch_next/{tag}/{nth}"

    def take(self):
        # an exhausted counter is a normal state, also at a rank's FIRST take (more ranks than targets, or a rank that
        # starts after the others have taken everything): that rank has nothing to do and must still reach the job's
        # summary reduction, so this never raises
        k = int(self._store.add(self._key, 1)) - 1
        return self._order[k] if k < len(self._order) else None


def cost_order(targets, iterations):
    """(indices in descending order of estimated cost, scans): identical on every rank."""
    scans = [scan_target(a) for a, _ in targets]
    costs = [shard.estimate_cost(L, N, iterations) for L, N in scans]
    return sorted(range(len(targets)), key=lambda i: (-costs[i], i)), scans


# --domains: what run_batch asks of its pipeline beside its own arguments, whose list callers know by position -
# (tau, min_size, min_segment) or None; `batch_domains` sets it for the duration of a block.
_DOMAINS = None


@contextlib.contextmanager
def batch_domains(tau=0.25, min_size=40, min_segment=10):
    """Every run_batch inside the block also splits every target's model into structural domains on the GPU
    (Pipeline.use_domains): the parse is written with the target (write_result) and `stats_out` receives "domains":
    {stem: the dict of score.domains_json}."""
    global _DOMAINS
    domains_options(tau, min_size, min_segment)                              # (a bad value raises before any work)
    before, _DOMAINS = _DOMAINS, (tau, min_size, min_segment)
    try:
        yield
    finally:
        _DOMAINS = before


_SCORE_DOMAINS = False
_FLEX = None                                            # --flex: the contact cutoff in Angstrom, or None
_MSA_REPORT = None                                      # --msa-report: whether the DCA contact map is wanted too, or None


@contextlib.contextmanager
def batch_msa_report(dca_map=False):
    """Every run_batch inside the block also reports on every target's alignment on the GPU (Pipeline.use_msa_report; `dca_map`:
    with the raw DCA contact map): the result is written with the target (write_result) and `stats_out` receives "msa": {stem:
    N, neff_80, median_coverage}."""
    global _MSA_REPORT
    before, _MSA_REPORT = _MSA_REPORT, bool(dca_map)
    try:
        yield
    finally:
        _MSA_REPORT = before


@contextlib.contextmanager
def batch_flex(cutoff=7.3):
    """Every run_batch inside the block also gives every target's model its Gaussian network model on the GPU (Pipeline.use_flex;
    contacts within `cutoff` Angstrom): the result is written with the target (write_result) and `stats_out` receives "flex":
    {stem: lambda_1, components, hinges, r_conf of the model's leg}."""
    global _FLEX
    _score.flex_cut_mA(cutoff)                          # (a bad value raises before any work)
    before, _FLEX = _FLEX, float(cutoff)
    try:
        yield
    finally:
        _FLEX = before


@contextlib.contextmanager
def batch_score_domains():
    """Every run_batch inside the block, which must be given `natives`, also scores every domain of a scored target against its
    native on the domain's own superposition (Pipeline.use_score_domains; the parse by the parameters of `batch_domains`, or the
    defaults): the target's scores gain the key "domain_scores" (score.domain_scores_json) wherever they are written."""
    global _SCORE_DOMAINS
    before, _SCORE_DOMAINS = _SCORE_DOMAINS, True
    try:
        yield
    finally:
        _SCORE_DOMAINS = before


def run_batch(targets, out_dir, iterations=default_iterations, minsteps=default_minsteps,
              weights_file=None, state_dict=None, streams=4, device=None, rank=0, world=1, fmt="pdb", store=None,
              converge=None, stats_out=None, distmap=False, natives=None, structures=None, library=None, search_top=10,
              score_map=False, score_passes=False, ss=False, restrain=None, restrain_cutoff=15.0, exposure=False):
    """Predict this rank's targets; returns (number done, seconds, [output paths]).
    `natives`: a directory of native structures, <stem>.pdb for the target <stem>.aln / .a3m: such a target is scored on
    the GPU (Pipeline.set_score) and its scores are written with it (write_result); a target without a file is predicted
    unscored.  `stats_out` then receives "scores": {stem: the dict of score.scores_json}.
    `score_map` (needs `natives`): a scored target's predicted distance map is scored against its native too
    (Pipeline.set_score_map); its scores gain the key "map" (score.map_scores_json) wherever they are written.
    `score_passes` (needs `natives`): every recycling pass of a scored target is scored against its native too
    (Pipeline.set_score_passes); its scores gain the key "passes" (score.pass_scores_json) wherever they are written.
    `ss`: every target's backbone gets its secondary structure assigned on the GPU (Pipeline.set_ss; with `natives`, a
    target whose native covers every column also gets the native's and Q3 / Q8) and it is written with the target
    (write_result); `stats_out` then receives "ss": {stem: the dict of score.ss_json}.
    `exposure`: every target's backbone gets its solvent exposure counted on the GPU (Pipeline.set_exposure; with `natives`, a
    target whose native covers every column also gets the native's) and it is written with the target (write_result);
    `stats_out` then receives "exposure": {stem: the dict of score.exposure_json}.
    `structures`: a directory of structures of any length and sequence, <stem>.pdb for the target <stem>.aln / .a3m: such a
    target's model is aligned with the structure's first chain on the GPU (Pipeline.set_align) and the alignment is written
    with it (write_result); a target without a file is predicted without one.  `stats_out` then receives "alignments":
    {stem: the header fields of score.alignment_json}.
    `library`: a fold library (a score.Library, a directory of PDB files or an .npz of tools/make_library.py): every
    target's model is aligned with every entry on the GPU (Pipeline.set_search) and the ranking is written with it
    (write_result); `stats_out` then receives "hits": {stem: the best `search_top` of score.hits_json, without R and t}.  A
    library with a `refine` of R is screened and only the best R entries refined (option "search_refine"); the hits then say which.
    `restrain` (force constant K, None or 0 = off) and `restrain_cutoff` (Angstrom): every target's final refinement is
    restrained to its predicted distance map (Pipeline.set_restrain, which turns the distance map on: it is written only with
    `distmap`); every target's report (predict.restrain_report) is written with it (write_result) and `stats_out` receives
    "restrain": {stem: the report}.
    `distmap`: every target's chosen-pass distance map is brought back and written too (write_result).
    `converge` (Angstrom, None = off): targets stop recycling once converged (Pipeline.set_converge); `stats_out`, a
    dict, then receives this rank's "passes_run" and "passes_saved".

    Which targets those are: with `store` (a torch.distributed key-value store shared by the ranks of the job) every
    rank takes the next most expensive target from ONE shared queue whenever it has room; without it the static
    partition of `plan_shard`.  Either way a rank reads and encodes only the targets it takes, reading / encoding,
    the GPU and the writing of finished structures overlap (targets are submitted while others run and results are
    written as they complete), and a failing target never costs the others their results."""
    if fmt not in ("pdb", "ca", "npz"):
        raise ValueError(f"unknown output format {fmt!r} (pdb, ca, npz)")
    for option, wanted in (("score_map", score_map), ("score_passes", score_passes)):
        if wanted and not natives:
            raise ValueError(needs_native(option, option, "`natives`", many=True))
    score_domains = _SCORE_DOMAINS                         # (batch_score_domains)
    if score_domains and not natives:
        raise ValueError("score_domains scores every domain against native structures: give `natives`")
    restraining = restrain_to_milli(restrain) > 0          # (a bad value raises before any work)
    restrain_cutoff_to_mA(restrain_cutoff)
    check_output_stems(targets)
    os.makedirs(out_dir, exist_ok=True)
    # sharding needs only (L, N) estimates from a header scan: a rank parses its own targets and nobody else's
    order, scans = cost_order(targets, iterations)
    if store is not None and world > 1:
        digest = hashlib.sha1("\n".join(f"{a}\t{t}" for a, t in targets).encode()).hexdigest()[:16]
        queue = _SharedQueue(order, store, f"{digest}.{iterations}.{minsteps}")
        mine_scans = scans                              # any target may come this way
    else:
        owned = plan_shard(targets, iterations, rank, world)
        queue = _StaticQueue(owned)
        mine_scans = [scans[i] for i in owned]
    if not mine_scans:
        return 0, 0.0, []
    # capacity of the engines from the scans (L and N are exact: scan_target counts the rows on the raw bytes)
    any_a3m = any(a.endswith(".a3m") for a, _ in targets)
    max_L = max(8, max(L for L, _ in mine_scans))
    max_N = MAX_SEQS if any_a3m else max(1, min(MAX_SEQS, max(N for _, N in mine_scans)))
    struct_ca = {}                                      # stem -> C-alpha trace of the structure to align with
    if structures:
        from .predict import MAX_L
        for a, _ in targets:
            stem = os.path.splitext(os.path.basename(a))[0]
            path = os.path.join(structures, stem + ".pdb")
            if os.path.exists(path):
                ca = _score.read_native_ca(path)[0]
                if 3 <= ca.shape[0] <= MAX_L:
                    struct_ca[stem] = ca
                else:
                    print(f"dmpfold-batch: {path}: {ca.shape[0]} C-alpha atoms, outside [3, {MAX_L}]: {stem} is predicted "
                          "without an alignment", file=sys.stderr)
        # the engines hold both traces: their capacity covers the longest structure too
        max_L = max([max_L] + [ca.shape[0] for ca in struct_ca.values()])
    if isinstance(library, (str, os.PathLike)):
        library = _score.Library.open(library)
    if library is not None:
        from .predict import MAX_L
        library.check(MAX_L)
        max_L = max(max_L, library.max_m)               # the engines' capacity bounds every entry's length
    domains = _DOMAINS                                  # (batch_domains)
    flex = _FLEX                                        # (batch_flex)
    msa_report = _MSA_REPORT                            # (batch_msa_report)
    search_domains = library is not None and bool(getattr(library, "domains", False))      # (--search-domains)
    if (search_domains or score_domains) and domains is None:
        domains = domains_options()                     # the library's flag, or --score-domains, turns "domains" on, with the defaults
        domains = (domains[0] * 1e-3,) + domains[1:]
    t0 = time.perf_counter()
    pipe, dev, copy_stream = None, None, None
    failed, outputs, parsed, faulted = [], [], {}, []
    n_taken = 0

    def ensure_pipe():
        nonlocal pipe, dev, copy_stream
        if pipe is None:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            sd = state_dict if state_dict is not None else load_state_dict(weights_file)
            pipe = Pipeline(dev, max_L, max_N, sd, streams=streams, precision=drop_in_precision())
            # (score_map and the restraint turn the distance map on: it is written only with `distmap`)
            if domains is not None:
                pipe.use_domains(True, *domains)            # (in front of set_search: a library with `domains` keeps these parameters)
            for setter, wanted, *value in (("converge", converge is not None, converge), ("distmap", distmap, True),
                                           ("score", natives, True), ("score_map", score_map, True),
                                           ("score_passes", score_passes, True), ("ss", ss, True), ("exposure", exposure, True),
                                           ("restrain", restraining, restrain, restrain_cutoff), ("align", structures, True),
                                           ("search", library is not None, library)):
                if wanted:
                    getattr(pipe, "set_" + setter)(*value)
            if score_domains:
                pipe.use_score_domains(True)                # (behind set_score, which it needs)
            if flex is not None:
                pipe.use_flex(True, flex)
            if msa_report is not None:
                pipe.use_msa_report(True, msa_report)
            if dev.type == "cuda":
                # every copy of this front end goes through its own (non-blocking) stream: nothing is ever enqueued on
                # the process's default stream while the engines run
                copy_stream = torch.cuda.Stream(device=dev)
        return pipe

    done = []                                           # completed on the GPU AND copied to the host, not yet written
    copying = []                                        # (ticket, (host coords, host confs[, map, info][, block]), event): D2H in flight

    # The scheduler's thread never blocks on the GPU: a synchronous copy on the default stream can queue behind an
    # engine's kernels (streams share hardware queues) and would stall the thread - and with it every engine.
    # Alignments go up from pinned memory and results come back into pinned memory, both asynchronously on the front
    # end's own stream; completion is polled.  (Measured at the north-star size: files -> PDB files 6.2 structures/s
    # including the pipeline's set-up against 6.7 for the same targets resident in HBM, tools/batch_throughput.py.)
    def start_copy_back(t):
        outs = pipe.peek(t)                           # (coords, confs), with `distmap` also (map, info)
        if search_domains:
            outs = outs + (pipe.outputs_of(t).domain_search_block,)      # which `peek` never hands out: last of all
        if score_domains:
            outs = outs + (pipe.outputs_of(t).domain_score_block,)       # likewise, behind that
        if flex is not None:
            outs = outs + (pipe.outputs_of(t).flex_block,)               # likewise, behind that
        if msa_report is not None:
            outs = outs + (pipe.outputs_of(t).msa_report_block,)         # likewise, behind that
        if outs[0].is_cuda:
            host = tuple(torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in outs)
            with (torch.cuda.stream(copy_stream) if copy_stream is not None else contextlib.nullcontext()):
                for h, x in zip(host, outs):
                    h.copy_(x, non_blocking=True)     # the prediction has completed (polled): no ordering needed
                ev = torch.cuda.Event()
                ev.record()
        else:
            host, ev = tuple(outs), None
        copying.append((t, host, ev))

    def reap_copies():
        while copying and (copying[0][2] is None or copying[0][2].query()):
            done.append(copying.pop(0)[:2])

    scored, aligned = set(), set()                      # the tickets that had a native / a structure
    asked = {"natives": bool(natives), "structures": bool(structures), "library": library is not None, "ss": ss,
             "exposure": exposure, "restrain": restraining, "domains": domains is not None, "search_domains": search_domains,
             "flex": flex is not None, "msa_report": msa_report is not None}
    blocks_on = {"score": asked["natives"], "align": asked["structures"], "search": asked["library"], "score_map": score_map,
                 "passes": score_passes, "ss": ss, "exposure": exposure, "domains": domains is not None}
    gathered = {}                                       # {key of `stats_out`: {stem: what the summary takes}}

    def write(t, public):
        """a finished target's files from what the pipeline handed out; its scores only if it had a native"""
        ds_block, score_block, flex_block, msa_block = None, None, None, None
        if msa_report is not None:
            public, msa_block = public[:-1], public[-1]
        if flex is not None:
            public, flex_block = public[:-1], public[-1]
        if score_domains:
            public, score_block = public[:-1], public[-1]
        if search_domains:
            public, ds_block = public[:-1], public[-1]
        out = Outputs.of(public, distmap=distmap or score_map or restraining, **blocks_on)
        aln_path, alnmat, _ = parsed.pop(t)
        stem = os.path.splitext(os.path.basename(aln_path))[0]
        had = {"score": t in scored, "score_map": t in scored, "passes": t in scored, "align": t in aligned}
        results = {row.name: row.unpack(getattr(out, row.field), alnmat.shape[1], library=library, seq=alnmat[0],
                                        coords=out.coords, confs=out.confs)
                   for row in _score.BLOCKS if getattr(out, row.field) is not None and had.get(row.key, True)}
        forms = results_json(results, search_top)
        if ds_block is not None:
            ds = dict(_score.unpack_domain_search(ds_block, alnmat.shape[1], len(library), library.refine), names=list(library.names))
            if "refined" in ds:
                ds["refine"] = library.refine
            results["domain_hits"] = ds
            forms["domain_hits"] = domain_hits_form(ds, results.get("domains"), search_top)
        if score_block is not None and t in scored and "scores" in forms:
            results["domain_scores"] = _score.unpack_domain_scores(score_block, alnmat.shape[1])
            forms["scores"]["domain_scores"] = _score.domain_scores_json(results["domain_scores"], results.get("domains"))
        if flex_block is not None:
            results["flex"] = _score.unpack_flex(flex_block, alnmat.shape[1], confs=out.confs, domains=results.get("domains"))
            forms["flex"] = _score.flex_json(results["flex"])
        if msa_block is not None:
            results["msa_report"] = _score.unpack_msa_report(msa_block, alnmat.shape[1], confs=out.confs,
                                                             seq="".join(_score.AA1[c] if c < 20 else "-" for c in alnmat[0]))
            forms["msa_report"] = _score.msa_report_json(results["msa_report"])
        rep = None
        if restraining:
            rep = forms["restrain"] = restrain_report(float(restrain), float(restrain_cutoff), max(minsteps, 0), out.distmap,
                                                      float(out.info[2]), out.coords)
        for name, form in forms.items():
            key, brief = GATHERED_AS.get(name, (name, None))
            gathered.setdefault(key, {})[stem] = form if brief is None else brief(form)
        outputs.append(write_result(out_dir, aln_path, out.coords, out.confs, alnmat, fmt, out.distmap if distmap else None,
                                    out.info if distmap else None, hits_top=search_top, restrain=rep, **results))

    def finish(item):
        t, public = item
        if bool(torch.isnan(public[1][:1]).any()):      # a device-side fault poisoned it: repeated alone at the end
            parsed[t] = parsed[t][:2] + (None,)
            faulted.append(t)
            return
        pipe.result(t)
        write(t, public)

    exhausted = False
    cap = 2 * max(1, int(streams))                      # started + queued per rank
    backlog_cap = max(1, int(streams))                  # queued, not yet started

    def take_one():
        """Read, encode and submit the next target of the queue; False when the queue is empty."""
        nonlocal exhausted, n_taken
        i = queue.take()
        if i is None:
            exhausted = True
            return False
        n_taken += 1
        aln_path, tpl_path = targets[i]
        try:
            rows = read_a3m(aln_path) if aln_path.endswith(".a3m") else read_aln(aln_path)
            tpl = read_template_ca(tpl_path) if tpl_path else None
            alnmat = encode_aln(rows)
            nat = None
            if natives:
                nat_path = os.path.join(natives, os.path.splitext(os.path.basename(aln_path))[0] + ".pdb")
                if os.path.exists(nat_path):
                    nat = _score.native_from_pdb(rows[0], nat_path)
            p = ensure_pipe()
            h_msa = torch.from_numpy(np.ascontiguousarray(alnmat))
            with (torch.cuda.stream(copy_stream) if copy_stream is not None else contextlib.nullcontext()):
                if dev.type == "cuda":
                    h_msa = h_msa.pin_memory()
                    d_msa = h_msa.to(dev, non_blocking=True)
                else:
                    d_msa = h_msa
                # the pinned source stays alive in `parsed` until the target is written; the engine that takes the
                # target orders its stream behind the stream that is current at submission (the copy stream)
                strc = struct_ca.get(os.path.splitext(os.path.basename(aln_path))[0])
                t = p.submit(d_msa, iterations, minsteps, template_ca=tpl, **({"native": nat} if nat is not None else {}),
                             **({"structure": strc} if strc is not None else {}))
                parsed[t] = (aln_path, alnmat, h_msa)
                if nat is not None:
                    scored.add(t)
                if strc is not None:
                    aligned.add(t)
        except (IndexError, ValueError, OSError, UnicodeDecodeError, RuntimeError) as exc:
            # unknown residue letter / ragged rows / unreadable file / larger than the scan said: this target only
            failed.append((aln_path, exc))
        return True

    def room():
        return (not exhausted and (pipe is None or pipe.backlog() < backlog_cap)
                and len(parsed) - len(faulted) - len(done) - len(copying) < cap)

    # Host work - reading / encoding / uploading the next alignment, bringing a finished structure back, formatting
    # and writing it - is done ONE item per scheduling round in which nothing could be issued (the GPU has work
    # queued), never while units are waiting to be issued: the targets of a group finish and start together, and
    # 4 x (0.6 + 1.5) ms of host work in front of the next group's first launches is GPU idle time.
    while True:
        if pipe is None or not pipe.busy():
            # nothing left to issue: refill from the queue, else write what has completed, else wait for the GPU
            while room():
                if not take_one():
                    break
            if pipe is None or not pipe.busy():
                if pipe is not None:
                    for t in pipe.poll():
                        start_copy_back(t)
                    reap_copies()
                if done:
                    finish(done.pop(0))
                    continue
                if len(parsed) > len(faulted):          # issued to the end, not yet completed on the GPU
                    time.sleep(0.0002)
                    continue
                if exhausted or not room():
                    break
                continue
        progressed = pipe.step()
        if not progressed:
            for t in pipe.poll():
                start_copy_back(t)
            reap_copies()
            if room():
                take_one()
            elif done:
                finish(done.pop(0))
    if copying:
        if copying[-1][2] is not None:
            copying[-1][2].synchronize()
        reap_copies()
    for item in done:
        finish(item)
    if faulted:
        res = pipe.collect(faulted)
        for t in faulted:
            if isinstance(res[t], Exception):
                failed.append((parsed.pop(t)[0], res[t]))
            else:
                write(t, res[t] + ((pipe.collected[t].domain_search_block,) if search_domains else ())
                      + ((pipe.collected[t].domain_score_block,) if score_domains else ())
                      + ((pipe.collected[t].flex_block,) if flex is not None else ())
                      + ((pipe.collected[t].msa_report_block,) if msa_report is not None else ()))
    elapsed = time.perf_counter() - t0
    if pipe is not None:
        if stats_out is not None and converge is not None:
            st = pipe.stats()
            stats_out["passes_run"], stats_out["passes_saved"] = st["passes_run"], st["passes_saved"]
        for key, argument, _ in GATHERED:
            if stats_out is not None and asked[argument]:
                stats_out[key] = gathered.get(key, {})
        pipe.close()
    if failed:
        raise BatchFailures(failed, len(outputs), elapsed, outputs)
    return n_taken, elapsed, outputs


def batch_parser():
    ap = argparse.ArgumentParser(description="DMPfold2 batch prediction on AMD MI355X (one process per GPU)")
    ap.add_argument("-l", "--list", default=None, help="text file: one alignment path (+ optional template) per line")
    ap.add_argument("-i", "--input", nargs="*", default=[],
                    help="alignment files (.aln / .a3m) and directories of them")
    ap.add_argument("-o", "--out_dir", required=True)
    ap.add_argument("--format", choices=("pdb", "ca", "npz"), default="pdb",
                    help="pdb: the single-target CLI's text; ca: its CA records only; npz: arrays")
    ap.add_argument("-n", "--iterations", type=int, default=default_iterations)
    ap.add_argument("-m", "--minsteps", type=int, default=default_minsteps)
    ap.add_argument("-w", "--model_weights", type=str, default=None)
    ap.add_argument("--streams", type=int, default=4, help="targets in flight per GPU")
    ap.add_argument("--static-shards", action="store_true",
                    help="several ranks: fixed partition by estimated cost instead of the shared work queue")
    ap.add_argument("--converge", type=_tolerance_arg, default=None, metavar="TOL",
                    help="stop a target's recycling once a pass changes its seed distance map by no more than TOL Angstrom "
                         "(RMS); the summary then counts the passes run and saved")
    ap.add_argument("--distmap", action="store_true",
                    help="also write every target's predicted C-alpha distance map (the pass the best-of rule chose): npz "
                         "gains the arrays distmap, best_pass, passes_run and map_rms; pdb / ca write <stem>.distmap.npy")
    ap.add_argument("--natives", default=None, metavar="DIR",
                    help="directory of native structures, <stem>.pdb per target: such targets are scored on the GPU (TM-score, "
                         "GDT, RMSD, lDDT-CA); the summary gains the per-target scores, their means and medians; npz gains the "
                         "arrays, pdb / ca write <stem>.scores.json; a target without a file is predicted unscored")
    ap.add_argument("--score-map", action="store_true",
                    help="with --natives: also score every such target's predicted distance map against its native on the GPU "
                         "(contact precision of the top L, L/2, L/5 per separation class, lDDT and distance error of the map); "
                         "the summary's scores gain the key \"map\" with means and medians of its figures, npz gains the map_* "
                         "arrays, <stem>.scores.json gains \"map\"")
    ap.add_argument("--score-passes", action="store_true",
                    help="with --natives: score every recycling pass of every such target against its native on the GPU (per "
                         "pass: mean confidence logit, convergence delta, TM-score, GDT, RMSD, lDDT-CA); the summary's scores "
                         "gain the key \"passes\" and the summary the share of targets whose chosen pass was the best one, the "
                         "regrets, the mean TM-score by pass and what each convergence tolerance would have cost; npz gains the "
                         "pass_* arrays, <stem>.scores.json gains \"passes\"")
    ap.add_argument("--structures", default=None, metavar="DIR",
                    help="directory of structures of any length and sequence, <stem>.pdb per target: such a target's model is "
                         "aligned with the structure's first chain on the GPU (structural alignment, TM-scores by both lengths); "
                         "the summary gains each target's header fields; npz gains the arrays, pdb / ca write "
                         "<stem>.alignment.json; a target without a file is predicted without an alignment")
    ap.add_argument("--library", default=None, metavar="DIR|FILE.npz",
                    help="fold library (a directory of PDB files or an .npz of tools/make_library.py): every target's model is "
                         "aligned with every entry on the GPU and the entries are ranked by TM-score; the summary gains each "
                         "target's top hits; npz gains hit_rank, hit_tm_model, hit_tm_struct and hit_names, pdb / ca write "
                         "<stem>.hits.json")
    ap.add_argument("--search-top", type=int, default=10, metavar="N", help="hits per target to report with --library (default 10)")
    # --search-refine R (with --library): screen every entry by its best gapless threading and refine only the best R by that;
    # the hits gain "refined", npz gains hit_refined.  The help text and the parsed namespace of the other flags are recorded
    # (tests/golden/host_plumbing.json.gz): the flag stays out of both unless given, and README.md describes it.
    ap.add_argument("--search-refine", type=int, default=argparse.SUPPRESS, metavar="R", help=argparse.SUPPRESS)
    # --search-domains (with --library): search the library with every domain of every target's model as well (the parse by the
    # parameters of --domains, or the defaults); npz gains dom_hit_rank and dom_hit_tm, pdb / ca write <stem>.domain_hits.json,
    # the summary carries every target's best hit per domain.  Hidden like --search-refine, for the same reason.
    ap.add_argument("--search-domains", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    # --score-domains (with --natives): score every domain of a scored target's model - and of its native, where that is whole -
    # against the native on the domain's own superposition (the parse by the parameters of --domains, or the defaults);
    # <stem>.scores.json gains the key "domain_scores", npz gains dom_score_table and dom_score_res, the summary carries per target
    # the domain count, tm_domains and lddt_inter with their means and medians.  Hidden like --search-refine, for the same reason.
    ap.add_argument("--score-domains", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    # --domains [--domains-tau Q --domains-min-size N --domains-min-segment N]: split every target's model into structural domains
    # on the GPU; the summary gains every target's domain count with mean, median and the share of multi-domain targets, npz
    # gains dom_label and dom_table, pdb / ca write <stem>.domains.json.  Hidden like --search-refine, for the same reason.
    ap.add_argument("--domains", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    ap.add_argument("--domains-tau", type=float, default=argparse.SUPPRESS, metavar="Q", help=argparse.SUPPRESS)
    ap.add_argument("--domains-min-size", type=int, default=argparse.SUPPRESS, metavar="N", help=argparse.SUPPRESS)
    ap.add_argument("--domains-min-segment", type=int, default=argparse.SUPPRESS, metavar="N", help=argparse.SUPPRESS)
    # --flex [--flex-cutoff A]: the Gaussian network model of every target's C-alpha trace on the GPU (contacts within A Angstrom,
    # 7.3 by default); the summary carries per target lambda_1, components, the hinge count and the correlation of msf with
    # 1 - confidence, with means and medians; npz gains flex_eig, flex_modes, flex_msf and flex_degree, pdb / ca write
    # <stem>.flex.json.  Hidden like --search-refine, for the same reason.
    ap.add_argument("--flex", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    ap.add_argument("--flex-cutoff", type=float, default=argparse.SUPPRESS, metavar="A", help=argparse.SUPPRESS)
    # --msa-report [--dca-map]: a report on every target's alignment made on the GPU (Neff at 62, 80 and 90 % identity, gaps, copies,
    # histograms, per-column conservation, the strongest DCA coupling per column; with --natives the DCA contact precisions); the
    # summary carries per target N, neff_80 and the median coverage, with means and medians, and with --natives Spearman's
    # correlation of log10 neff_80 with the TM-score and the mean TM-score per Neff bin; npz gains msa_header, msa_columns and (--dca-map,
    # which implies --msa-report) dca_map, pdb / ca write <stem>.msa.json and <stem>.dca_map.npy.  Hidden like --search-refine, for the same reason.
    ap.add_argument("--msa-report", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    ap.add_argument("--dca-map", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)
    ap.add_argument("--ss", action="store_true",
                    help="assign secondary structure to every target's backbone on the GPU from its hydrogen bonds; the summary "
                         "gains every target's eight-state string and helix / strand / coil fractions with their means and "
                         "medians (with --natives also mean Q3 / Q8 over the targets whose native covers every column); npz "
                         "gains ss8, ss_bp and the energy arrays, pdb / ca write <stem>.ss.json")
    ap.add_argument("--exposure", action="store_true",
                    help="count the solvent exposure of every target's backbone on the GPU (a Shrake-Rupley surface of N, CA, C, O "
                         "and CB, half-sphere exposure and CB contact number per residue); the summary gains every target's total "
                         "area, burial ratio and mean counts with their means and medians; npz gains exp_n, exp_hse_up, "
                         "exp_hse_down, exp_cn10 and exp_area, pdb / ca write <stem>.exposure.json")
    add_restrain_arguments(ap)
    return ap


CONVERGE_SWEEP = (0.05, 0.1, 0.2, 0.5, 1.0)          # Angstrom: the tolerances the summary of --score-passes tries


def pass_summary(tables, tolerances=CONVERGE_SWEEP):
    """{stem: the dict of score.pass_scores_json} of full-depth runs -> the summary's part for --score-passes, over the
    targets whose table holds a pass and a TM-score: how often the pass the confidence picked was the best by TM-score, mean
    and median of the regrets, the mean TM-score by pass index (each over the targets that ran that pass), and the
    convergence sweep - per tolerance the mean passes score.simulate_converge says a `--converge` run would have run and
    the mean TM-score lost against the full-depth choice (tm of the pass kept at full depth minus tm of the pass kept by
    the stop, both from the table)."""
    tabs = [_score.pass_scores_from_json(t) for t in tables.values()]
    tabs = [t for t in tabs if t["rows"] > 0 and t["tm_pass"] is not None]
    out = {"pass_scored_targets": len(tabs)}
    if not tabs:
        return out
    out["best_is_tm_pass"] = float(np.mean([t["best_pass"] == t["tm_pass"] for t in tabs]))
    for name in ("regret_tm", "regret_lddt"):
        vals = [t[name] for t in tabs if t[name] == t[name]]
        out["mean_" + name] = float(np.mean(vals)) if vals else None
        out["median_" + name] = float(np.median(vals)) if vals else None
    depth = max(t["rows"] for t in tabs)
    by_pass = [[float(t["tm"][p]) for t in tabs if p < t["rows"] and t["tm"][p] == t["tm"][p]] for p in range(depth)]
    out["mean_tm_by_pass"] = [float(np.mean(v)) if v else None for v in by_pass]
    sweep = []
    for tol in tolerances:
        runs, lost = [], []
        for t in tabs:
            full = _score.simulate_converge(t["conf_mean"], t["delta"], None)
            run, best = _score.simulate_converge(t["conf_mean"], t["delta"], tol)
            runs.append(run)
            lost.append(float(t["tm"][full[1]]) - float(t["tm"][best]))
        sweep.append({"tol": tol, "mean_passes": float(np.mean(runs)), "mean_tm_lost": float(np.mean(lost))})
    out["converge_sweep"] = sweep
    return out


def ss_summary(ss):
    """{stem: the dict of score.ss_json} -> the summary's part for --ss: per target the eight-state string and the three
    fractions (and q3, q8 where it had a whole native), mean and median of the fractions, mean Q3 / Q8 over the targets that
    have them."""
    out = {"ss_targets": len(ss), "ss": {stem: {k: v[k] for k in ("ss8", "helix", "strand", "coil", "q3", "q8") if k in v}
                                         for stem, v in ss.items()}}
    for name in ("helix", "strand", "coil"):
        vals = [v[name] for v in ss.values()]
        out["mean_" + name] = float(np.mean(vals)) if vals else None
        out["median_" + name] = float(np.median(vals)) if vals else None
    for name in ("q3", "q8"):
        vals = [v[name] for v in ss.values() if v.get(name) is not None]
        if vals:
            out["mean_" + name] = float(np.mean(vals))
    return out


EXPOSURE_SUMMARY = ("area", "mean_hse_up", "mean_hse_down", "mean_cn10", "mean_cb_exposed", "cb_hydrophobic", "cb_other", "burial_ratio")


def exposure_summary(exposure):
    """{stem: the dict of score.exposure_json} -> the summary's part for --exposure: per target the total area, the means of
    the three per-residue counts and of cb_exposed, the burial figures (and the three correlations where it had a whole native),
    and mean and median of each over the targets that have it."""
    keys = EXPOSURE_SUMMARY + ("r_area", "r_hse_up", "r_cn10")
    out = {"exposure_targets": len(exposure), "exposure": {stem: {k: v[k] for k in keys if k in v} for stem, v in exposure.items()}}
    for name in keys:
        vals = [v[name] for v in exposure.values() if v.get(name) is not None]
        if vals or name in EXPOSURE_SUMMARY:
            out["mean_exposure_" + name] = float(np.mean(vals)) if vals else None
            out["median_exposure_" + name] = float(np.median(vals)) if vals else None
    return out


def domains_summary(domains):
    """{stem: the dict of score.domains_json} -> the summary's part for --domains: per target the number of domains, of
    discontinuous ones and the sizes; mean and median of the domain count and the share of targets with more than one domain."""
    counts = [v["domains"] for v in domains.values()]
    return {"domain_targets": len(domains),
            "domains": {stem: {"domains": v["domains"], "discontinuous": v["discontinuous"], "sizes": [row["size"] for row in v["table"]]}
                        for stem, v in domains.items()},
            "mean_domains": float(np.mean(counts)) if counts else None,
            "median_domains": float(np.median(counts)) if counts else None,
            "multi_domain_share": float(np.mean([c > 1 for c in counts])) if counts else None}


def flex_brief(form):
    """The summary's figures of one target from its "flex" (score.flex_json): the first non-zero eigenvalue, the components, the
    hinge count and the correlation of msf with 1 - confidence, of the model's leg."""
    k = form["first_mode"]
    return {"lambda_1": None if k is None else form["eigenvalues"][k], "components": form["components"], "hinges": len(form["hinges"]),
            "r_conf": form.get("r_conf")}


def flex_summary(flex):
    """{stem: flex_brief} -> the summary's part for --flex: every target's figures, and mean and median of each over the targets
    that have it."""
    out = {"flex_targets": len(flex), "flex": flex}
    for name in ("lambda_1", "components", "hinges", "r_conf"):
        vals = [v[name] for v in flex.values() if v.get(name) is not None]
        out["mean_flex_" + name] = float(np.mean(vals)) if vals else None
        out["median_flex_" + name] = float(np.median(vals)) if vals else None
    return out


def msa_brief(form):
    """The summary's figures of one target from its "msa" (score.msa_report_json): the depth, Neff at 80 % and the median coverage."""
    return {k: form[k] for k in ("N", "neff_80", "median_coverage")}


def msa_summary(found):
    """{stem: msa_brief} -> the summary's part for --msa-report: every target's figures, and mean and median of each."""
    out = {"msa_targets": len(found), "msa": found}
    for name in ("N", "neff_80", "median_coverage"):
        vals = [v[name] for v in found.values() if v.get(name) is not None]
        out["mean_msa_" + name] = float(np.mean(vals)) if vals else None
        out["median_msa_" + name] = float(np.median(vals)) if vals else None
    return out


NEFF_BINS = (("<10", 0.0, 10.0), ("10-100", 10.0, 100.0), ("100-1000", 100.0, 1000.0), (">=1000", 1000.0, float("inf")))


def neff_tm_summary(msa, scores):
    """{stem: msa_brief} and {stem: scores} -> the summary's part for --msa-report with --natives, over the targets that have both
    a Neff above 0 and a TM-score: Spearman's correlation of log10 neff_80 with tm (None below two targets or without any
    spread), and per Neff bin the targets and their mean tm."""
    both = [(msa[s]["neff_80"], scores[s]["tm"]) for s in sorted(msa) if s in scores and scores[s].get("tm") is not None
            and msa[s].get("neff_80") is not None and msa[s]["neff_80"] > 0]
    rho = _score._spearman(np.log10([n for n, _ in both]), [t for _, t in both]) if len(both) >= 2 else float("nan")
    bins = {}
    for name, lo, hi in NEFF_BINS:
        tms = [t for n, t in both if lo <= n < hi]
        bins[name] = {"targets": len(tms), "mean_tm": float(np.mean(tms)) if tms else None}
    return {"neff_tm_targets": len(both), "neff_tm_spearman": rho if rho == rho else None, "neff_tm_bins": bins}


def restrain_summary(reports):
    """{stem: the dict of predict.restrain_report} -> the summary's part for --restrain: every target's report, and mean and
    median of map_rms, restrained_pairs, clashes and bond_dev_max."""
    out = {"restrained_targets": len(reports), "restrain": reports}
    for name in ("map_rms", "restrained_pairs", "clashes", "bond_dev_max"):
        vals = [r[name] for r in reports.values() if r.get(name) is not None]
        out["mean_" + name] = float(np.mean(vals)) if vals else None
        out["median_" + name] = float(np.median(vals)) if vals else None
    return out


def domain_scores_brief(form):
    """The summary's figures of one target from its "domain_scores" (score.domain_scores_json): the domain count, tm_domains and
    lddt_inter of the native's leg - of the model's leg where the native has none - and which leg that is."""
    leg = "native" if "native" in form else "model"
    if leg not in form:
        return {"leg": None, "domains": 0, "tm_domains": None, "lddt_inter": None}
    return {"leg": leg, "domains": len(form[leg]["rows"]), "tm_domains": form[leg]["tm_domains"], "lddt_inter": form[leg]["lddt_inter"]}


def score_summary(scores):
    """{stem: scores} -> the summary's part: the per-target scores, and mean and median of each score over the targets
    that have it."""
    out = {"scored_targets": len(scores), "scores": scores}
    for name in ("tm", "gdt_ts", "gdt_ha", "rmsd", "lddt"):
        vals = [s[name] for s in scores.values() if s.get(name) is not None]
        out["mean_" + name] = float(np.mean(vals)) if vals else None
        out["median_" + name] = float(np.median(vals)) if vals else None
    flat = {stem: _score.map_scores_flat(s["map"]) for stem, s in scores.items() if s.get("map") is not None}
    if flat:                                         # --score-map: the map's figures the same way
        out["map_scored_targets"] = len(flat)
        for name in next(iter(flat.values())):
            vals = [f[name] for f in flat.values() if f.get(name) is not None]
            out["mean_" + name] = float(np.mean(vals)) if vals else None
            out["median_" + name] = float(np.median(vals)) if vals else None
    per_domain = {stem: domain_scores_brief(s["domain_scores"]) for stem, s in scores.items() if s.get("domain_scores") is not None}
    if per_domain:                                   # --score-domains: per target D, tm_domains and lddt_inter
        out["domain_scored_targets"], out["domain_scores"] = len(per_domain), per_domain
        for name in ("domains", "tm_domains", "lddt_inter"):
            vals = [b[name] for b in per_domain.values() if b.get(name) is not None]
            out["mean_domain_" + name] = float(np.mean(vals)) if vals else None
            out["median_domain_" + name] = float(np.median(vals)) if vals else None
    tables = {stem: s["passes"] for stem, s in scores.items() if s.get("passes") is not None}
    if tables:                                       # --score-passes: the pass tables' aggregates
        out.update(pass_summary(tables))
    return out


# What a job gathers per target for its summary: (the key in run_batch's `stats_out`, in the job's store and in the summary;
# the argument that asks for it; the summary's part from {stem: what was gathered}).  GATHERED_AS: a result (by the `name` of its
# row of score.BLOCKS) that is gathered under another key, in a briefer form than its JSON form.
GATHERED = (("scores", "natives", score_summary),
            ("alignments", "structures", lambda found: {"aligned_targets": len(found), "alignments": found}),
            ("hits", "library", lambda found: {"searched_targets": len(found), "hits": found}),
            ("ss", "ss", ss_summary), ("exposure", "exposure", exposure_summary), ("restrain", "restrain", restrain_summary),
            ("domains", "domains", domains_summary), ("flex", "flex", flex_summary),
            ("msa", "msa_report", msa_summary),
            ("domain_hits", "search_domains", lambda found: {"domain_searched_targets": len(found), "domain_hits": found}))
GATHERED_AS = {"flex": ("flex", flex_brief), "msa_report": ("msa", msa_brief),
               "alignment": ("alignments", lambda form: {k: form[k] for k in ("m",) + _score.ALIGN_NAMES}),
               "hits": ("hits", lambda form: [{k: v for k, v in hit.items() if k not in ("R", "t")} for hit in form["hits"]]),
               # every domain's best hit
               "domain_hits": ("domain_hits", lambda form: [dict({k: d[k] for k in ("domain", "size") if k in d},
                                                                 **({k: v for k, v in d["hits"][0].items() if k not in ("R", "t")}
                                                                    if d["hits"] else {})) for d in form["domains"]])}


def gather(key, mine, world, job_store):
    """{stem: value} of one GATHERED key over the ranks of a job, sorted: this rank's and what ranks 1 .. world - 1 left in
    the job's store."""
    found = dict(mine.get(key, {}))
    for r in range(1, world):
        found.update(json.loads(job_store.get(f"dmpfold_batch_{key}/{r}").decode()))
    return dict(sorted(found.items()))


def main(argv=None):
    ap = batch_parser()
    args = ap.parse_args(argv)
    if not args.list and not args.input:
        ap.error("give -l targets.txt and / or -i alignments ...")
    for option in NATIVE_NEEDED:
        if getattr(args, option) and not args.natives:
            ap.error(needs_native(option, "--" + option.replace("_", "-"), "--natives DIR", many=True))

    library = args.library
    if hasattr(args, "search_refine"):
        if not args.library:
            ap.error("--search-refine needs --library")
        if not 0 <= args.search_refine <= _score.SEARCH_MAX:
            ap.error(f"--search-refine must be 0 or 1 .. {_score.SEARCH_MAX}, got {args.search_refine}")
        library = _score.Library.open(args.library, refine=args.search_refine)
    if hasattr(args, "search_domains"):
        if not args.library:
            ap.error("--search-domains needs --library")
        library = library if isinstance(library, _score.Library) else _score.Library.open(args.library)
        library.domains = True
    if hasattr(args, "score_domains") and not args.natives:
        ap.error("--score-domains needs --natives")

    if hasattr(args, "dca_map"):
        args.msa_report = True                           # (--dca-map implies --msa-report)
    dom_given = {k: getattr(args, "domains_" + k) for k in ("tau", "min_size", "min_segment") if hasattr(args, "domains_" + k)}
    if dom_given and not hasattr(args, "domains"):
        ap.error("--domains-tau, --domains-min-size and --domains-min-segment need --domains")
    try:
        domains_options(**dom_given)                     # (a bad value is an error of the command line)
        if hasattr(args, "flex_cutoff"):
            if not hasattr(args, "flex"):
                ap.error("--flex-cutoff needs --flex")
            _score.flex_cut_mA(args.flex_cutoff)
    except ValueError as exc:
        ap.error(str(exc))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        job_store = shard.job_store(rank, world)
        dist.init_process_group("nccl", store=job_store, rank=rank, world_size=world,
                                device_id=torch.device("cuda", local_rank))
    if world > 1:
        shard.pin_rank_to_cores(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    targets = (read_target_list(args.list) if args.list else []) + expand_inputs(args.input)
    status, n_failed, broke = 0, 0, 0
    store = job_store if (world > 1 and not args.static_shards) else None
    passes = {}
    try:
        with (batch_domains(**dom_given) if hasattr(args, "domains") else contextlib.nullcontext()), \
                (batch_score_domains() if hasattr(args, "score_domains") else contextlib.nullcontext()), \
                (batch_flex(getattr(args, "flex_cutoff", 7.3)) if hasattr(args, "flex") else contextlib.nullcontext()), \
                (batch_msa_report(hasattr(args, "dca_map")) if hasattr(args, "msa_report") else contextlib.nullcontext()):
            n, elapsed, _ = run_batch(targets, args.out_dir, args.iterations, args.minsteps,
                                      weights_file=args.model_weights, streams=args.streams,
                                      device=f"cuda:{local_rank}", rank=rank, world=world, fmt=args.format, store=store,
                                      converge=args.converge, stats_out=passes, distmap=args.distmap, natives=args.natives,
                                      structures=args.structures, library=library, search_top=args.search_top,
                                      score_map=args.score_map, score_passes=args.score_passes, ss=args.ss,
                                      restrain=args.restrain, restrain_cutoff=args.restrain_cutoff, exposure=args.exposure)
    except BatchFailures as bf:                      # keep going: the other ranks wait in job_summary
        for aln_path, exc in bf.failed:
            print(f"dmpfold-batch: {aln_path}: {type(exc).__name__}: {exc}", file=sys.stderr)
        n, elapsed, status, n_failed = bf.n_done, bf.elapsed, 1, len(bf.failed)
    except Exception as exc:                         # noqa: BLE001 - whatever went wrong on THIS rank, the others are
        # waiting in job_summary's reduction: report, take part in it, and fail the job through the exit status.  What
        # this rank had already taken from the shared queue is lost with it: the summary says so
        print(f"dmpfold-batch: rank {rank}: {type(exc).__name__}: {exc}", file=sys.stderr)
        n, elapsed, status, broke = 0, 0.0, 2, 1
    for key, argument, _ in GATHERED:                # host side, through the job's key-value store: read behind the reduction
        if getattr(args, argument, None) and world > 1:
            job_store.set(f"dmpfold_batch_{key}/{rank}", json.dumps(passes.get(key, {})))
    total, tmax, failed_all, broke_all = shard.job_summary(n, elapsed, failures=(n_failed, broke))
    if args.converge is not None:
        passes_all = shard.sum_over_ranks([passes.get("passes_run", 0), passes.get("passes_saved", 0)])
    if rank == 0:
        summary = {"targets": total, "seconds": tmax, "structures_per_s": total / tmax if tmax > 0 else 0.0,
                   "n_gpus": world, "failed_targets": failed_all, "failed_ranks": broke_all}
        if broke_all:
            summary["note"] = ("%d rank(s) broke down: the targets they had taken are missing from the output directory - "
                               "compare it with the target list" % broke_all)
        if args.converge is not None:
            summary["converge"], summary["passes_run"], summary["passes_saved"] = args.converge, passes_all[0], passes_all[1]
        for key, argument, part in GATHERED:
            if getattr(args, argument, None):
                summary.update(part(gather(key, passes, world, job_store if world > 1 else None)))
        if "msa" in summary and "scores" in summary:    # --msa-report with --natives: accuracy against depth
            summary.update(neff_tm_summary(summary["msa"], summary["scores"]))
        print(json.dumps(summary), flush=True)
    if (failed_all or broke_all) and status == 0:
        status = 1                                   # every rank of a job that lost targets fails, rank 0 included
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return status


if __name__ == "__main__":
    sys.exit(main())
