#!/usr/bin/env python
"""Record what the Python host does around a prediction - where the blocks lie, which options a call sets, what the front
ends accept and write - as tests/golden/host_plumbing.json.gz (JSON, gzip with no time stamp: two runs on one commit give
the same bytes; `zcat` shows it).

    python tools/record_host_plumbing.py [OUT.json.gz]

Run it on the commit whose behaviour is to be kept; tests/test_host_plumbing_cpu.py then holds every later commit to the
file, section by section and row by row.  It reaches the code through public names only (and Engine._call_options, which
the tests of the options have always called on a stub), so it runs unchanged on both sides of a change.  No GPU, no library.

Every section is a list of [case, value] rows:

  signatures    str(inspect.signature) of the callables whose signature carries the options, the first eight parameters of
                batch.write_result, the fields and defaults of Prediction
  parsers       the help text of both parsers (white space normalised: the wrapping follows the terminal) and vars() of
                the empty command line and of one that sets every option
  layout        score.Layout on L (8, 2048) x (distmap, score, score_map) x search (None, (3, 40)) x passes (None, 1, 128) x ss
                x exposure, with one align block (m = 65, one more than max_L = 64: the rule of B0 puts the search block inside
                it): the eleven named offsets of OFFSETS, then field, first element, size - flat - of every view `split`
                gives on an arange buffer (a field by its index in FIELDS)
  outputs       score.Outputs over all 2^9 presence patterns of distmap, info and the seven blocks: what `public()` and
                `public(blocks=False)` hand out, a letter per part (C coords, c confs, the index in FIELDS of the rest, - for a
                None), and whether `Outputs.of` gives every part back (by identity)
  call_options  Engine._call_options on a recording stub for every subset of the ten things of ASKED a call can ask for, on
                an engine with nothing set by hand ("n") and on one with everything set ("e"): the set_option calls on entry
                and on exit as indices into "texts" (an option by its letter in SHORT), or "raised" and the exception; the
                recorder itself checks that a call that raised had set nothing and that the others left the options as they were
  agreement     agree_options ("o") over all pairs of 32 option states, agree_passes ("p": a, b, score, iterations) and
                agree_ss ("s", "x" with the names of "exposure") over all pairs of two engines' values: the Flags / value, or
                "raised" and the exception as an index into "texts"
  batch_files   batch.write_result with every result given, per format: the SHA-256 of every file it writes (of an .npz
                the digest of its arrays - names, dtypes, shapes, bytes -, since the container holds a time stamp)
  batch_summary the JSON line batch.main prints as rank 0 of 3 from hand-made per-rank results, with the GPU, the run and
                the process group replaced by stand-ins, and the SHA-256 of what it wrote to the job's store under each key"""
import contextlib
import gzip
import hashlib
import inspect
import io
import itertools
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmpfold2_amd import batch, predict as P, score as S          # noqa: E402

FIELDS = ("confs", "distmap", "info", "score_block", "align_block", "search_block", "map_block", "pass_block", "ss_block",
          "exposure_block")
OFFSETS = ("info_off", "score_off", "mapscore_off", "pass_off", "ss_off", "exposure_off", "align_off", "align_end",
           "search_off", "search_end", "total")


class Texts:
    """Long strings (exception messages, lists of calls) stored once; rows hold their index."""

    def __init__(self):
        self.all = []

    def __call__(self, text):
        if text not in self.all:
            self.all.append(text)
        return self.all.index(text)


def _raised(exc):
    return f"{type(exc).__name__}: {exc}"


# ---- 1. signatures ------------------------------------------------------------------------------------------------------
def signatures():
    fns = [("Engine." + n, getattr(P.Engine, n)) for n in ("predict", "predict_device", "predict_checked", "predict_device_checked")]
    fns += [("Pipeline.__init__", P.Pipeline.__init__), ("Pipeline.submit", P.Pipeline.submit)]
    fns += [("Pipeline." + n, getattr(P.Pipeline, n)) for n in sorted(dir(P.Pipeline)) if n.startswith("set_")]
    fns += [("aln_to_coords", P.aln_to_coords), ("_predict_file", P._predict_file), ("run_batch", batch.run_batch)]
    rows = [[name, str(inspect.signature(fn))] for name, fn in fns]
    rows.append(["write_result[:8]", [str(p) for p in list(inspect.signature(batch.write_result).parameters.values())[:8]]])
    rows.append(["Prediction", [list(P.Prediction._fields), {k: v for k, v in P.Prediction._field_defaults.items()}]])
    return rows


# ---- 2. parsers ---------------------------------------------------------------------------------------------------------
EVERY_DMPFOLD = ("-i x.aln -d cuda:1 -t t.pdb -n 3 -m 20 -w w.pt -c 0.25 --distmap d.npy --native n.pdb --native-chain B --score-map "
                 "--score-passes --scores s.json --compare c.pdb --compare-chain C --alignment a.json --search lib.npz --search-top 4 "
                 "--hits h.json --ss --ss-file ss.json --exposure --exposure-file e.json -r 1.5 --restrain-cutoff 12").split()
EVERY_BATCH = ("-l t.txt -i a.aln b -o out --format npz -n 3 -m 20 -w w.pt --streams 2 --static-shards --converge 0.25 --distmap "
               "--natives nat --score-map --score-passes --structures st --library lib.npz --search-top 4 --ss --exposure "
               "--restrain 1.5 --restrain-cutoff 12").split()


def parsers():
    rows = []
    for name, make, empty, every in (("dmpfold", P.dmpfold_parser, ["-i", "x.aln"], EVERY_DMPFOLD),
                                     ("dmpfold-batch", batch.batch_parser, ["-o", "out"], EVERY_BATCH)):
        parser = make()
        parser.prog = name                               # (not the running program's name)
        rows.append([name + " --help", " ".join(parser.format_help().split())])
        rows.append([name + " empty", vars(make().parse_args(empty))])
        rows.append([name + " every option", vars(make().parse_args(every))])
    return rows


# ---- 3. layout ----------------------------------------------------------------------------------------------------------
def layout_cells():
    return itertools.product((8, 2048), itertools.product((False, True), repeat=3), ((65, 64),),
                             (None, (3, 40)), (None, 1, 128), (False, True), (False, True))


def layout():
    rows, bufs = [], {}
    for L, (distmap, score, score_map), (align_m, max_L), search, passes, ss, exposure in layout_cells():
        lay = S.Layout(L, distmap, score, score_map, align_m, search, max_L, passes=passes, ss=ss, exposure=exposure)
        if L not in bufs:
            bufs[L] = np.arange(L + L * L + 3 + 64 * L + 8192, dtype=np.float64)       # (float64: every index is exact)
        out = lay.split(bufs[L][:lay.total])
        views = [n for k, f in enumerate(FIELDS) for v in [getattr(out, f)] if v is not None for n in (k, int(v.reshape(-1)[0]), int(v.size))]
        rows.append(["L%d %d%d%d m%d/%d K%s R%s ss%d exp%d" % (L, distmap, score, score_map, align_m, max_L, search and search[0], passes, ss, exposure),
                     [int(getattr(lay, name)) for name in OFFSETS] + views])
    return rows


# ---- 4. Outputs ---------------------------------------------------------------------------------------------------------
def outputs():
    rows = []
    for present in itertools.product((False, True), repeat=9):
        parts = {f: f for f, on in zip(FIELDS[1:], present) if on}                   # (each part is its own name)
        out = S.Outputs(coords="coords", confs="confs", **parts)
        pub = out.public()
        on = dict(zip(FIELDS[1:], present))
        back = S.Outputs.of(pub, on["distmap"], on["score_block"], on["align_block"], on["search_block"], on["map_block"],
                            on["pass_block"], ss=on["ss_block"], exposure=on["exposure_block"])
        same = all(getattr(back, f) is getattr(out, f) for f in ("coords",) + FIELDS)
        letters = dict({"coords": "C", "confs": "c", None: "-"}, **{f: str(k) for k, f in enumerate(FIELDS)})
        rows.append(["".join("1" if p else "0" for p in present), "".join(letters[x] for x in pub) + " "
                     + "".join(letters[x] for x in out.public(blocks=False)) + (" same" if same else " differs")])
    return rows


# ---- 5. _call_options ---------------------------------------------------------------------------------------------------
ASKED = ("distmap", "native", "structure", "library", "score_map", "score_passes", "ss", "exposure", "restrain", "converge")
NOTHING = {"recycle_tol_mA": 0, "emit_distmap": 0, "score_native": 0, "score_map": 0, "score_passes": 0, "assign_ss": 0, "exposure": 0,
           "align_structure": 0, "search_structures": 0, "search_max_m": 0, "restrain_milli": 0, "restrain_cut_mA": 15000}
BY_HAND = {"recycle_tol_mA": 40, "emit_distmap": 1, "score_native": 1, "score_map": 1, "score_passes": 1, "assign_ss": 1, "exposure": 1,
           "align_structure": 1, "search_structures": 3, "search_max_m": 9, "restrain_milli": 500, "restrain_cut_mA": 9000}
NATIVE = np.zeros((8, 3), dtype=np.float32)
STRUCTURE = np.zeros((6, 3), dtype=np.float32)
LIBRARY = S.Library.from_traces([np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32), np.zeros((3, 3), np.float32)])


SHORT = {"recycle_tol_mA": "T", "emit_distmap": "D", "score_native": "N", "score_map": "M", "score_passes": "P", "assign_ss": "S",
         "exposure": "X", "align_structure": "A", "search_structures": "K", "search_max_m": "m", "restrain_milli": "r",
         "restrain_cut_mA": "c"}


class Stub:
    """get_option / set_option of an engine, every set recorded."""

    def __init__(self, options):
        self.options, self.sets, self.max_L = dict(options), [], 64

    def get_option(self, name):
        return self.options[name]

    def set_option(self, name, value):
        self.sets.append(f"{SHORT[name]}{value}")
        self.options[name] = value


def call_options(texts):
    rows = []
    for hand, options in (("n", NOTHING), ("e", BY_HAND)):
        for asked in itertools.product((False, True), repeat=len(ASKED)):
            a = dict(zip(ASKED, asked))
            extras = P.Extras(a["distmap"], NATIVE if a["native"] else None, STRUCTURE if a["structure"] else None,
                              LIBRARY if a["library"] else None, a["score_map"], a["score_passes"], ss=a["ss"], exposure=a["exposure"])
            stub = Stub(options)
            case = hand + "".join("1" if v else "0" for v in asked)
            try:
                with P.Engine._call_options(stub, 0.25 if a["converge"] else None, extras,
                                            P.restrain_options(1.5, 12.0) if a["restrain"] else None):
                    entry = list(stub.sets)
                assert stub.options == options, case
                value = [texts(" ".join(entry)), texts(" ".join(stub.sets[len(entry):]))]
            except Exception as exc:                                         # noqa: BLE001 - whatever it is, it is recorded
                assert stub.sets == [], case
                value = ["raised", texts(_raised(exc))]
            rows.append([case, value])
    return rows


# ---- 6. agreement -------------------------------------------------------------------------------------------------------
STATES = [bits + (k,) for bits in itertools.product((0, 1), repeat=4) for k in (0, 3)]


def _or_text(texts, fn, *args):
    try:
        out = fn(*args)
        return list(out) if isinstance(out, tuple) else out
    except Exception as exc:                                                 # noqa: BLE001
        return ["raised", texts(_raised(exc))]


def agreement(texts):
    def name(state):
        return "".join(str(v) for v in state)
    rows = [[f"o {name(a)} {name(b)}", _or_text(texts, P.agree_options, [a, b])] for a in STATES for b in STATES]
    rows.append(["o three engines", _or_text(texts, P.agree_options, iter([(1, 0, 0, 0, 0)] * 2 + [(0, 0, 0, 0, 0)]))])
    for a, b, score, iterations in itertools.product((0, 1), (0, 1), (False, True), (0, 10, 500)):
        rows.append([f"p {a}{b} {int(score)} {iterations}", _or_text(texts, P.agree_passes, [a, b], score, iterations)])
    for a, b in itertools.product((0, 1), repeat=2):
        rows.append([f"s {a}{b}", _or_text(texts, P.agree_ss, iter([a, b]))])
        rows.append([f"x {a}{b}", _or_text(texts, P.agree_ss, [a, b], "exposure", "set_exposure")])
    return rows


# ---- 7. the batch front end ---------------------------------------------------------------------------------------------
L, R = 12, 4


def _pattern(n, seed):
    """n floats in 0 .. 5 by halves: counts, codes and indices every unpacker can read."""
    return (((np.arange(n) + seed) * 37) % 11).astype(np.float32) * np.float32(0.5)


def results(seed):
    """What run_batch unpacks for one target with every option on, from blocks made here."""
    alnmat = ((np.arange(2 * L).reshape(2, L) + seed) % 20).astype(np.uint8)
    search = _pattern(S.search_floats(L, 3, 15), seed)
    search[3:6] = [2.0, 0.0, 1.0]
    distmap = _pattern(L * L, seed).reshape(L, L)
    coords = _pattern(L * 15, seed + 1).reshape(L, 5, 3)
    return {"alnmat": alnmat, "coords": coords, "confs": _pattern(L, seed + 2), "distmap": distmap,
            "info": np.asarray([1.0, 3.0, 0.25], dtype=np.float32),
            "scores": S.unpack_scores(_pattern(S.score_floats(L), seed), L),
            "map_scores": S.unpack_map_scores(_pattern(S.mapscore_floats(L), seed), L),
            "pass_scores": S.unpack_pass_scores(_pattern(S.pass_floats(R), seed), R),
            "ss": S.unpack_ss(_pattern(S.ss_floats(L), seed), L),
            "exposure": S.unpack_exposure(_pattern(S.exposure_floats(L), seed), L, seq=alnmat[0]),
            "alignment": S.unpack_alignment(_pattern(S.align_floats(L, 5), seed), L),
            "hits": dict(S.unpack_search(search, L, LIBRARY.lengths), names=list(LIBRARY.names)),
            "restrain": P.restrain_report(1.5, 12.0, 20, distmap, 0.25, coords)}


def _digest(path):
    h = hashlib.sha256()
    if path.endswith(".npz"):
        with np.load(path) as z:
            for name in sorted(z.files):
                h.update(f"{name} {z[name].dtype.str} {z[name].shape} ".encode() + np.ascontiguousarray(z[name]).tobytes())
    else:
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def batch_files():
    import torch
    rows = []
    r = results(0)
    for fmt in ("pdb", "ca", "npz"):
        with tempfile.TemporaryDirectory() as tmp:
            path = batch.write_result(tmp, "some/where/t1.aln", torch.from_numpy(r["coords"]), torch.from_numpy(r["confs"]),
                                      r["alnmat"], fmt, torch.from_numpy(r["distmap"]), torch.from_numpy(r["info"]), hits_top=2,
                                      **{k: r[k] for k in ("scores", "map_scores", "pass_scores", "ss", "exposure", "alignment",
                                                           "hits", "restrain")})
            rows.append([fmt, [os.path.basename(path), {f: _digest(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp))}]])
    return rows


def rank_stats(rank):
    """The `stats_out` of run_batch on one rank: two targets, the second without native and structure (rank 0; the other
    ranks have the first only)."""
    stats = {"passes_run": 7 + rank, "passes_saved": 3 * rank, "scores": {}, "alignments": {}, "hits": {}, "ss": {}, "exposure": {},
             "restrain": {}}
    for k in range(2 if rank == 0 else 1):
        stem, r = f"r{rank}t{k}", results(10 * rank + k)
        if k == 0:
            stats["scores"][stem] = dict(S.scores_json(r["scores"]), map=S.map_scores_json(r["map_scores"]),
                                         passes=S.pass_scores_json(r["pass_scores"]))
            js = S.alignment_json(r["alignment"])
            stats["alignments"][stem] = {name: js[name] for name in ("m",) + S.ALIGN_NAMES}
        stats["hits"][stem] = [{n: v for n, v in h.items() if n not in ("R", "t")}
                               for h in S.hits_json(r["hits"], LIBRARY.names, 2)["hits"]]
        stats["ss"][stem] = S.ss_json(r["ss"])
        stats["exposure"][stem] = S.exposure_json(r["exposure"])
        stats["restrain"][stem] = r["restrain"]
    return stats


class FakeStore(dict):
    """The job's key-value store: `set` / `get` of torch.distributed's, backed by a dict."""

    def set(self, key, value):
        self[key] = value.encode() if isinstance(value, str) else value

    def get(self, key):
        return self[key]


def batch_summary():
    import torch
    import torch.distributed as dist
    store = FakeStore()
    for rank in (1, 2):
        for name, value in rank_stats(rank).items():
            if isinstance(value, dict):
                store.set(f"dmpfold_batch_{name}/{rank}", json.dumps(value))
    theirs = sorted(store)

    def fake_run(targets, out_dir, *args, stats_out=None, **kw):
        stats_out.update(rank_stats(0))
        return 2, 1.5, []

    stand_ins = [(batch, "run_batch", fake_run), (batch.shard, "job_store", lambda rank, world: store),
                 (batch.shard, "job_summary", lambda n, elapsed, failures=None: (3 * n, 2.0 * elapsed, 0, 0)),
                 (batch.shard, "sum_over_ranks", lambda counts: [3 * c + 3 for c in counts]),
                 (batch.shard, "pin_rank_to_cores", lambda *a, **kw: []), (torch.cuda, "set_device", lambda d: None),
                 (dist, "init_process_group", lambda *a, **kw: None), (dist, "destroy_process_group", lambda *a, **kw: None)]
    kept = [(mod, name, getattr(mod, name)) for mod, name, _ in stand_ins]
    env = {k: os.environ.get(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "HSA_ENABLE_IPC_MODE_LEGACY")}
    text = io.StringIO()
    try:
        for mod, name, fn in stand_ins:
            setattr(mod, name, fn)
        os.environ.update(RANK="0", WORLD_SIZE="3", LOCAL_RANK="0")
        with contextlib.redirect_stdout(text):
            status = batch.main("-i a.aln -o out --converge 0.25 --distmap --natives nat --score-map --score-passes --structures st "
                                "--library lib.npz --search-top 2 --ss --exposure --restrain 1.5".split())
    finally:
        for mod, name, fn in kept:
            setattr(mod, name, fn)
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return [["status", status], ["rank 0 stored", {k: hashlib.sha256(store[k]).hexdigest() for k in sorted(store) if k not in theirs}],
            ["summary line", text.getvalue()]]


def record():
    os.environ["COLUMNS"] = "100"
    texts = Texts()
    doc = {"signatures": signatures(), "parsers": parsers(), "layout": layout(), "outputs": outputs(),
           "call_options": call_options(texts), "agreement": agreement(texts), "batch_files": batch_files(),
           "batch_summary": batch_summary()}
    doc["texts"] = [[k, t] for k, t in enumerate(texts.all)]
    return json.loads(json.dumps(doc))                  # (as the file gives it back: tuples are lists, keys are strings)


def _packed(rows, width=400):
    """The rows as JSON, several to a line of at most `width` characters (a longer row has a line to itself)."""
    lines = []
    for text in (json.dumps(row, separators=(",", ":")) for row in rows):
        if lines and len(lines[-1]) + len(text) < width:
            lines[-1] += "," + text
        else:
            lines.append(text)
    return ",\n".join(lines)


def main(argv):
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", "host_plumbing.json.gz")
    doc = record()
    with open(out, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as fh:
        fh.write(("{\n" + ",\n".join(json.dumps(name) + ": [\n" + _packed(rows) + "\n]" for name, rows in doc.items()) + "\n}\n").encode())
    print(", ".join(f"{name}: {len(rows)}" for name, rows in doc.items()), "->", out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
