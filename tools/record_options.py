"""Record what dmp_ctx_get_option / dmp_ctx_set_option answer for every option name of include/dmpfold_hip.h, on one GPU:

    python tools/record_options.py [--out tests/golden/options.json]

Per name, on a fresh context of its own (max_L 8, max_N 1, no weights): what the option reads, then for each probe value
the setter's return code and error text and what the option reads afterwards.  An unknown name is recorded the same way.
tests/test_gpu_options.py replays the file against the built library: run this tool on the commit whose behaviour is to be
kept, commit the file, change the library.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_L, MAX_N = 8, 1
PROBES = (-2, -1, 0, 1, 2, 3, 4, 8, 9, 4096, 4097)
UNTOUCHED = -12345          # what the value read holds where the getter left it alone
# every name of include/dmpfold_hip.h, the "act_scale_log2_block<k>" family at k = 0, 1, 16 and 17
NAMES = ("precision", "conv_mode", "conv_f32_exact", "vgru_f32", "vgru_persistent", "vgru_debug_drop_wg", "tridiag_single",
         "tridiag_cluster", "cluster_local", "refine_single", "gj_diag_groups", "gj_diag_blocked", "gj_pairs", "gj_lookahead",
         "conv_tile_bands", "act_scaling", "act_scale_log2_block0", "act_scale_log2_block1", "act_scale_log2_block16",
         "act_scale_log2_block17", "device_mib", "chain_issued", "passes_run", "recycle_tol_mA", "emit_distmap", "score_native",
         "score_map", "score_passes", "score_passes_chunk", "assign_ss", "align_structure", "search_structures", "search_max_m",
         "search_chunk", "search_chunk_used", "search_wg_per_cu")
UNKNOWN = "no_such_option"


def _error(lib, rc):
    return lib.dmp_last_error().decode("utf-8", "replace") if rc != 0 else ""


def _get(lib, ctx, name):
    v = C.c_int(UNTOUCHED)
    rc = lib.dmp_ctx_get_option(ctx, name.encode(), C.byref(v))
    return [rc, v.value, _error(lib, rc)]


def probe(lib, name, device=0):
    """-> {"fresh": [rc, value, error], "set": [[probe, rc, error, [rc, value, error]], ...]} of one name on one new context."""
    ctx = C.c_void_p()
    assert lib.dmp_ctx_create(device, MAX_L, MAX_N, C.byref(ctx)) == 0, lib.dmp_last_error()
    try:
        rec = {"fresh": _get(lib, ctx, name), "set": []}
        for value in PROBES:
            rc = lib.dmp_ctx_set_option(ctx, name.encode(), value)
            rec["set"].append([value, rc, _error(lib, rc), _get(lib, ctx, name)])
        return rec
    finally:
        lib.dmp_ctx_destroy(ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "options.json"))
    args = ap.parse_args()
    from dmpfold2_amd import _lib
    lib = _lib.load()
    doc = {"max_L": MAX_L, "max_N": MAX_N, "probes": list(PROBES), "untouched": UNTOUCHED,
           "options": {name: probe(lib, name) for name in NAMES + (UNKNOWN,)}}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d names x %d probes -> %s" % (len(doc["options"]), len(PROBES), args.out))


if __name__ == "__main__":
    main()
