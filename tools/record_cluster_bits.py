#!/usr/bin/env python
"""Record the bits of the three cluster kernels - seq_gru_kernel, refine_cluster_kernel, tridiag_cluster_kernel: the
kernels whose workgroups hand values over inside one launch (DESIGN section "Cluster hand-off") - at the sizes where the
hand-off can go wrong.

    python tools/record_cluster_bits.py [out.json]      (default: tests/golden/cluster_bits.json)

Runs the stage calls of tests/abi.py on host-generated inputs and one whole restrained prediction, each with option
"cluster_local" 1 and 0 and each twice (the two runs must agree), and writes the SHA-256 of the raw output bytes per
case.  Run it on the build whose bits are the reference (the commit before a change of cluster.h or of one of the three
kernels that must not change them; DMPFOLD_HIP_LIB selects a library) and commit the JSON;
tests/test_gpu_cluster_bits.py asserts that the current build gives the same digests.  The cases and the inputs are
defined here, once, for both sides.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster_bits.json")

LOCALS = [1, 0]                     # option "cluster_local": XCD-local publication where the cluster finds itself on one XCD / never
# dmp_gru_bidir: `which` 0 (hgru, input T x 512) and 1 (coord_gru, T x 520).  T = 2: both granule parities once; 9 and 65:
# odd lengths, so the two directions end on different parities
GRU_WIDTH = {0: 512, 1: 520}
GRU_T = [2, 9, 65]
# dmp_refine_coords: 32 = first length that takes the cluster (every workgroup owns two residues), 33 = the last five
# workgroups own nothing, 47 = ragged last owner, 513 = 33 residues per workgroup and 15 slices
REFINE_L = [32, 33, 47, 513]
REFINE_STEPS = [1, 2, 21]
# dmp_eigh_top8: 8 and 9 = fewer rows than workgroups, 33 = one workgroup owns two rows, 65, 257 and 513 = the second
# and third per-thread index of the sweep, 640 = the kernel's largest order
EIG_N = [8, 9, 33, 65, 257, 513, 640]
# one whole prediction with the restrained final refinement (RESTRAIN = true, which no stage call reaches)
PREDICT = dict(L=33, N=17, seed=5, iterations=1, minsteps=20, restrain=1.0)
MAX_L, MAX_N = 640, 64


def case_names():
    names = [f"gru_which{w}_T{T}" for w in GRU_WIDTH for T in GRU_T]
    names += [f"refine_L{L}_steps{s}" for L in REFINE_L for s in REFINE_STEPS]
    names += [f"eigh_n{n}" for n in EIG_N]
    names += ["predict_restrained_coords", "predict_restrained_confs"]
    return [f"{n}_local{loc}" for loc in LOCALS for n in names]


def gru_input(which, T):
    rng = np.random.default_rng(8100 + 10 * T + which)
    return rng.standard_normal((T, GRU_WIDTH[which])).astype(np.float32)


def refine_input(L):
    """a well-spread random-walk chain with bonds of 3.8 A"""
    rng = np.random.default_rng(8200 + L)
    step = rng.standard_normal((L, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, axis=0).astype(np.float32)


def eig_input(n):
    rng = np.random.default_rng(8300 + n)
    b = rng.standard_normal((n, n))
    return ((b + b.T) * 3).astype(np.float32)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make_stages(state_dict=None):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from abi import Stages
    from dmpfold2_amd import synth
    st = Stages(state_dict if state_dict is not None else synth.synth_weights(0, coord_scale=5.0), max_L=MAX_L, max_N=MAX_N)
    st.eng.set_option("precision", 2)       # the whole prediction's trunk: a context's default, whatever DMPFOLD_PRECISION says
    return st


def run_cases(st):
    """{case name: sha256} of every case on the Stages `st`; raises if two runs of a case differ or a hand-off timed out"""
    from dmpfold2_amd import synth
    from dmpfold2_amd.predict import encode_aln
    out = {}

    def twice(name, local, run):
        a, b = digest(run()), digest(run())
        st.eng.sync_check()                       # raises DeviceFault on a hand-off time-out
        assert a == b, f"{name}: two runs differ"
        out[f"{name}_local{local}"] = a

    gru = {(w, T): st.to(gru_input(w, T)) for w in GRU_WIDTH for T in GRU_T}
    chains = {L: st.to(refine_input(L)) for L in REFINE_L}
    mats = {n: st.to(eig_input(n)) for n in EIG_N}
    aln = encode_aln(synth.synth_msa(PREDICT["L"], PREDICT["N"], PREDICT["seed"]))
    try:
        for local in LOCALS:
            st.eng.set_option("cluster_local", local)
            for (w, T), x in gru.items():
                twice(f"gru_which{w}_T{T}", local, lambda: st.gru_bidir(w, x))
            for L, ca in chains.items():
                for steps in REFINE_STEPS:
                    twice(f"refine_L{L}_steps{steps}", local, lambda: st.refine(ca, steps))
            for n, m in mats.items():
                twice(f"eigh_n{n}", local, lambda: st.eigh_top8(m))
            res = []
            for _ in range(2):
                c, f = st.eng.predict(aln, None, PREDICT["iterations"], PREDICT["minsteps"], restrain=PREDICT["restrain"])
                res.append((digest(c), digest(f)))
            st.eng.sync_check()
            assert res[0] == res[1], "predict_restrained: two runs differ"
            out[f"predict_restrained_coords_local{local}"], out[f"predict_restrained_confs_local{local}"] = res[0]
        st.check_guards()
    finally:
        st.eng.set_option("cluster_local", 1)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    st = make_stages()
    try:
        got = run_cases(st)
    finally:
        st.eng.close()
    assert sorted(got) == sorted(case_names())
    with open(path, "w") as f:
        json.dump({"inputs": "numpy default_rng(8100 + 10 T + which) / (8200 + L) / (8300 + n), see the tool",
                   "weights": "synth.synth_weights(0, coord_scale=5.0)", "cases": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases -> {path}")


if __name__ == "__main__":
    main()
