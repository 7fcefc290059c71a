#!/usr/bin/env python
"""Record the bits of a split-product convolution - bf16x6 (option "conv_mode" 2) or f16x3 (0, default "act_scaling") - at
the sizes where the kernel can go wrong.

    python tools/record_conv_bits.py [conv_mode [out.json]]      (default: 2 -> tests/golden/conv_bf16_bits.json,
                                                                            0 -> tests/golden/conv_f16_bits.json)

Runs the stage-level convolution (tests/abi.py Stages.conv) on host-generated inputs and writes the SHA-256 of the output
`u` and of the InstanceNorm statistics per case.  Run it on the build whose bits are the reference (the commit before a
change of conv_split.h, conv_bf16.h or conv_f16.h that must not change them) and commit the JSON;
tests/test_gpu_conv_bits.py asserts that the current build gives the same digests.  The cases and the inputs are defined
here, once, for both modes and for both sides.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = {mode: os.path.join(ROOT, "tests", "golden", name)
          for mode, name in ((2, "conv_bf16_bits.json"), (0, "conv_f16_bits.json"))}

# (L, "conv_tile_bands"): 0 = chosen by length (8 x 16 tiles up to L = 80, 16 x 16 above)
SIZES = [
    (16, 0),            # one tile column
    (17, 0),            # a second tile row and column of one pixel; bands below the last row write zero partial sums
    (33, 1), (33, 2),   # both template instances at one size
    (80, 0), (81, 0),   # the automatic switch <4> -> <8>
    (96, 0),            # exact multiple of 16 in the <8> shape
]
BLOCKS = [1, 16]        # first and last weight block
MAX_L = 96


def case_name(L, bands, block):
    return f"L{L}_bands{bands}_block{block}"


def case_input(L):
    """float32 (128, L, L), host generator"""
    rng = np.random.default_rng(7000 + L)
    return (rng.standard_normal((128, L, L)) * 3).astype(np.float32)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make_stages(state_dict=None, mode=2):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from abi import Stages
    from dmpfold2_amd import synth
    st = Stages(state_dict if state_dict is not None else synth.synth_weights(0, coord_scale=5.0), max_L=MAX_L, max_N=64)
    st.eng.set_option("conv_mode", mode)
    return st


def run_cases(st):
    """{case name: {"u": sha256, "stats": sha256}} of every case on the Stages `st` (conv_mode set by make_stages)"""
    out = {}
    try:
        for L, bands in SIZES:
            x = st.to(case_input(L))
            st.eng.set_option("conv_tile_bands", bands)
            for block in BLOCKS:
                u, stats = st.conv(block, x)
                st.eng.sync_check()
                out[case_name(L, bands, block)] = {"u": digest(u), "stats": digest(stats)}
        st.check_guards()
    finally:
        st.eng.set_option("conv_tile_bands", 0)
    return out


def main():
    mode = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN[mode]
    st = make_stages(mode=mode)
    try:
        got = run_cases(st)
    finally:
        st.eng.close()
    with open(path, "w") as f:
        json.dump({"conv_mode": mode, "input": "numpy default_rng(7000 + L).standard_normal((128, L, L)) * 3, float32",
                   "weights": "synth.synth_weights(0, coord_scale=5.0)", "cases": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases -> {path}")


if __name__ == "__main__":
    main()
