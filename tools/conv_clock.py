#!/usr/bin/env python
"""In-kernel clock of the bf16x6 convolution (precision 2) at L = 300: shader cycles over 100 MHz reference ticks around
the stage loop of every workgroup, after >= 2 s of back-to-back trunk passes on random data.  Tells whether cycles saved
in the kernel came back as time or as a lower clock.

Needs a DIAGNOSTIC library: trunk.hip compiled with -DCQ_CLOCK_STAMPS (conv_bf16.h; the library `python -m
dmpfold2_amd.build` makes executes no stamp), given through DMPFOLD_HIP_LIB:

    DMPFOLD_HIP_LIB=/path/to/diagnostic/libdmpfold_hip.so python tools/conv_clock.py [tag]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dmpfold2_amd import synth                       # noqa: E402
from abi import Stages                               # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "conv"
L = 300
st = Stages(synth.synth_weights(0, coord_scale=5.0), L, 8)
if not hasattr(st.lib, "dmp_debug_conv_clock"):
    sys.exit("this library has no clock stamps: build trunk.hip with -DCQ_CLOCK_STAMPS and point DMPFOLD_HIP_LIB at it")
st.eng.set_option("precision", 2)
z0 = torch.randn(384, L, L, device=st.dev)
dmap = torch.full((L, L), -1.0, device=st.dev)
t0 = time.time()
while time.time() - t0 < 2.5:
    for _ in range(10):
        st.trunk_pass(z0, dmap)
    torch.cuda.synchronize()
blocks = 8 * ((19 * 19 + 1) // 2)                    # conv_split_grid(19 tiles)
buf = np.zeros((blocks, 2), dtype=np.uint64)
st.lib.dmp_debug_conv_clock.restype = C.c_int
st.lib.dmp_debug_conv_clock.argtypes = [C.c_void_p, C.c_int]
assert st.lib.dmp_debug_conv_clock(buf.ctypes.data, blocks) == 0
ok = buf[:, 1] > 0                                   # slots past the last tile return without stamping
cyc, ticks = buf[ok, 0].astype(np.float64), buf[ok, 1].astype(np.float64)
print(f"CONVCLOCK {tag}: workgroups={int(ok.sum())} median stage-loop cycles={np.median(cyc):.0f} "
      f"ticks={np.median(ticks):.0f} clock={np.median(cyc / ticks) * 100:.0f} MHz "
      f"(p10 {np.percentile(cyc / ticks, 10) * 100:.0f}, p90 {np.percentile(cyc / ticks, 90) * 100:.0f})", flush=True)
st.eng.close()
