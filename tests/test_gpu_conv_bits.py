"""The bf16x6 convolution (option "conv_mode" 2) gives the bits recorded from the build before its weight staging and
tile buffering were changed (tests/golden/conv_bf16_bits.json, written by tools/record_conv_bits.py on that build), and
the f16x3 convolution (mode 0) those of the build before the two kernels were put on one frame (conv_f16_bits.json): the
order of the MFMAs per accumulator is part of a kernel's contract, so a change of how operands reach the registers, or
of the frame around the MFMA loop, must not move a bit of the output or of the InstanceNorm statistics."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_conv_bits", os.path.join(ROOT, "tools", "record_conv_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module", params=[2, 0], ids=["bf16x6", "f16x3"])
def mode(request):
    return request.param


@pytest.fixture(scope="module")
def recorded(mode):
    rec = _tool()
    with open(rec.GOLDEN[mode]) as f:
        golden = json.load(f)
    assert golden["conv_mode"] == mode
    return golden["cases"]


def test_recorded_cases_are_the_tools_cases(recorded):
    rec = _tool()
    want = {rec.case_name(L, bands, block) for L, bands in rec.SIZES for block in rec.BLOCKS}
    assert set(recorded) == want


def test_convolution_bits_equal_the_recorded_build(synth_sd, mode, recorded):
    """Every case of tools/record_conv_bits.py: one 8 x 16 tile column (L = 16), a second tile row and column of one
    pixel (17), both tile shapes at one size (33), the automatic switch of the shape (80 / 81), an exact multiple of the
    16 x 16 tile (96); first and last weight block.  The 8 input stages x 10 passes and the parity of the tile buffer are
    the same at every L."""
    rec = _tool()
    st = rec.make_stages(synth_sd, mode)
    try:
        got = rec.run_cases(st)
    finally:
        st.eng.close()
    bad = [k for k in sorted(recorded) if got.get(k) != recorded[k]]
    assert not bad, f"bits differ from the recorded build in {bad}"


def test_two_streams_back_to_back_give_the_recorded_bits(synth_sd, mode, recorded):
    """Two engines on two streams each run the L = 81 case four times back to back, concurrently: workgroups of different
    launches then share a CU's LDS (two workgroups of 77824 bytes fit, bf16x6; two of 55296 bytes, f16x3).  Every result
    equals the recorded digest."""
    rec = _tool()
    L, block, reps = 81, 1, 4
    want = recorded[rec.case_name(L, 0, block)]
    stages = [rec.make_stages(synth_sd, mode) for _ in range(2)]
    try:
        x = [st.to(rec.case_input(L)) for st in stages]
        outs = [[(st.f32(128, L, L), st.poisoned((128, 2), torch.float64)) for _ in range(reps)] for st in stages]
        torch.cuda.synchronize()
        for st in stages:
            st.eng._stream = torch.cuda.Stream(st.dev)          # each engine's launches on a stream of its own
        for r in range(reps):
            for st, xi, o in zip(stages, x, outs):
                st.call("dmp_block_conv5x5_maxout", block, xi, L, o[r][0], o[r][1])
        for st in stages:
            st.eng.sync_check()
        torch.cuda.synchronize()
        for e, (st, o) in enumerate(zip(stages, outs)):
            st.check_guards()
            for r, (u, stats) in enumerate(o):
                assert {"u": rec.digest(u), "stats": rec.digest(stats)} == want, (e, r)
    finally:
        for st in stages:
            st.eng.close()
