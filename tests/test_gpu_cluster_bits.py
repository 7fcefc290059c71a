"""The three cluster kernels - seq_gru_kernel, refine_cluster_kernel, tridiag_cluster_kernel - give the bits recorded from
the build before their hand-off was put into one header (tests/golden/cluster_bits.json, written by
tools/record_cluster_bits.py on that build): the hand-off carries values, it computes nothing, so a change of how granules
are packed, published, gathered or laid out must not move a bit of what the kernels produce - with the XCD-local
publication and without it, and twice in a row."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_cluster_bits", os.path.join(ROOT, "tools", "record_cluster_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(_tool().GOLDEN) as f:
        return json.load(f)["cases"]


def test_recorded_cases_are_the_tools_cases(recorded):
    assert set(recorded) == set(_tool().case_names())


def test_cluster_kernel_bits_equal_the_recorded_build(synth_sd, recorded):
    """Every case of tools/record_cluster_bits.py, each with "cluster_local" 1 and 0 and each twice (run_cases raises if the
    two runs differ or if a hand-off timed out).  Sequence GRUs of both widths at T = 2 (both granule parities once), 9 and
    65 (odd: the directions end on different parities); the minimiser at L = 32 (first length of the cluster), 33 (the last
    five workgroups own nothing), 47 (ragged last owner) and 513 (33 residues per workgroup, 15 slices) for 1, 2 and 21
    steps; the tridiagonalisation inside dmp_eigh_top8 at n = 8, 9 (fewer rows than workgroups), 33, 65, 257, 513 (second
    and third per-thread index of the sweep) and 640 (largest order); one whole prediction with the restrained final
    refinement, the RESTRAIN = true instantiation."""
    rec = _tool()
    st = rec.make_stages(synth_sd)
    try:
        got = rec.run_cases(st)
    finally:
        st.eng.close()
    bad = [k for k in sorted(recorded) if got.get(k) != recorded[k]]
    assert not bad, f"bits differ from the recorded build in {bad}"
