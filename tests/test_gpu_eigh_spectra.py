"""dmp_eigh_top8 on degenerate, clamped and exactly structured spectra (tests/eigh_ref.py): repeated eigenvalues, a
cluster across the 8th / 9th boundary, all-negative spectra, scale extremes, and the diagonal / tridiagonal / block
inputs that take the tau == 0 branch of the three Householder forms.  Eigenvectors inside a cluster are not unique, so
every output is held to the basis-independent invariants of eigh_ref.check, whose bounds are derived there from the
number formats; tests/test_eigh_ref_cpu.py shows that they are fair and that they bite.

Orders: 8 (all eigenvalues wanted), 9, 16, 63 .. 65 (one wave's rows; the 64-step graph chain and its padding), 129;
321 (backtransform_kernel<10, 2>), 385 (tri_eig_kernel<1>), 641 (above TC_MAX_N: the default is the per-step graph);
1281 (tri_eig_kernel<2>: Gram-Schmidt on global memory, tridiag_step_kernel<8>).  Every form is run twice and must
repeat its bits; the forms need not agree with each other bit for bit (near-null columns may differ).

`pytest -s` prints the largest error / bound per check and where it occurred."""
import numpy as np
import pytest
import torch

import eigh_ref as E

pytestmark = pytest.mark.gpu

CLUSTER = {"tridiag_cluster": 1, "tridiag_single": 0}           # the default
PER_STEP = {"tridiag_cluster": 0, "tridiag_single": 0}
SINGLE = {"tridiag_cluster": 1, "tridiag_single": 1}
SMALL = (8, 9, 16, 63, 64, 65, 129)
MEDIUM = (321, 385, 641)
MEDIUM_GENERATORS = ("separated", "octet", "straddle", "rank3", "zero", "identity_1", "identity_1e6", "identity_neg1")
LARGE = (1281,)
LARGE_GENERATORS = ("octet", "rank3")

_WORST = {}


def _context(synth_sd, max_L):
    from abi import Stages
    st = Stages(synth_sd, max_L=max_L, max_N=4)
    yield st
    st.eng.sync_check()
    st.check_guards()
    st.eng.close()


@pytest.fixture(scope="module")
def small(synth_sd):
    yield from _context(synth_sd, max(SMALL))


@pytest.fixture(scope="module")
def medium(synth_sd):
    yield from _context(synth_sd, max(MEDIUM))


@pytest.fixture(scope="module")
def large(synth_sd):
    yield from _context(synth_sd, max(LARGE))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\ndmp_eigh_top8: largest error / bound per check (generator, order, form):")
        for k in sorted(_WORST):
            r, name, n, form, note = _WORST[k]
            print(f"  check {k}: {r:.4f}  ({name}, n = {n}, {form}, {note})")


def _run(st, name, n, forms):
    M = E.GENERATORS[name](n)
    T = E.truth(M)
    dM = st.to(M)
    bad = []
    try:
        for form, opts in forms.items():
            for k, v in opts.items():
                st.eng.set_option(k, v)
            a = st.eigh_top8(dM).clone()
            b = st.eigh_top8(dM).clone()
            st.eng.sync_check()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} n = {n} {form}: two runs differ"
            res = E.check(M, a.cpu().numpy(), T)
            for k, (r, note) in res.items():
                if k not in _WORST or r > _WORST[k][0]:
                    _WORST[k] = (r, name, n, form, note)
            f = E.failed(res)
            if f:
                bad.append((form, {k: res[k] for k in f}))
    finally:
        for k, v in CLUSTER.items():
            st.eng.set_option(k, v)
    st.check_guards()
    assert not bad, f"{name} n = {n}: {bad}"


@pytest.mark.parametrize("name", sorted(E.GENERATORS))
@pytest.mark.parametrize("n", SMALL)
def test_small_orders_every_generator_three_forms(small, n, name):
    _run(small, name, n, {"cluster": CLUSTER, "per step": PER_STEP, "single workgroup": SINGLE})


@pytest.mark.parametrize("name", MEDIUM_GENERATORS)
@pytest.mark.parametrize("n", MEDIUM)
def test_medium_orders_two_forms(medium, n, name):
    _run(medium, name, n, {"default": CLUSTER, "per step": PER_STEP})


@pytest.mark.parametrize("name", LARGE_GENERATORS)
@pytest.mark.parametrize("n", LARGE)
def test_large_order_default_form(large, n, name):
    _run(large, name, n, {"default": CLUSTER})
