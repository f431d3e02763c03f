"""Host-side checks of the full-covariance GMM work (no GPU): the references of tests/gmm_full_cases.py against sklearn and its golden,
the rule's room (emu32_alt at half of every limit), the C-ABI's bindings, the M step and the refusals of the Python layer."""
import os
import pickle
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmm_full_cases as FC  # noqa: E402

REL = 1e-10


@pytest.fixture(scope="module")
def gold():
    return np.load(FC.GOLDEN)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= REL * (np.abs(b).max() + 1e-300), (what, float(np.abs(a - b).max()))


def _step_checks(w, mu, cov, X, lse, log_resp, nk, means, covs, U_new):
    U = FC.prec_chol_of(cov)
    r = FC.ref64(w, mu, U, X)
    _close(r["lse"], lse, "lse")
    _close(r["resp"], np.exp(log_resp), "resp")
    st = FC.stats_of(r, len(w), X.shape[1])
    _close(st["nk"] + 10 * np.finfo(np.float64).eps, nk, "nk")
    w2, m2, c2, U2 = FC.m_step64(st, X.shape[0], 1e-6)
    _close(m2, means, "means")
    _close(c2, covs, "covariances")
    _close(U2, U_new, "precisions_cholesky")
    # about a shift: the same model (translation invariance), the same M step
    shift = np.asarray(X, dtype=np.float64).mean(axis=0) + 3.0
    rs = FC.ref64(w, mu, U, X, shift)
    _close(rs["lse"], lse, "lse (shift)")
    w3, m3, c3, U3 = FC.m_step64(FC.stats_of(rs, len(w), X.shape[1]), X.shape[0], 1e-6, shift)
    _close(m3, means, "means (shift)")
    _close(c3, covs, "covariances (shift)")


def test_ref64_equals_the_golden_sklearn_steps(gold):
    _step_checks(gold["step_w"], gold["step_mu"], gold["step_cov"], gold["step_X"], gold["step_lse"], gold["step_log_resp"], gold["step_nk"],
                 gold["step_means"], gold["step_covs"], gold["step_U_new"])
    _close(FC.prec_chol_of(gold["step_cov"]), gold["step_U"], "U")


def test_ref64_equals_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.mixture import GaussianMixture
    from sklearn.mixture import _gaussian_mixture as G
    rng = np.random.default_rng(5)
    w, mu, cov, _ = FC.draw_model(rng, 5, 13)
    X = FC.draw_frames(rng, w, mu, cov, 300)
    g = GaussianMixture(n_components=5, covariance_type="full")
    g.weights_, g.means_, g.covariances_, g.precisions_cholesky_ = w, mu, cov, G._compute_precision_cholesky(cov, "full")
    lse, log_resp = g._estimate_log_prob_resp(X.astype(np.float64))
    nk, means, covs = G._estimate_gaussian_parameters(X.astype(np.float64), np.exp(log_resp), 1e-6, "full")
    _step_checks(w, mu, cov, X, lse, log_resp, nk, means, covs, G._compute_precision_cholesky(covs, "full"))


def test_the_golden_inputs_are_the_seeded_ones(gold):
    for name in FC.FIT_CASES:
        X = FC.fit_data(name)[0]
        assert np.array_equal(X[:4], gold[name + "_x_head"]) and float(X.astype(np.float64).sum()) == float(gold[name + "_x_sum"]), name
    assert float(gold["orient_acc_full"]) >= 0.95 and float(gold["orient_acc_diag"]) <= 0.5


@pytest.mark.parametrize("shape", [(3, 13, 257), (5, 39, 65), (3, 64, 65), (65, 4, 130)])
@pytest.mark.parametrize("offset", [0.0, 30.0])
def test_emu32_alt_passes_at_half_of_every_limit(shape, offset):
    K, D, n = shape
    c = FC.em_case(K, D, n, offset)
    alt = FC.emu32_alt(c["w"], c["mu"], c["U"], c["X"], c["shift"])
    res = FC.compare(alt, c["ev"], FC.acc_frames(n, K), c["name"] + " emu32_alt", scale=0.5)
    assert res["worst"] <= 1.0


def test_the_rule_has_no_room_for_a_fault():
    """one mean entry moved by a hundredth of a sigma: the statistics miss the rule"""
    c = FC.em_case(3, 13, 257, 0.0)
    mu = c["mu"].copy()
    mu[0, 0] += 0.01
    bad = FC.emu32(c["w"], mu, c["U"], c["X"], c["shift"])
    with pytest.raises(AssertionError):
        FC.compare(bad, c["ev"], FC.acc_frames(257, 3), "shifted mean")


def test_acc_frames_restates_the_cap():
    assert FC.acc_frames(257, 3) == 64
    assert FC.acc_frames(125000, 130) == 64 * 123          # 1954 tiles over max(16, min(1954, 15)) walkers
    assert FC.acc_frames(125000, 130) <= 64 * FC.CAP_TILES
    assert FC.acc_frames(125000, 130, budget_mb=1) == 128   # slabs of 1792 frames: 28 tiles over 15 walkers -> two tiles each
    assert FC.slab_frames(125000, 130, 1) == 1792


def test_header_declarations_are_bound():
    from speech_signal_processing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ssp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("ssp_gmm_full_em_stats", "ssp_gmm_full_pack", "ssp_gmm_full_destroy", "ssp_gmm_full_score"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, (name, n_args)
    assert re.search(r"#define\s+SSP_ABI_VERSION\s+4\b", hdr) and _lib.ABI_VERSION == 4


def test_the_unit_is_part_of_the_build():
    from speech_signal_processing_amd.build import SOURCES
    assert "gmm_full.hip" in SOURCES


def test_constructor_takes_full_and_refuses_the_rest():
    from speech_signal_processing_amd.gmm_train import GaussianMixture
    gm = GaussianMixture(n_components=3, covariance_type="full")
    assert gm.covariance_type == "full"
    assert pickle.loads(pickle.dumps(gm)).covariance_type == "full"
    for kind in ("tied", "spherical"):
        with pytest.raises(ValueError):
            GaussianMixture(n_components=3, covariance_type=kind)


def test_m_step_matches_sklearn_on_the_golden_statistics(gold):
    from speech_signal_processing_amd.gmm_train import GaussianMixture, precision_cholesky_from_precisions_full
    w, mu, cov, X = gold["step_w"], gold["step_mu"], gold["step_cov"], gold["step_X"]
    U = FC.prec_chol_of(cov)
    gm = GaussianMixture(n_components=len(w), covariance_type="full", reg_covar=1e-6)
    for shift in (None, np.asarray(X, dtype=np.float64).mean(axis=0) - 2.0):
        st = FC.stats_of(FC.ref64(w, mu, U, X, shift), len(w), X.shape[1])
        w2, m2, c2, U2 = gm._m_step_full(st, X.shape[0], shift)
        _close(m2, gold["step_means"], "means")
        _close(c2, gold["step_covs"], "covariances")
        _close(U2, gold["step_U_new"], "precisions_cholesky")
        _close(w2, gold["step_nk"] / gold["step_nk"].sum(), "weights")
    P = np.linalg.inv(cov)
    Uf = precision_cholesky_from_precisions_full(0.5 * (P + P.transpose(0, 2, 1)))
    assert np.allclose(Uf, np.triu(Uf)) and np.allclose(Uf @ Uf.transpose(0, 2, 1), P, rtol=1e-9, atol=1e-12)
    _close(Uf, U, "precisions_cholesky from precisions")


def test_an_ill_defined_covariance_raises_sklearns_error():
    """a cluster of two identical frames, reg_covar = 0"""
    from speech_signal_processing_amd.gmm_train import GaussianMixture
    rng = np.random.default_rng(3)
    X = np.concatenate([rng.standard_normal((50, 3)), np.zeros((2, 3))])
    resp = np.zeros((52, 2))
    resp[:50, 0] = 1.0
    resp[50:, 1] = 1.0
    a1 = np.concatenate([np.ones((52, 1)), X], axis=1)
    st = FC.stats_of(dict(block=FC._block(resp, a1), ll=0.0), 2, 3)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        GaussianMixture(n_components=2, covariance_type="full", reg_covar=0.0)._m_step_full(st, 52)
    pytest.importorskip("sklearn")
    from sklearn.mixture import _gaussian_mixture as G
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        G._compute_precision_cholesky(G._estimate_gaussian_parameters(X, resp, 0.0, "full")[2], "full")


def _model(kind, K=2, D=3):
    rng = np.random.default_rng(1)
    m = types.SimpleNamespace(covariance_type=kind, weights_=np.full(K, 1.0 / K), means_=rng.standard_normal((K, D)))
    if kind == "full":
        m.covariances_ = np.tile(np.eye(D), (K, 1, 1))
        m.precisions_cholesky_ = np.tile(np.eye(D), (K, 1, 1))
    else:
        m.covariances_ = np.ones((K, D))
        m.precisions_cholesky_ = np.ones((K, D))
    return m


def test_score_matrix_refuses_mixed_sets_and_top_c_with_full_models():
    from speech_signal_processing_amd import GMM_UBM
    feats = [np.zeros((4, 3), np.float32)]
    with pytest.raises(ValueError, match="mix covariance types"):
        GMM_UBM.score_matrix([_model("full"), _model("diag")], _model("full"), feats)
    with pytest.raises(ValueError, match="mix covariance types"):
        GMM_UBM.score_matrix([_model("full")], _model("diag"), feats)
    with pytest.raises(ValueError, match="top_c"):
        GMM_UBM.score_matrix([_model("full")], _model("full"), feats, top_c=2)


def test_emu_fit_deviation_is_the_stored_one(gold):
    """the loop of fit with emu32 statistics in place of the kernel: its deviation from sklearn per parameter block is what the golden
    holds as d_emu (the GPU file's fit limit is 8 d_emu + 1e-6 (|value| + 1))"""
    for name, it in (("K5_D13", 1), ("K5_D13", 5), ("K3_D39", 1)):
        X, w0, mu0, P0 = FC.fit_data(name)
        e = FC.emu_fit(X, w0, mu0, P0, it)
        dev = FC.fit_deviation(e, FC.golden_fit(gold, "%s_it%d" % (name, it)))
        stored = dict(zip(FC.FIT_BLOCKS, gold["%s_it%d_d_emu" % (name, it)]))
        for b in FC.FIT_BLOCKS:
            assert abs(dev[b] - stored[b]) <= 0.05 * stored[b] + 1e-12, (it, b, dev[b], stored[b])
            assert dev[b] < 1e-5, (it, b, dev[b])
