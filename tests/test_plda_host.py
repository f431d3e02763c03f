"""Host tests of the PLDA back end's restatement (tests/plda_oracle.py) and of the host half of speech_signal_processing_amd/plda.py: the
log-likelihood ratio pinned by brute force on the joint Gaussians of the two-covariance model, the packed form, the diagonalisation, the
EM's monotone objective, plda.em against the oracle's EM, the LDA identities, the ValueError cases, the exclusion share of every scorer
case, and that the header, the bindings and the build declare the feature.  No GPU."""
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_oracle as PO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ssp_plda_stats", "ssp_plda_pack", "ssp_plda_destroy", "ssp_plda_info", "ssp_plda_score")


def _spd(rng, q, scale=1.0):
    M = rng.standard_normal((q, q))
    return scale * (M @ M.T / q + 0.3 * np.eye(q))


def _log_gauss(x, mean, cov):
    d = x - mean
    return -0.5 * (np.linalg.slogdet(cov)[1] + d @ np.linalg.solve(cov, d) + x.size * np.log(2.0 * np.pi))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_llr_equals_the_brute_force_ratio_of_joint_gaussians(n):
    """log p(t, enrol | same speaker) - log p(t) - log p(enrol) from the (n + 1) q-dimensional covariance in the ORIGINAL space: vectors of
    one speaker share y, so their joint covariance has B + W on the diagonal blocks and B off them"""
    q = 3
    rng = np.random.default_rng(40 + n)
    W, B, mu = _spd(rng, q), _spd(rng, q, 2.0), rng.standard_normal(q)
    A, psi = PO.diagonalise(W, B)
    for _ in range(5):
        enrol = mu + rng.standard_normal((n, q)) * 1.5
        t = mu + rng.standard_normal(q) * 1.5

        def joint(k):
            return np.kron(np.ones((k, k)), B) + np.kron(np.eye(k), W)
        both = np.concatenate([t, enrol.reshape(-1)])
        brute = (_log_gauss(both, np.tile(mu, n + 1), joint(n + 1)) - _log_gauss(t, mu, joint(1))
                 - _log_gauss(enrol.reshape(-1), np.tile(mu, n), joint(n)))
        got = PO.llr_direct(psi, (A @ (enrol.mean(axis=0) - mu))[None], [n], (A @ (t - mu))[None])[0, 0]
        assert abs(got - brute) <= 1e-9, (n, got, brute)


@pytest.mark.parametrize("case", PO.SCORER_CASES, ids=lambda c: "q%d-S%d-N%d-G%d-x%g" % c[:5])
def test_packed_form_and_exclusion_share(case):
    g = PO.scorer_case(case)
    beta, alpha, c = PO.pack(g["psi"], g["enrol"], g["counts"])
    packed = PO.llr_packed(beta, alpha, c, g["T"])
    assert np.abs(packed - g["ref"]).max() <= 1e-10 * max(1.0, np.abs(g["ref"]).max())
    assert g["G"] == min(case[3], case[1])
    # alpha depends on the speaker only through its count
    for n in np.unique(g["counts"]):
        rows = alpha[g["counts"] == n]
        assert (rows == rows[0]).all()
    left_out = 1.0 - g["keep"].mean()
    print("[measured] %s: %d of %d rows left out of the arg-max check; fp32 emulation of the packed form: max err %.3g of bound" % (
        case, int((~g["keep"]).sum()), g["keep"].size,
        (np.abs(PO.llr_packed(beta, alpha, c, g["T"], np.float32) - g["ref"]).max(axis=1) / PO.llr_bound(g["ref"])).max()))
    assert left_out <= PO.EXCLUSION_CAP, left_out


def test_scorer_cases_cover_what_the_issue_lists():
    assert {c[0] for c in PO.SCORER_CASES} == {5, 64, 200, 256}
    assert {c[1] for c in PO.SCORER_CASES} == {1, 33, 70}
    assert {c[2] for c in PO.SCORER_CASES} == {1, 129, 300}
    assert {PO.scorer_case(c)["G"] for c in PO.SCORER_CASES} >= {1, 3, 32, 40}
    allc = np.concatenate([PO.scorer_case(c)["counts"] for c in PO.SCORER_CASES])
    assert 1 in allc and 1000 in allc
    assert any(c[4] != 1.0 and c[0] == 5 for c in PO.SCORER_CASES)   # the hard case


def _train_stats(seed=3, q=6, S=12):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((q, q)) / np.sqrt(q) + np.eye(q)
    per = rng.integers(2, 6, S)
    lab = np.repeat(np.arange(S), per)
    y = rng.standard_normal((S, q)) * 2.0
    X = (0.5 + (y[lab] + rng.standard_normal((lab.size, q))) @ M.T).astype(np.float32)
    st = PO.class_stats(X, lab, S)
    return X, lab, st


def test_diagonalisation_identities_and_signs():
    rng = np.random.default_rng(7)
    W, B = _spd(rng, 9), _spd(rng, 9, 3.0)
    A, psi = PO.diagonalise(W, B)
    assert np.abs(A @ W @ A.T - np.eye(9)).max() <= 1e-10
    assert np.abs(A @ B @ A.T - np.diag(psi)).max() <= 1e-10
    assert (np.diff(psi) <= 0).all()
    assert (A[np.arange(9), np.abs(A).argmax(axis=1)] > 0).all()
    from speech_signal_processing_amd import plda
    A2, psi2 = plda.diagonalise(W, B)
    assert np.abs(A2 - A).max() <= 1e-10 and np.abs(psi2 - psi).max() <= 1e-10


def test_em_objective_never_decreases_and_plda_em_reproduces_the_oracle():
    from speech_signal_processing_amd import plda
    _, _, st = _train_stats()
    W, B, obj = PO.em(st["sw"], st["class_mean"], st["count"], st["mean"], 10)
    assert obj.shape == (10,) and (np.diff(obj) >= 0).all(), obj
    assert obj[-1] > obj[0]
    W2, B2, obj2 = plda.em(st["sw"], st["class_mean"], st["count"], st["mean"], 10)
    assert np.abs(W2 - W).max() <= 1e-10 and np.abs(B2 - B).max() <= 1e-10
    assert np.abs(obj2 - obj).max() <= 1e-9 * np.abs(obj).max()
    # the model's host half, fed the oracle's statistics
    m = plda.Plda(n_iter=10)._fit_stats(st)
    assert np.abs(m.within_ - W).max() <= 1e-10 and np.abs(m.between_ - B).max() <= 1e-10
    assert np.abs(m.transform_ @ W @ m.transform_.T - np.eye(W.shape[0])).max() <= 1e-10
    assert np.abs(m.transform_ @ B @ m.transform_.T - np.diag(m.psi_)).max() <= 1e-10


def test_lda_identities():
    from speech_signal_processing_amd import plda
    _, _, st = _train_stats(seed=11)
    p = 4
    V, lam, Sb = PO.lda(st["sw"], st["class_mean"], st["count"], st["mean"], p)
    assert np.abs(V.T @ st["sw"] @ V - np.eye(p)).max() <= 1e-10
    assert np.abs(V.T @ Sb @ V - np.diag(lam)).max() <= 1e-9 * lam.max()
    assert (np.diff(lam) <= 0).all() and (lam > 0).all()
    assert (V[np.abs(V).argmax(axis=0), np.arange(p)] > 0).all()
    fit = plda.Lda(p)._fit_stats(st)
    assert np.abs(fit.components_ - V).max() <= 1e-10 and np.abs(fit.eigenvalues_ - lam).max() <= 1e-9 * lam.max()


def test_value_errors_of_the_host_half():
    from speech_signal_processing_amd import plda
    m = plda.Plda()
    for call in (lambda: m.project(np.zeros((2, 3), np.float32)), lambda: m.save("/nonexistent/x"), lambda: m.enroll(np.zeros((2, 3)), [0, 1], 2),
                 lambda: plda.Lda(2).transform(np.zeros((2, 3), np.float32))):
        with pytest.raises(ValueError, match="not fitted"):
            call()
    _, _, st = _train_stats()
    one = dict(st, count=np.where(np.arange(st["count"].size) == 0, st["count"], 0))
    with pytest.raises(ValueError, match="fewer than two classes"):
        plda.Plda()._fit_stats(one)
    q = st["sw"].shape[0]
    few = {"count": np.array([2, 2, 1]), "sum": np.ones((3, q)), "mean": np.zeros(q), "sw": np.eye(q)}   # N - S = 2 < q
    with pytest.raises(ValueError, match="singular"):
        plda.Plda()._fit_stats(few)
    with pytest.raises(ValueError, match="singular"):
        plda.Lda(2)._fit_stats(few)
    with pytest.raises(ValueError):
        plda.Plda(n_iter=-1)
    with pytest.raises(ValueError):
        plda.Plda(lda_dim=0)
    with pytest.raises(ValueError, match="n_components"):
        plda.Lda(q + 1)._fit_stats(st)


def test_pack_refuses_before_any_gpu_work():
    """every refusal of ssp_plda_pack is answered before the context is touched: a context that holds no device gets it"""
    from speech_signal_processing_amd import _lib, api
    ctx = types.SimpleNamespace(_lib=_lib.load(), _h=None)
    psi, em, cnt = np.array([2.0, 1.0, 0.5]), np.zeros((4, 3)), np.array([1, 2, 2, 7])
    bad = [(np.array([2.0, -1.0, 0.5]), em, cnt), (np.array([2.0, np.nan, 0.5]), em, cnt), (np.array([np.inf, 1.0, 0.5]), em, cnt),
           (psi, em, np.array([1, 0, 2, 7])), (psi, np.where(np.arange(12).reshape(4, 3) == 7, np.inf, 0.0), cnt),
           (psi[:0], em[:, :0], cnt), (psi, em[:0], cnt[:0])]
    for args in bad:
        with pytest.raises(ValueError):
            api.PldaScorer(ctx, *args)
    with pytest.raises(NotImplementedError, match="256"):
        api.PldaScorer(ctx, np.ones(257), np.zeros((2, 257)), np.array([1, 1]))
    with pytest.raises(ValueError, match="expected psi"):
        api.PldaScorer(ctx, psi, np.zeros((4, 2)), cnt)


def test_header_bindings_sources_and_python_surface_declare_the_feature():
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    from speech_signal_processing_amd import _lib, api, build, ivector, plda
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "plda.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "speech_signal_processing_amd", "csrc", "plda.hip"))
    block = header[header.index("PLDA back end"):]
    for word in ("EXTENSION", "UNPINNED", "Ioffe", "Kaldi", "SSP_ERR_UNSUPPORTED", "BIT-IDENTICAL", "class-shared", "tests/plda_oracle.py"):
        assert word in block, word
    assert "no PLDA / WCCN / LDA back end" not in header
    assert "#define SSP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4
    assert hasattr(api, "plda_stats") and hasattr(api, "PldaScorer") and api.PLDA_NO_CLASS_PATH == 1
    for name in ("class_stats", "Lda", "Plda", "em", "diagonalise"):
        assert hasattr(plda, name), name
    for name in ("fit", "project", "enroll", "score", "identify", "save", "load"):
        assert callable(getattr(plda.Plda, name)), name
    import inspect
    sig = inspect.signature(plda.Plda.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("n_iter", 10), ("lda_dim", None), ("length_norm", True), ("ctx", None)]
    assert "Plda(" in ivector.__doc__ and ".enroll(" in ivector.__doc__ and ".identify(" in ivector.__doc__
