"""Non-finite feature rows through GMM scoring and EM training: the yardstick itself, and the parts of the Python layer that need no GPU.

The sidekit front end hands a digitally silent frame on as a NaN row on purpose; include/ssp.h (ssp_gmm_score, ssp_gmm_em_stats) says what
the scorer and the EM kernels do with one.  tests/test_gmm_nonfinite_gpu.py holds the kernels to that against oracle.ref_cpu — so here the
oracle is held to what it is taken for (a bad frame is NaN under the model, every other frame is untouched, the EM sums are non-finite),
and sklearn, the reference these stand in for, to what the Python layer copies from it: ValueError from its input validation."""
import numpy as np
import pytest

from oracle import ref_cpu as O

BAD_VALUES = [np.nan, np.inf, -np.inf]
K, D, T = 5, 7, 40


def _model(seed=0):
    rng = np.random.default_rng(seed)
    return rng.dirichlet(5 * np.ones(K)), rng.standard_normal((K, D)), rng.uniform(0.5, 2.0, (K, D))


def _frames(seed=1):
    return np.random.default_rng(seed).standard_normal((T, D))


@pytest.mark.parametrize("bad", BAD_VALUES, ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("col", range(D))
@pytest.mark.parametrize("row", [0, 17, T - 1])
def test_oracle_score_samples_bad_frame_is_nan_and_the_rest_is_untouched(bad, col, row):
    w, mu, cov = _model()
    X = _frames()
    clean = O.gmm_score_samples(w, mu, cov, X)
    assert np.isfinite(clean).all()
    Xb = X.copy()
    Xb[row, col] = bad
    with np.errstate(all="ignore"):
        got = O.gmm_score_samples(w, mu, cov, Xb)
        score = O.gmm_score(w, mu, cov, Xb)
    assert np.isnan(got[row]), (bad, col, row, got[row])  # NaN, not -inf: inf - inf in the quadratic form or against the running maximum
    keep = np.arange(T) != row
    assert np.array_equal(got[keep], clean[keep])         # bit for bit: the frames are independent
    assert np.isnan(score)


@pytest.mark.parametrize("bad", BAD_VALUES, ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("col", [0, D // 2, D - 1])
def test_oracle_em_stats_are_all_non_finite(bad, col):
    w, mu, cov = _model()
    Xb = _frames()
    Xb[11, col] = bad
    with np.errstate(all="ignore"):
        nk, sx, sxx, ll = O.gmm_em_stats(w, mu, cov, Xb)
    assert not np.isfinite(nk).any() and not np.isfinite(sx).any() and not np.isfinite(sxx).any() and not np.isfinite(ll)


@pytest.mark.parametrize("bad", BAD_VALUES, ids=["nan", "+inf", "-inf"])
def test_sklearn_raises_value_error_at_fit_score_and_score_samples(bad):
    from sklearn import mixture
    w, mu, cov = _model()
    X = _frames()
    gm = mixture.GaussianMixture(n_components=K, covariance_type="diag", weights_init=w, means_init=mu, precisions_init=1.0 / cov,
                                 max_iter=2, random_state=0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(X)
    assert np.isfinite(gm.score(X)) and np.isfinite(gm.score_samples(X)).all()
    Xb = X.copy()
    Xb[3, 2] = bad
    fresh = mixture.GaussianMixture(n_components=K, covariance_type="diag", random_state=0)
    with pytest.raises(ValueError):
        fresh.fit(Xb)
    assert not hasattr(fresh, "weights_")
    with pytest.raises(ValueError):
        gm.score(Xb)
    with pytest.raises(ValueError):
        gm.score_samples(Xb)


# ------------------------------------------------------------------------------------------------- the Python layer, no GPU
class _FakeScorer:
    """stands in for api.GmmScorer: a fixed (U, M) score matrix, as ssp_gmm_score_list would leave it"""

    def __init__(self, scores):
        self.scores = np.asarray(scores, dtype=np.float32)
        self.calls = 0

    def score_list(self, feats, precision=0, timing=False):
        self.calls += 1
        sc = self.scores
        with np.errstate(all="ignore"):
            am = np.array([0 if np.isnan(r).all() else int(np.nanargmax(r[1:] - r[0])) for r in sc], dtype=np.int32)
        return {"scores": sc, "argmax": am}


def _patched_score_matrix(monkeypatch, scores):
    from speech_signal_processing_amd import GMM_UBM, api
    fake = _FakeScorer(scores)
    monkeypatch.setattr(api, "default_context", lambda *a, **k: object())
    monkeypatch.setattr(api.GmmScorer, "from_sklearn", classmethod(lambda cls, ctx, models, ubm=None: fake))
    return GMM_UBM, fake


def test_score_matrix_raises_on_a_nan_row_with_frames_and_names_the_utterance(monkeypatch):
    sc = np.array([[-40.0, -39.0, -41.0], [np.nan] * 3, [-38.0, -38.5, -37.0], [np.nan] * 3], dtype=np.float32)
    GMM_UBM, fake = _patched_score_matrix(monkeypatch, sc)
    feats = [np.zeros((5, 4)), np.zeros((0, 4)), np.zeros((3, 4)), np.zeros((2, 4))]   # utterance 1 is empty, utterance 3 is bad
    with pytest.raises(ValueError, match=r"utterance 3\b"):
        GMM_UBM.score_matrix([None, None], None, feats)
    assert fake.calls == 1   # decided from the one scoring call's result
    for fn, arg in ((GMM_UBM.identify_language, feats), (GMM_UBM.identify_with_confidence, feats[3])):
        if fn is GMM_UBM.identify_with_confidence:
            fake.scores = sc[3:4]
        with pytest.raises(ValueError, match="utterance"):
            fn([None, None], None, arg)


def test_score_matrix_keeps_an_empty_utterances_nan_row(monkeypatch):
    sc = np.array([[-40.0, -39.0, -41.0], [np.nan] * 3, [-38.0, -38.5, -37.0]], dtype=np.float32)
    GMM_UBM, _ = _patched_score_matrix(monkeypatch, sc)
    pred, am = GMM_UBM.score_matrix([None, None], None, [np.zeros((5, 4)), np.zeros((0, 4)), np.zeros((3, 4))])
    assert np.isnan(pred[1]).all() and am[1] == 0
    assert np.array_equal(am, [0, 0, 1]) and np.isfinite(pred[[0, 2]]).all()


def test_score_matrix_raises_on_an_infinite_score(monkeypatch):
    sc = np.array([[-40.0, -39.0, -41.0], [-40.0, -np.inf, -41.0]], dtype=np.float32)
    GMM_UBM, _ = _patched_score_matrix(monkeypatch, sc)
    with pytest.raises(ValueError, match=r"utterance 1\b"):
        GMM_UBM.score_matrix([None, None], None, [np.zeros((5, 4)), np.zeros((2, 4))])


@pytest.mark.parametrize("bad", BAD_VALUES, ids=["nan", "+inf", "-inf"])
def test_fit_raises_before_any_kernel_runs_and_sets_no_attribute(bad):
    """fit looks at the matrix that sits on the device with one reduction, before the first E step: a tensor that is already a torch
    tensor is taken as it is, so the look itself can be watched here without a GPU (the context is never touched before it)."""
    import torch
    from speech_signal_processing_amd import gmm_train

    class NoCtx:
        def __getattr__(self, name):
            raise AssertionError("the context was used (%s) before the input was validated" % name)
    X = _frames().astype(np.float32)
    X[23, D - 1] = bad
    gm = gmm_train.GaussianMixture(n_components=K, ctx=NoCtx())
    with pytest.raises(ValueError, match=r"row 23\b"):
        gm.fit(torch.from_numpy(X))
    assert not hasattr(gm, "weights_") and not hasattr(gm, "converged_")


def test_first_bad_row_finds_the_first_and_only_then_looks_it_up():
    import torch
    from speech_signal_processing_amd import gmm_train
    X = torch.zeros((50, 3))
    assert gmm_train._first_bad_row(X) is None
    X[41, 0] = float("inf")
    X[17, 2] = float("nan")
    assert gmm_train._first_bad_row(X) == 17
