"""MAP adaptation and top-C scoring, the parts that need no GPU: the float64 restatement that specifies gmm_train.map_adapt and
api.MapScorer (tests/map_oracle.py, used by tests/test_gmm_map_gpu.py) is held to sklearn, the adaptation formulas to their limits, and
the new entry points, bindings and build unit are declared."""
import os
import re

import numpy as np
import pytest

import map_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ubm(rng, K, D):
    w = rng.dirichlet(5 * np.ones(K))
    mu = rng.standard_normal((K, D))
    cv = rng.uniform(0.5, 1.5, (K, D))
    return w, mu, cv


def _draw(rng, w, mu, cv, n):
    k = rng.choice(len(w), size=n, p=w)
    return mu[k] + np.sqrt(cv[k]) * rng.standard_normal((n, mu.shape[1]))


def _sk(w, mu, cv):
    """a fitted sklearn model with the given parameters"""
    from sklearn.mixture import GaussianMixture
    gm = GaussianMixture(n_components=len(w), covariance_type="diag")
    gm.weights_, gm.means_, gm.covariances_ = w, mu, cv
    gm.precisions_cholesky_ = 1.0 / np.sqrt(cv)
    gm.precisions_ = 1.0 / cv
    gm.converged_, gm.n_iter_, gm.lower_bound_ = True, 1, 0.0
    return gm


@pytest.mark.parametrize("K,D", [(8, 13), (70, 39)])
def test_oracle_responsibilities_are_sklearns(K, D):
    rng = np.random.default_rng(K)
    w, mu, cv = _ubm(rng, K, D)
    X = _draw(rng, w, mu, cv, 300)
    assert np.abs(MO.responsibilities(w, mu, cv, X) - _sk(w, mu, cv).predict_proba(X)).max() <= 1e-12


@pytest.mark.parametrize("adapt", ["m"])
def test_oracle_full_selection_is_the_dense_score_difference(adapt):
    """C = K: diff[u, s] = gm_s.score(X_u) - ubm.score(X_u) of sklearn models built from the adapted means, to 1e-10"""
    rng = np.random.default_rng(5)
    K, D, S = 16, 26, 3
    w, mu, cv = _ubm(rng, K, D)
    ubm = _sk(w, mu, cv)
    means = [MO.map_adapt(w, mu, cv, _draw(rng, w, mu + 0.3 * rng.standard_normal((K, D)), cv, 400), 16.0, adapt)[1] for _ in range(S)]
    lens = [1, 63, 129, 0, 40]
    off = np.concatenate([[0], np.cumsum(lens)])
    X = _draw(rng, w, mu, cv, off[-1])
    r = MO.topc_scores(w, mu, cv, means, X, off, K)
    assert np.isinf(r["gap"]).all()
    for u, n in enumerate(lens):
        if n == 0:
            assert np.isnan(r["diff"][u]).all() and np.isnan(r["ubm"][u])
            continue
        x = X[off[u]:off[u + 1]]
        want = np.array([_sk(w, m, cv).score(x) - ubm.score(x) for m in means])
        assert np.abs(r["diff"][u] - want).max() <= 1e-10
        assert abs(r["ubm"][u] - ubm.score(x)) <= 1e-10


def test_oracle_selection_ranks_and_gap():
    lp = np.array([[0.0, 3.0, 3.0, -1.0, 2.0], [5.0, 5.0, 5.0, 5.0, 5.0]])
    idx, gap = MO.select(lp, 3)
    assert idx.tolist() == [[1, 2, 4], [0, 1, 2]] and gap.tolist() == [2.0, 0.0]
    # an imposed selection is used as given; rows of -1 fall back to the oracle's own
    rng = np.random.default_rng(2)
    w, mu, cv = _ubm(rng, 6, 4)
    X = _draw(rng, w, mu, cv, 5)
    sm = mu[None] + 0.3 * rng.standard_normal((2, 6, 4))
    own = MO.topc_scores(w, mu, cv, sm, X, [0, 5], 2)
    imposed = own["idx"].copy()
    imposed[0] = -1
    imposed[1] = imposed[1][::-1]  # the order inside T(x) does not change a log-sum-exp
    again = MO.topc_scores(w, mu, cv, sm, X, [0, 5], 2, idx=imposed)
    assert np.allclose(again["diff"], own["diff"], rtol=0, atol=1e-13)
    other = own["idx"].copy()
    other[2] = [(own["idx"][2, 0] + 1) % 6, (own["idx"][2, 0] + 2) % 6]
    assert not np.allclose(MO.topc_scores(w, mu, cv, sm, X, [0, 5], 2, idx=other)["frame_diff"][2], own["frame_diff"][2])


def test_adaptation_limits():
    rng = np.random.default_rng(9)
    K, D = 6, 5
    w, mu, cv = _ubm(rng, K, D)
    w = w.copy()
    mu = mu.copy()
    mu[4] += 60.0  # a mixture no frame ever reaches: resp underflows to exactly 0
    X = _draw(rng, np.r_[w[:4], 0, w[5]] / (w.sum() - w[4]), mu, cv, 500)
    nk, sx, sxx = MO.stats(w, mu, cv, X)
    assert nk[4] == 0.0 and (nk[[0, 1, 2, 3, 5]] > 0).all()
    for adapt in ("m", "mw", "mwv"):
        # relevance factor -> infinity: the UBM
        w2, m2, v2 = MO.map_adapt(w, mu, cv, X, np.inf, adapt)
        assert np.array_equal(m2, mu) and np.allclose(w2, w, rtol=0, atol=1e-15) and np.allclose(v2, cv, rtol=0, atol=1e-12)
        w2, m2, v2 = MO.map_adapt(w, mu, cv, X, 1e18, adapt)
        assert np.allclose(m2, mu, rtol=0, atol=1e-12)
        # relevance factor 0: the data's own means wherever a mixture saw data; the empty mixture keeps the UBM's row
        w2, m2, v2 = MO.map_adapt(w, mu, cv, X, 0.0, adapt)
        seen = nk > 0
        assert np.array_equal(m2[seen], (sx / np.where(seen, nk, 1)[:, None])[seen])
        assert np.array_equal(m2[4], mu[4])
        if "v" in adapt:
            assert np.array_equal(v2[4], cv[4]) and (v2 >= 1e-6).all()
        else:
            assert v2 is cv
        if "w" not in adapt:
            assert w2 is w
        else:
            assert abs(w2.sum() - 1.0) <= 1e-15
    # the package's batch arithmetic is the oracle's, speaker by speaker
    from speech_signal_processing_amd.gmm_train import _map_formulas
    Xs = [X[:200], X[200:]]
    st = [MO.stats(w, mu, cv, x) for x in Xs]
    for r in (0.0, 16.0, np.inf):
        wb, mb, vb = _map_formulas(w, mu, cv, np.stack([s[0] for s in st]), np.stack([s[1] for s in st]), np.stack([s[2] for s in st]),
                                   np.array([200, 300]), r, "mwv", 1e-6)
        for i, x in enumerate(Xs):
            w2, m2, v2 = MO.adapt_from_stats(w, mu, cv, *st[i], len(x), r, "mwv")
            assert np.allclose(wb[i], w2, rtol=1e-14, atol=0) and np.allclose(mb[i], m2, rtol=1e-14, atol=1e-14)
            assert np.allclose(vb[i], v2, rtol=1e-12, atol=1e-12)


def test_entry_points_are_declared():
    from speech_signal_processing_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    names = ("ssp_gmm_em_stats_shared", "ssp_gmm_map_pack", "ssp_gmm_map_destroy", "ssp_gmm_map_score", "ssp_gmm_map_score_list")
    for name in names:
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    assert "gmm_map.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gmm_map.hip"))
    assert "GMM_UBM.py:158-170,181-197" in header and "EXTENSION" in header


def test_keywords_and_argument_errors_need_no_gpu():
    import inspect
    from speech_signal_processing_amd import GMM_UBM, api, gmm_train
    sig = inspect.signature(GMM_UBM.GMM).parameters
    assert sig["adapt"].default is None and sig["relevance_factor"].default == 16.0 and sig["top_c"].default is None
    assert inspect.signature(GMM_UBM.score_matrix).parameters["top_c"].default is None
    sig = inspect.signature(gmm_train.map_adapt).parameters
    assert sig["relevance_factor"].default == 16.0 and sig["adapt"].default == "m"
    sig = inspect.signature(api.MapScorer.score).parameters
    assert [sig[k].default for k in ("top_c", "diff", "ubm", "argmax", "idx", "timing")] == [5, True, False, True, False, False]
    rng = np.random.default_rng(0)
    w, mu, cv = _ubm(rng, 4, 3)
    ubm = _sk(w, mu, cv)
    with pytest.raises(ValueError, match="not fitted"):
        gmm_train.map_adapt(gmm_train.GaussianMixture(n_components=4), [np.zeros((5, 3))])
    with pytest.raises(ValueError, match="adapt"):
        gmm_train.map_adapt(ubm, [np.zeros((5, 3))], adapt="")
    with pytest.raises(ValueError, match="adapt"):
        gmm_train.map_adapt(ubm, [np.zeros((5, 3))], adapt="mx")
    with pytest.raises(ValueError, match="features"):
        gmm_train.map_adapt(ubm, [np.zeros((5, 3)), np.zeros((5, 4))])
    # from_sklearn names the first model that is not mean-adapted, before anything touches a device
    good = _sk(w, mu + 0.1, cv)
    other_w = _sk(np.roll(w, 1), mu, cv)
    other_cv = _sk(w, mu, cv * 1.5)
    with pytest.raises(ValueError, match=r"model 1: weights_"):
        api.MapScorer.from_sklearn(None, [good, other_w, other_cv], ubm)
    with pytest.raises(ValueError, match=r"model 0: covariances_"):
        api.MapScorer.from_sklearn(None, [other_cv], ubm)


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a gfx950 device the new surface raises as its neighbours do."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speech_signal_processing_amd import GMM_UBM, _lib, gmm_train
    rng = np.random.default_rng(0)
    w, mu, cv = _ubm(rng, 4, 3)
    ubm = _sk(w, mu, cv)
    X = _draw(rng, w, mu, cv, 50)
    with pytest.raises(_lib.SspError):
        gmm_train.map_adapt(ubm, [X])
    with pytest.raises(_lib.SspError):
        GMM_UBM.score_matrix([_sk(w, mu + 0.1, cv)], ubm, [X], top_c=2)
