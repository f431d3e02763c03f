"""Full-covariance GMMs on the GPU (csrc/gmm_full.hip) against float64 under the rule of tests/gmm_full_cases.py: the EM statistics on
both sides of every pad and threshold, centred and at a common offset of 30 sigma with the shift set to it; the scorer with and without a
UBM and loglik_out; non-finite rows; the refusals of the C-ABI; the fit against sklearn's stored iterates; GMM_UBM.GMM end to end.
No test imports sklearn or reads anything outside the repository."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_cases as GC               # noqa: E402
import gmm_full_cases as FC          # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -12345.5


@pytest.fixture(scope="module")
def ssp():
    import torch
    from speech_signal_processing_amd import api, _lib
    return api, _lib, api.default_context(), torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def gold():
    return np.load(FC.GOLDEN)


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:%d" % ctx.device)


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in ("nk", "sx", "sxx", "loglik_sum"))


# ------------------------------------------------------------------------------------------------- EM statistics
@pytest.mark.parametrize("offset", [0.0, 30.0])
@pytest.mark.parametrize("shape", FC.EM_SHAPES, ids=["K%d_D%d_n%d" % s for s in FC.EM_SHAPES])
def test_em_stats_under_the_rule(ssp, shape, offset):
    api, _, ctx, num_cu = ssp
    K, D, n = shape
    c = FC.em_case(K, D, n, offset)
    st = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"], shift=c["shift"])
    res = FC.measure(st, c["ev"], FC.acc_frames(n, K, num_cu), c["name"])
    print("[measured]", res["message"], "max vs emu32 %.3g" % res["max_vs_emu"])
    assert res["worst"] <= 1.0, res["message"]
    assert np.array_equal(st["sxx"], np.transpose(st["sxx"], (0, 2, 1))), "sxx is not exactly symmetric"
    assert _same(st, api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"], shift=c["shift"])), "two calls differ"
    assert _same(st, api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], _dev(ctx, c["X"]), shift=c["shift"])), "host-fed and device-fed differ"


def test_em_stats_past_the_accumulator_cap_and_the_slab_budget(ssp):
    """K = 130, D = 4, n = 125000: 1954 tiles need 16 walkers of at most 128 tiles (the cap; filling the machine asks for 15), and with
    the budget at 1 MB the frames go through 70 slabs of 1792"""
    api, _, ctx, num_cu = ssp
    K, D, n = 130, 4, 125000
    c = FC.em_case(K, D, n, 30.0)
    assert FC.acc_frames(n, K, num_cu) > 64 and FC.slab_frames(n, K, 1) < n
    st = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"], shift=c["shift"])
    res = FC.measure(st, c["ev"], FC.acc_frames(n, K, num_cu), c["name"])
    print("[measured]", res["message"])
    assert res["worst"] <= 1.0, res["message"]
    old = os.environ.get(FC.BUDGET_ENV)
    os.environ[FC.BUDGET_ENV] = "1"
    try:
        st1 = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"], shift=c["shift"])
        st2 = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"], shift=c["shift"])
    finally:
        if old is None:
            del os.environ[FC.BUDGET_ENV]
        else:
            os.environ[FC.BUDGET_ENV] = old
    res = FC.measure(st1, c["ev"], FC.acc_frames(n, K, num_cu, 1), c["name"] + " 1 MB")
    print("[measured]", res["message"])
    assert res["worst"] <= 1.0, res["message"]
    assert _same(st1, st2) and np.array_equal(st1["sxx"], np.transpose(st1["sxx"], (0, 2, 1)))


def test_em_stats_never_reads_below_the_diagonal(ssp):
    api, _, ctx, _ = ssp
    c = FC.em_case(5, 17, 65, 0.0)
    U = c["U"].copy()
    U[:, np.tril_indices(17, -1)[0], np.tril_indices(17, -1)[1]] = np.nan
    assert _same(api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"]), api.gmm_full_em_stats(ctx, c["w"], c["mu"], U, c["X"]))


def test_em_stats_non_finite_rows(ssp):
    api, _, ctx, _ = ssp
    c = FC.em_case(5, 39, 65, 0.0)
    clean = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"])
    for value, where in ((np.nan, (17, 3)), (np.inf, (64, 38)), (-np.inf, (0, 0))):
        X = c["X"].copy()
        X[where] = value
        for feats in (X, _dev(ctx, X)):
            st = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], feats)
            assert np.isnan(st["nk"]).all() and np.isnan(st["sx"]).all() and np.isnan(st["sxx"]).all() and np.isnan(st["loglik_sum"]), value
        assert _same(clean, api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], c["X"])), "a bad call left something behind"


# ------------------------------------------------------------------------------------------------- scorer
SCORER = [(1, False), (3, False), (2, True), (4, True)]   # one and three speaker models, without and with a UBM


@pytest.mark.parametrize("M,ubm", SCORER)
def test_scorer_under_the_rule(ssp, M, ubm):
    api, _, ctx, _ = ssp
    c = FC.scorer_case(M, ubm)
    sc = api.GmmFullScorer(ctx, c["w"], c["mus"], c["Us"], has_ubm=ubm)
    seg = api.Segments.from_lengths(ctx, c["lens"])
    a = sc.score(c["X"], seg, loglik=True)
    b = sc.score(c["X"], seg, loglik=False)
    d = sc.score(_dev(ctx, c["X"]), seg, loglik=True)
    res = FC.compare_loglik(a["loglik"], c["ref_ll"], c["emu_ll"], "loglik M %d" % M)
    print("[measured] scorer M %d ubm %d: %s" % (M, ubm, res))
    GC.compare(a["scores"], c["ref_sc"], c["emu_sc"], "scores")
    GC.compare(b["scores"], c["ref_sc"], c["emu_sc"], "scores without loglik_out")
    tol = GC.entry_tolerance(c["ref_sc"], c["emu_sc"])
    nz = np.asarray(c["lens"]) > 0
    assert (np.abs(np.asarray(a["scores"], np.float64) - b["scores"])[nz] <= 2 * tol[nz]).all()
    assert np.isnan(a["scores"][~nz]).all() and np.isnan(b["scores"][~nz]).all() and (a["argmax"][~nz] == 0).all()
    first = 1 if ubm else 0
    ref_am = (c["ref_sc"][nz][:, first:] - (c["ref_sc"][nz][:, :1] if ubm else 0.0)).argmax(axis=1)
    assert np.array_equal(a["argmax"][nz], ref_am) and np.array_equal(a["argmax"], b["argmax"])
    for k in ("loglik", "scores", "argmax"):
        assert np.array_equal(a[k], d[k].cpu().numpy(), equal_nan=True), "host-fed and device-fed differ: " + k
    r = sc.score_list([c["X"][o:o + n] for o, n in zip(np.concatenate([[0], np.cumsum(c["lens"])[:-1]]), c["lens"])])
    assert np.array_equal(r["scores"], b["scores"], equal_nan=True) and np.array_equal(r["argmax"], b["argmax"])
    sc.close()


def test_scorer_in_runs_of_utterances_gives_the_same_bits(ssp):
    """3 models, 5 utterances of 30000 frames: with the budget at 1 MB (87381 frames of three models) they go in runs of 2, 2 and 1"""
    api, _, ctx, _ = ssp
    rng = np.random.default_rng(9)
    models = [FC.draw_model(rng, 2, 4) for _ in range(3)]
    w, mus, Us = (np.stack([m[i] for m in models]) for i in (0, 1, 3))
    lens = [30000] * 5
    X = rng.standard_normal((sum(lens), 4)).astype(np.float32)
    sc = api.GmmFullScorer(ctx, w, mus, Us, has_ubm=False)
    seg = api.Segments.from_lengths(ctx, lens)
    whole = sc.score(X, seg)
    old = os.environ.get(FC.BUDGET_ENV)
    os.environ[FC.BUDGET_ENV] = "1"
    try:
        runs = sc.score(X, seg)
    finally:
        if old is None:
            del os.environ[FC.BUDGET_ENV]
        else:
            os.environ[FC.BUDGET_ENV] = old
    assert np.isfinite(whole["scores"]).all()
    assert np.array_equal(whole["scores"], runs["scores"]) and np.array_equal(whole["argmax"], runs["argmax"])
    sc.close()


def test_a_zero_weight_mixture_does_not_exist(ssp):
    api, _, ctx, _ = ssp
    c = FC.scorer_case(2, True)
    w = c["w"].copy()
    w[1, 2] = 0.0
    w[1] /= w[1].sum()
    keep = [0, 1, 3, 4]
    seg = api.Segments.from_lengths(ctx, c["lens"])
    a = api.GmmFullScorer(ctx, w[1:], c["mus"][1:], c["Us"][1:], has_ubm=False).score(c["X"], seg, loglik=True)
    b = api.GmmFullScorer(ctx, w[1:, keep], c["mus"][1:, keep], c["Us"][1:, keep], has_ubm=False).score(c["X"], seg, loglik=True)
    assert np.isfinite(a["loglik"]).all() and np.array_equal(a["loglik"], b["loglik"]) and np.array_equal(a["scores"], b["scores"], equal_nan=True)
    # and in the statistics: its mass is 0, the others' sums are the bits of the model without it
    e = FC.em_case(5, 13, 65, 0.0)
    w5 = e["w"].copy()
    w5[2] = 0.0
    w5 /= w5.sum()
    s5 = api.gmm_full_em_stats(ctx, w5, e["mu"], e["U"], e["X"])
    s4 = api.gmm_full_em_stats(ctx, w5[keep], e["mu"][keep], e["U"][keep], e["X"])
    assert s5["nk"][2] == 0.0 and not s5["sxx"][2].any()
    assert np.array_equal(s5["nk"][keep], s4["nk"]) and np.array_equal(s5["sxx"][keep], s4["sxx"]) and s5["loglik_sum"] == s4["loglik_sum"]


def test_score_samples_of_the_golden_models(ssp, gold):
    api, _, ctx, _ = ssp
    for name in FC.FIT_CASES:
        g = FC.golden_fit(gold, name + "_it5")
        Y = gold[name + "_held"]
        sc = api.GmmFullScorer(ctx, g["weights"][None], g["means"][None], g["precisions_cholesky"][None], has_ubm=False)
        got = sc.score(Y, api.Segments.from_lengths(ctx, [len(Y)]), loglik=True, scores=False, argmax=False)["loglik"]
        emu = FC.emu32_loglik(g["weights"][None], g["means"][None], g["precisions_cholesky"][None], Y)
        res = FC.compare_loglik(got, gold[name + "_score_samples"][None], emu, name)
        print("[measured] score_samples %s: %s" % (name, res))
        sc.close()


def test_scorer_non_finite_rows(ssp):
    api, _, ctx, _ = ssp
    lens = [0, 1, 70, 300, 33]
    c = FC.scorer_case(4, True, lens=lens)
    sc = api.GmmFullScorer(ctx, c["w"], c["mus"], c["Us"], has_ubm=True)
    seg = api.Segments.from_lengths(ctx, lens)
    bad = c["X"].copy()
    bad[100, 3] = np.nan      # utterance 3 (frames 71 .. 370)
    bad[100, 7] = np.inf
    bad[372, 0] = -np.inf     # utterance 4
    repaired = bad.copy()
    repaired[100, 3] = repaired[100, 7] = 0.25
    repaired[372, 0] = -0.5
    for loglik in (True, False):
        g = sc.score(bad, seg, loglik=loglik)
        r = sc.score(repaired, seg, loglik=loglik)
        if loglik:
            assert np.isnan(g["loglik"][:, [100, 372]]).all(), "a bad frame must be NaN under every model"
            ok = np.ones(bad.shape[0], bool)
            ok[[100, 372]] = False
            assert np.array_equal(g["loglik"][:, ok], r["loglik"][:, ok]) and np.isfinite(r["loglik"]).all()
        assert np.isnan(g["scores"][[0, 3, 4]]).all() and (g["argmax"][[0, 3, 4]] == 0).all()
        assert np.array_equal(g["scores"][[1, 2]], r["scores"][[1, 2]]) and np.array_equal(g["argmax"][[1, 2]], r["argmax"][[1, 2]])
        assert np.isfinite(r["scores"][1:]).all()
    sc.close()


# ------------------------------------------------------------------------------------------------- validation
def _raw_em(ssp, w, mu, U, X, K=None, D=None):
    """ssp_gmm_full_em_stats through the C-ABI with guard-filled outputs -> (status, outputs untouched)"""
    api, _lib, ctx, _ = ssp
    K = len(w) if K is None else K
    D = X.shape[1] if D is None else D
    w, mu, U = (np.ascontiguousarray(a, dtype=np.float64) for a in (w, mu, U))
    X = np.ascontiguousarray(X, dtype=np.float32)
    n_out = max(len(w), 1) * (X.shape[1] + 1) ** 2
    outs = [np.full(n_out, GUARD) for _ in range(3)]
    ll = C.c_double(GUARD)
    rc = ctx._lib.ssp_gmm_full_em_stats(ctx._h, K, D, w.ctypes.data, mu.ctypes.data, U.ctypes.data, None, X.ctypes.data, X.shape[0],
                                        outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, C.byref(ll), 0, None)
    return rc, all((o == GUARD).all() for o in outs) and ll.value == GUARD


def _bad_models():
    e = FC.em_case(5, 13, 65, 0.0)
    out = {}
    for name, (arr, idx, val) in {"negative weight": ("w", (3,), -0.1), "nan weight": ("w", (3,), np.nan), "inf weight": ("w", (3,), np.inf),
                                  "zero diagonal": ("U", (3, 4, 4), 0.0), "nan diagonal": ("U", (3, 4, 4), np.nan),
                                  "inf diagonal": ("U", (3, 4, 4), np.inf), "negative diagonal": ("U", (3, 4, 4), -1.0),
                                  "nan above the diagonal": ("U", (3, 2, 9), np.nan), "inf mean": ("mu", (3, 5), np.inf)}.items():
        p = {k: e[k].copy() for k in ("w", "mu", "U")}
        p[arr][idx] = val
        out[name] = p
    out["all weights zero"] = dict(w=np.zeros(5), mu=e["mu"], U=e["U"])
    return e, out


def test_invalid_parameters_are_refused_before_anything_runs(ssp):
    api, _lib, ctx, _ = ssp
    e, bad = _bad_models()
    for name, p in bad.items():
        rc, untouched = _raw_em(ssp, p["w"], p["mu"], p["U"], e["X"])
        msg = ctx._lib.ssp_last_error().decode()
        assert rc == _lib.SSP_ERR_INVALID and untouched, (name, rc, msg)
        if name != "all weights zero":
            assert "mix 3" in msg, (name, msg)
        with pytest.raises(ValueError):
            api.GmmFullScorer(ctx, np.stack([e["w"], p["w"]]), np.stack([e["mu"], p["mu"]]), np.stack([e["U"], p["U"]]), has_ubm=False)
        assert "model 1" in ctx._lib.ssp_last_error().decode(), name
    h = C.c_void_p(77)
    p = bad["zero diagonal"]
    w, mu, U = (np.ascontiguousarray(p[k][None], dtype=np.float64) for k in ("w", "mu", "U"))
    assert ctx._lib.ssp_gmm_full_pack(ctx._h, 1, 5, 13, w.ctypes.data, mu.ctypes.data, U.ctypes.data, 0, C.byref(h)) == _lib.SSP_ERR_INVALID
    assert not h.value
    # the ctx stays usable
    assert np.isfinite(api.gmm_full_em_stats(ctx, e["w"], e["mu"], e["U"], e["X"])["loglik_sum"])


def test_unsupported_and_bad_shapes_are_refused(ssp):
    api, _lib, ctx, _ = ssp
    D = 65
    w, mu, U, X = np.ones(1), np.zeros((1, D)), np.eye(D)[None], np.zeros((4, D), np.float32)
    rc, untouched = _raw_em(ssp, w, mu, U, X)
    assert rc == _lib.SSP_ERR_UNSUPPORTED and untouched
    with pytest.raises(NotImplementedError):
        api.GmmFullScorer(ctx, w[None], mu[None], U[None], has_ubm=False)
    e = FC.em_case(5, 13, 65, 0.0)
    for K, Dd in ((0, 13), (5, 0)):
        rc, untouched = _raw_em(ssp, e["w"], e["mu"], e["U"], e["X"], K=K, D=Dd)
        assert rc == _lib.SSP_ERR_INVALID and untouched, (K, Dd)
    rc, untouched = _raw_em(ssp, e["w"], e["mu"], e["U"], e["X"][:0])
    assert rc == _lib.SSP_ERR_INVALID and untouched
    with pytest.raises(ValueError):
        api.GmmFullScorer(ctx, e["w"][None], e["mu"][None], e["U"][None], has_ubm=True)   # a UBM and no speaker model


# ------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("it", [1, 5])
@pytest.mark.parametrize("name", sorted(FC.FIT_CASES))
def test_fit_follows_sklearns_iterates(ssp, gold, name, it):
    """given *_init, tol = 0: every parameter block within 8 d_emu + 1e-6 (|value| + 1) of sklearn's, d_emu the deviation of the same
    loop on the float32 yardstick statistics (tests/golden/make_golden_gmm_full.py; the host file recomputes it)"""
    from speech_signal_processing_amd.gmm_train import GaussianMixture
    api, _, ctx, _ = ssp
    X, w0, mu0, P0 = FC.fit_data(name)
    K = len(w0)
    gm = GaussianMixture(n_components=K, covariance_type="full", tol=0.0, max_iter=it, reg_covar=1e-6, weights_init=w0, means_init=mu0,
                         precisions_init=P0, ctx=ctx).fit(X)
    ref = FC.golden_fit(gold, "%s_it%d" % (name, it))
    d_emu = dict(zip(FC.FIT_BLOCKS, gold["%s_it%d_d_emu" % (name, it)]))
    got = dict(weights=gm.weights_, means=gm.means_, covariances=gm.covariances_, precisions_cholesky=gm.precisions_cholesky_)
    assert gm.n_iter_ == it and gm.covariances_.shape == (K, X.shape[1], X.shape[1])
    for b in FC.FIT_BLOCKS:
        err = np.abs(got[b] - ref[b])
        lim = 8 * d_emu[b] + 1e-6 * (np.abs(ref[b]) + 1)
        print("[measured] fit %s it %d %s: max err %.3g, d_emu %.3g, worst err / limit %.3g" % (name, it, b, err.max(), d_emu[b], (err / lim).max()))
        assert (err <= lim).all(), (name, it, b, float(err.max()), d_emu[b])
    assert np.allclose(gm.precisions_, np.linalg.inv(gm.covariances_), rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("name", sorted(FC.FIT_CASES))
def test_fit_stops_where_sklearn_stops(ssp, gold, name):
    """tol = 1e-3: n_iter_ within one of sklearn's; lower_bound_ within the loglik rule per frame, 8 |mean d| + 2^-22 (|bound| + 1) with
    the yardstick loop's own deviation for |mean d| — plus tol when the two stopped an iteration apart (what one more step may add)"""
    from speech_signal_processing_amd.gmm_train import GaussianMixture
    api, _, ctx, _ = ssp
    X, w0, mu0, P0 = FC.fit_data(name)
    gm = GaussianMixture(n_components=len(w0), covariance_type="full", tol=1e-3, reg_covar=1e-6, weights_init=w0, means_init=mu0,
                         precisions_init=P0, ctx=ctx).fit(X)
    n_ref, lb_ref = int(gold[name + "_tol_n_iter"]), float(gold[name + "_tol_lower_bound"])
    lim = 8 * float(gold[name + "_it5_d_emu_lower"]) + 2.0 ** -22 * (abs(lb_ref) + 1) + (1e-3 if gm.n_iter_ != n_ref else 0.0)
    print("[measured] fit %s tol: n_iter %d (sklearn %d), lower bound off by %.3g (limit %.3g)" % (name, gm.n_iter_, n_ref, abs(gm.lower_bound_ - lb_ref), lim))
    assert gm.converged_ and abs(gm.n_iter_ - n_ref) <= 1
    assert abs(gm.lower_bound_ - lb_ref) <= lim


@pytest.mark.parametrize("init", ["kmeans", "random_from_data"])
def test_fit_from_its_own_start(ssp, init):
    """well-separated data at an offset: the k-means start recovers the generating means to 0.1 sigma; every covariance has a Cholesky
    factor; the object pickles; score_samples / score go through the full scorer and refuse non-finite input"""
    from speech_signal_processing_amd.gmm_train import GaussianMixture, fit_many
    api, _, ctx, _ = ssp
    rng = np.random.default_rng(31)
    K, D, n = 4, 6, 6000
    w, mu, cov, U = FC.draw_model(rng, K, D)
    mu = 12.0 * rng.choice([-1.0, 1.0], (K, D)) * (1 + np.arange(K))[:, None] / K + 40.0
    X = FC.draw_frames(rng, w, mu, cov, n)
    gm = GaussianMixture(n_components=K, covariance_type="full", random_state=0, init_params=init, n_init=1 if init == "kmeans" else 4,
                         ctx=ctx).fit(X)
    for k in range(K):
        np.linalg.cholesky(gm.covariances_[k])
    assert gm.precisions_cholesky_.shape == (K, D, D) and np.allclose(gm.precisions_cholesky_, np.triu(gm.precisions_cholesky_))
    if init == "kmeans":
        sigma = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
        order = [int(np.argmin(((gm.means_ - m) ** 2).sum(axis=1))) for m in mu]
        assert sorted(order) == list(range(K))
        dev = np.abs(gm.means_[order] - mu) / sigma
        print("[measured] k-means start: means off by at most %.3g sigma" % dev.max())
        assert dev.max() <= 0.1
    back = pickle.loads(pickle.dumps(gm))
    ll = back.score_samples(X[:300])
    ref = FC.ref64_loglik(gm.weights_[None], gm.means_[None], gm.precisions_cholesky_[None], X[:300])[0]
    assert np.abs(ll - ref).max() <= 1e-3 and abs(back.score(X[:300]) - ref.mean()) <= 1e-3
    Xb = X[:50].copy()
    Xb[7, 2] = np.nan
    with pytest.raises(ValueError):
        back.score_samples(Xb)
    with pytest.raises(ValueError):
        back.score(Xb)
    with pytest.raises(ValueError):
        GaussianMixture(n_components=K, covariance_type="full", ctx=ctx).fit(Xb)
    if init == "kmeans":
        two = fit_many([X[:3000], X[3000:]], n_components=2, covariance_type="full", random_state=0, ctx=ctx)
        assert len(two) == 2 and all(g.covariances_.shape == (2, D, D) for g in two)


# ------------------------------------------------------------------------------------------------- end to end
def test_orientation_only_speakers_need_full_covariances(ssp, gold):
    """three speakers with the same mean and the same per-axis variances, different covariance orientation: GMM_UBM.GMM with
    covariance_type='full' identifies them, the 'diag' call on the same data stays near chance (1 / 3; at most 0.55 = chance + 3.5
    binomial standard deviations of 60 trials).  sklearn's own models on this set: the golden's orient_acc_full / orient_acc_diag."""
    from speech_signal_processing_amd import GMM_UBM
    assert float(gold["orient_acc_full"]) >= 0.95 and float(gold["orient_acc_diag"]) <= 0.5
    train, x_test, y_test = FC.orientation_set()
    acc = {}
    for kind in ("diag", "full"):
        acc[kind] = GMM_UBM.GMM(train, x_test, y_test, x_test, y_test, n_components=4, random_state=0, covariance_type=kind)[1]
    print("[measured] orientation set: full %.3f, diag %.3f" % (acc["full"], acc["diag"]))
    assert acc["full"] >= 0.9
    assert acc["diag"] <= 0.55
    gmms, ubm = GMM_UBM.GMM.last_model
    with pytest.raises(ValueError):
        GMM_UBM.score_matrix(gmms, ubm, [np.full((5, 16), np.nan, np.float32)])
