"""Batched EM training on the GPU (ssp_gmm_em_stats_batch, gmm_train.fit_many): for K <= 64 every model's statistics and every fitted
model are the bits of the single-model path; K > 64 agrees with the float64 oracle; fit_many reproduces sklearn's per-speaker fits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssp():
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import api
    return pkg, api


def _params(rng, M, K, D, X):
    w = rng.dirichlet(3 * np.ones(K), size=M)
    mu = X.mean(0) + X.std(0) * rng.standard_normal((M, K, D))
    cov = (X.std(0) ** 2) * rng.uniform(0.4, 2.5, (M, K, D))
    return w, mu, cov


def _layout(rng, lens, gap=37):
    """rows of the models placed out of order, with gaps: (n_rows, row_off)"""
    order = rng.permutation(len(lens))
    off = np.zeros(len(lens), np.int64)
    pos = 11
    for m in order:
        off[m] = pos
        pos += lens[m] + gap
    return pos + 5, off


def _stats_case(api, ctx, K, D, seed):
    rng = np.random.default_rng(seed)
    import torch
    cap = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 64 + 1000  # above 2 num_cu tiles: the workgroup count is capped
    lens = [1, 63, 64, 65, 2500, 4097, cap]
    n_rows, off = _layout(rng, lens)
    X = (1.5 * rng.standard_normal((n_rows, D)) + rng.standard_normal(D)).astype(np.float32)
    w, mu, cov = _params(rng, len(lens), K, D, X)
    return X, w, mu, cov, off, np.array(lens, np.int64)


@pytest.mark.parametrize("K", [5, 16, 64])
@pytest.mark.parametrize("D", [7, 26, 39, 47])
def test_batch_stats_bit_identical(ssp, K, D, monkeypatch):
    """every model's nk / sx / sxx / loglik_sum = ssp_gmm_em_stats on its rows, bit for bit: host and device features, and with the
    scratch budget forced small (launch groups)"""
    import torch
    pkg, api = ssp
    ctx = api.default_context()
    X, w, mu, cov, off, lens = _stats_case(api, ctx, K, D, 100 * K + D)
    ref = [api.gmm_em_stats(ctx, w[m], mu[m], cov[m], X[off[m]:off[m] + lens[m]]) for m in range(len(lens))]

    def check(st):
        for m, r in enumerate(ref):
            assert np.array_equal(st["nk"][m], r["nk"]), m
            assert np.array_equal(st["sx"][m], r["sx"]), m
            assert np.array_equal(st["sxx"][m], r["sxx"]), m
            assert st["loglik_sum"][m] == r["loglik_sum"], m

    check(api.gmm_em_stats_batch(ctx, w, mu, cov, X, off, lens))
    check(api.gmm_em_stats_batch(ctx, w, mu, cov, torch.from_numpy(X).cuda(), off, lens))
    monkeypatch.setenv("SSP_EM_BATCH_SCRATCH_MB", "1")  # every model's partials exceed 1 MB at D >= 26: one launch group per model
    check(api.gmm_em_stats_batch(ctx, w, mu, cov, X, off, lens))


@pytest.mark.parametrize("K", [70, 128, 512])
def test_batch_stats_many_chunks(ssp, K):
    """K > 64: the segmented log-sum-exp path vs the float64 oracle (tolerances of test_gmm_em_stats_vs_oracle) and vs the single path"""
    from oracle import ref_cpu as O
    pkg, api = ssp
    ctx = api.default_context()
    D = 39
    rng = np.random.default_rng(K)
    lens = [1, 65, 700, 3001]
    n_rows, off = _layout(rng, lens)
    X = (1.5 * rng.standard_normal((n_rows, D))).astype(np.float32)
    w, mu, cov = _params(rng, len(lens), K, D, X)
    st = api.gmm_em_stats_batch(ctx, w, mu, cov, X, off, np.array(lens))
    for m, n in enumerate(lens):
        x = X[off[m]:off[m] + n]
        nk, sx, sxx, ll = O.gmm_em_stats(w[m], mu[m], cov[m], x.astype(np.float64))
        assert abs(st["loglik_sum"][m] - ll) <= 1e-5 * abs(ll)
        assert np.allclose(st["nk"][m], nk, rtol=1e-4, atol=1e-4 * nk.max())
        assert np.allclose(st["sx"][m], sx, rtol=1e-4, atol=1e-4 * np.abs(sx).max())
        assert np.allclose(st["sxx"][m], sxx, rtol=1e-4, atol=1e-4 * np.abs(sxx).max())
        r = api.gmm_em_stats(ctx, w[m], mu[m], cov[m], x)
        assert abs(st["loglik_sum"][m] - r["loglik_sum"]) <= 1e-5 * abs(r["loglik_sum"])
        for key in ("nk", "sx", "sxx"):
            assert np.allclose(st[key][m], r[key], rtol=1e-5, atol=1e-5 * np.abs(r[key]).max()), (m, key)


def _golden_speakers(g, tag):
    S = int(g[tag + "_cfg"][2])
    return [("%s%d_" % (tag, s)) for s in range(S)]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fit_many_vs_sklearn_golden(golden, ssp, tag):
    """fit_many from the golden's per-speaker inits: per speaker sklearn's n_iter_ / converged_, parameters and lower bound within the
    tolerances of test_gmm_fit_vs_sklearn_golden"""
    from speech_signal_processing_amd.gmm_train import fit_many
    g = golden("gmm_em_batch")
    K, D, S, max_iter, tol = g[tag + "_cfg"]
    ps = _golden_speakers(g, tag)
    gms = fit_many([g[p + "X"] for p in ps], n_components=int(K), tol=float(tol), max_iter=int(max_iter),
                   weights_init=[g[p + "w0"] for p in ps], means_init=[g[p + "mu0"].astype(np.float64) for p in ps],
                   precisions_init=[1.0 / g[p + "cov0"].astype(np.float64) for p in ps])
    assert len(gms) == len(ps)
    for gm, p in zip(gms, ps):
        assert gm.n_iter_ == int(g[p + "niter"]) and gm.converged_ == bool(g[p + "conv"]), p
        assert abs(gm.lower_bound_ - float(g[p + "lb"])) <= 1e-4 * abs(float(g[p + "lb"]))
        assert np.allclose(gm.weights_, g[p + "w"], rtol=1e-4, atol=1e-6)
        assert np.allclose(gm.means_, g[p + "mu"], rtol=1e-4, atol=1e-4)
        assert np.allclose(gm.covariances_, g[p + "cov"], rtol=1e-3, atol=1e-5)


ATTRS = ("weights_", "means_", "covariances_", "precisions_cholesky_", "precisions_", "lower_bound_")


def _same(a, b):
    for k in ATTRS:
        assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
    assert a.n_iter_ == b.n_iter_ and a.converged_ == b.converged_


def _speaker_data(seed, S=5, K=8, D=13):
    rng = np.random.default_rng(seed)
    Xs = []
    for s in range(S):
        centres = 3.0 * rng.standard_normal((K, D))
        n = int(rng.integers(400, 3000))
        Xs.append((centres[rng.integers(0, K, n)] + rng.standard_normal((n, D))).astype(np.float32))
    return Xs


@pytest.mark.parametrize("case", ["kmeans", "random_from_data", "n_init2", "shared_rng"])
def test_fit_many_is_the_loop(ssp, case):
    """fit_many = a loop of GaussianMixture(...).fit, bit for bit, from the default k-means start (int random_state), random_from_data,
    n_init = 2 and a shared RandomState instance (drawn in model order)"""
    from speech_signal_processing_amd.gmm_train import GaussianMixture, fit_many
    Xs = _speaker_data(7)
    kw = {"kmeans": dict(random_state=3), "random_from_data": dict(random_state=4, init_params="random_from_data"),
          "n_init2": dict(random_state=5, n_init=2), "shared_rng": {}}[case]
    kw.update(max_iter=40, tol=1e-4)
    if case == "shared_rng":
        loop = [GaussianMixture(n_components=8, random_state=rs, **kw).fit(X) for rs in [np.random.RandomState(9)] for X in Xs]
        many = fit_many(Xs, n_components=8, random_state=np.random.RandomState(9), **kw)
    else:
        loop = [GaussianMixture(n_components=8, **kw).fit(X) for X in Xs]
        many = fit_many(Xs, n_components=8, **kw)
    for a, b in zip(loop, many):
        _same(a, b)


def test_fit_many_shared_rng_draws_in_model_order(ssp):
    """a RandomState shared by the loop's models is drawn from model after model: fit_many leaves it where the loop leaves it"""
    from speech_signal_processing_amd.gmm_train import GaussianMixture, fit_many
    Xs = _speaker_data(8, S=3)
    r1, r2 = np.random.RandomState(2), np.random.RandomState(2)
    loop = [GaussianMixture(n_components=8, random_state=r1, max_iter=10).fit(X) for X in Xs]
    many = fit_many(Xs, n_components=8, random_state=r2, max_iter=10)
    for a, b in zip(loop, many):
        _same(a, b)
    assert r1.randint(1 << 30) == r2.randint(1 << 30)


def test_gmm_ubm_trains_speakers_in_one_batch(ssp, capsys):
    """GMM_UBM.GMM(model=None): the speaker models are the loop's bit for bit, the UBM is unchanged, and the accuracies too"""
    from speech_signal_processing_amd import GMM_UBM
    from speech_signal_processing_amd.gmm_train import GaussianMixture
    rng = np.random.default_rng(11)
    S, K, D = 4, 8, 26
    centres = [2.0 * rng.standard_normal((K, D)) for _ in range(S)]

    def utt(s, n):
        return centres[s][rng.integers(0, K, n)] + rng.standard_normal((n, D))

    x_train = [utt(s, 300 + 40 * i) for s in range(S) for i in range(3)]
    y_train = [s for s in range(S) for i in range(3)]
    x_test = [utt(s, 250) for s in range(S) for i in range(2)]
    y_test = [s for s in range(S) for i in range(2)]
    train = {}
    for f, lab in zip(x_train, y_train):
        train[lab] = np.vstack((train[lab], f)) if lab in train else f
    acc = GMM_UBM.GMM(train, x_train, y_train, x_test, y_test, n_components=K, model=None, random_state=0)
    printed = capsys.readouterr().out
    gmms, ubm = GMM_UBM.GMM.last_model
    loop = [GaussianMixture(n_components=K, covariance_type='diag', random_state=0).fit(train[s]) for s in sorted(train)]
    for a, b in zip(loop, gmms):
        _same(a, b)
    ubm_ref = GaussianMixture(n_components=K, covariance_type='diag', random_state=0).fit(np.vstack([train[s] for s in sorted(train)]))
    _same(ubm_ref, ubm)
    acc_ref = GMM_UBM.GMM(train, x_train, y_train, x_test, y_test, model=(loop, ubm_ref))
    assert acc == acc_ref
    assert printed == capsys.readouterr().out


def test_batch_errors(ssp):
    pkg, api = ssp
    ctx = api.default_context()
    rng = np.random.default_rng(3)
    K, D = 4, 6
    X = rng.standard_normal((100, D)).astype(np.float32)
    w, mu, cov = _params(rng, 2, K, D, X)
    off, n = np.array([0, 50]), np.array([50, 50])
    with pytest.raises(ValueError):  # shapes
        api.gmm_em_stats_batch(ctx, w[:, :3], mu, cov, X, off, n)
    with pytest.raises(ValueError):
        api.gmm_em_stats_batch(ctx, w, mu, cov, X[:, :5], off, n)
    with pytest.raises(ValueError):
        api.gmm_em_stats_batch(ctx, w, mu, cov, X, off[:1], n)
    with pytest.raises(ValueError, match="model 1"):  # a range past n_rows
        api.gmm_em_stats_batch(ctx, w, mu, cov, X, np.array([0, 60]), n)
    with pytest.raises(ValueError, match="model 0"):  # a zero-length model
        api.gmm_em_stats_batch(ctx, w, mu, cov, X, off, np.array([0, 50]))
    bad = cov.copy()
    bad[1, 2, 3] = -1.0
    with pytest.raises(ValueError, match="model 1"):  # a non-positive covariance
        api.gmm_em_stats_batch(ctx, w, mu, bad, X, off, n)
    with pytest.raises(NotImplementedError):  # D > 47: no batched kernel
        api.gmm_em_stats_batch(ctx, np.ones((1, 1)), np.zeros((1, 1, 48)), np.ones((1, 1, 48)), np.zeros((10, 48), np.float32), [0], [10])
