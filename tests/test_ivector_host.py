"""i-vector extraction and total-variability training, the parts that need no GPU: the float64 restatement that specifies ssp_ivector_*
(tests/ivector_oracle.py, used by tests/test_ivector_gpu.py) is held to brute-force Gaussian conditioning and to EM's monotonicity, and
the new entry points, bindings, build unit and argument errors are checked."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ivector_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ubm(K=4, D=3, seed=0):
    rng = np.random.default_rng(seed)
    return SimpleNamespace(weights_=rng.dirichlet(5 * np.ones(K)), means_=rng.standard_normal((K, D)), covariances_=rng.uniform(0.5, 2.0, (K, D)))


def test_oracle_posterior_mean_is_gaussian_conditioning():
    """w = L^-1 b equals E[w | y] of the joint Gaussian over (w, stacked per-mixture means), to 1e-10"""
    rng = np.random.default_rng(3)
    K, D, R, U = 6, 4, 5, 4
    mu = rng.standard_normal((K, D))
    cv = rng.uniform(0.5, 2.0, (K, D))
    T = 0.5 * rng.standard_normal((K, D, R))
    nk = rng.uniform(0.5, 30.0, (U, K))
    sx = nk[:, :, None] * (mu[None] + 0.7 * rng.standard_normal((U, K, D)))
    w, logdet, quad, Linv = IO.posterior(mu, cv, T, nk, sx)
    f = IO.centred(mu, nk, sx)
    for u in range(U):
        assert np.abs(w[u] - IO.conditioned_mean(cv, T, nk[u], f[u])).max() <= 1e-10
    # the other outputs, against their definitions written another way
    P, G = IO.precision_terms(cv, T)
    for u in range(U):
        L = np.eye(R) + sum(nk[u, k] * T[k].T @ np.diag(1.0 / cv[k]) @ T[k] for k in range(K))
        assert abs(logdet[u] - np.linalg.slogdet(L)[1]) <= 1e-10
        b = sum(T[k].T @ (f[u, k] / cv[k]) for k in range(K))
        assert abs(quad[u] - b @ np.linalg.solve(L, b)) <= 1e-9 * max(1.0, abs(quad[u]))
        assert np.abs(Linv[u] @ L - np.eye(R)).max() <= 1e-10


@pytest.mark.parametrize("name", ["tiny", "odd", "chunks"])
def test_oracle_em_objective_never_decreases(name):
    c = IO.case(name)
    T, obj = IO.em(c["mu"], c["cv"], c["T0"], c["nk"], c["sx"], 6)
    obj = np.append(obj, IO.objective(c["mu"], c["cv"], T, c["nk"], c["sx"]))
    assert np.isfinite(obj).all()
    assert (np.diff(obj) >= -1e-9 * np.abs(obj[:-1])).all(), obj
    assert obj[-1] > obj[0]
    # the case's T1 is the first of these iterations, and its empty utterances have zero statistics
    assert np.array_equal(IO.em(c["mu"], c["cv"], c["T0"], c["nk"], c["sx"], 1)[0], c["T1"])
    K, D, R, U = c["shape"]
    lens = IO.CASES[name][4]
    for u in range(U):
        if lens[u % len(lens)] == 0:
            assert not c["nk"][u].any() and not c["sx"][u].any()
            assert not c["T1_post"]["w"][u].any() and c["T1_post"]["logdet"][u] == 0.0


def test_package_m_step_is_the_oracles():
    from speech_signal_processing_amd import ivector
    c = IO.case("odd")
    A, C = c["T0_post"]["A"], c["T0_post"]["C"]
    got, want = ivector.m_step(A, C), IO.mstep(A, C)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    A0 = A.copy()
    A0[3] = 0.0
    assert not ivector.m_step(A0, C)[3].any()


def test_entry_points_are_declared():
    from speech_signal_processing_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    names = ("ssp_ivector_create", "ssp_ivector_destroy", "ssp_ivector_set_t", "ssp_ivector_set_workspace", "ssp_ivector_last_slab",
             "ssp_ivector_last_stages", "ssp_ivector_extract", "ssp_ivector_estep")
    for name in names:
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    assert "ivector.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ivector.hip"))
    assert "typedef struct ssp_ivector ssp_ivector;" in header and "UNPINNED" in header and "device-resident statistics are a" in header
    assert _lib.ABI_VERSION == 4  # added without a version step


def test_keywords_and_argument_errors_need_no_gpu(tmp_path):
    import inspect
    from speech_signal_processing_amd import api, ivector
    sig = inspect.signature(ivector.TotalVariability.__init__).parameters
    assert [sig[k].default for k in ("n_iter", "seed", "init_scale", "workspace_bytes", "ctx")] == [10, 0, 0.1, None, None]
    sig = inspect.signature(ivector.TotalVariability.transform).parameters
    assert [sig[k].default for k in ("Xs", "stats", "normalize")] == [None, None, False]
    sig = inspect.signature(api.IvectorExtractor.extract).parameters
    assert [sig[k].default for k in ("logdet", "quad")] == [False, False]
    for rank in (0, -3, 2.5):
        with pytest.raises(ValueError, match="rank"):
            ivector.TotalVariability(rank)
    with pytest.raises(NotImplementedError, match="256"):
        ivector.TotalVariability(257)
    with pytest.raises(NotImplementedError, match="256"):
        api.IvectorExtractor(None, np.zeros((2, 3)), np.ones((2, 3)), np.zeros((2, 3, 257)))
    with pytest.raises(ValueError, match="T \\(K,D,R\\)"):
        api.IvectorExtractor(None, np.zeros((2, 3)), np.ones((2, 3)), np.zeros((2, 4, 5)))
    ubm = _ubm()
    tv = ivector.TotalVariability(2)
    with pytest.raises(ValueError, match="exactly one"):
        tv.fit(ubm)
    with pytest.raises(ValueError, match="exactly one"):
        tv.fit(ubm, Xs=[np.zeros((5, 3))], stats=(np.zeros((1, 4)), np.zeros((1, 4, 3))))
    with pytest.raises(ValueError, match="not fitted"):
        tv.fit(SimpleNamespace(), Xs=[np.zeros((5, 3))])
    with pytest.raises(ValueError, match="not fitted"):
        ivector.baum_welch_stats(SimpleNamespace(weights_=ubm.weights_), [np.zeros((5, 3))])
    with pytest.raises(ValueError, match="features"):
        tv.fit(ubm, Xs=[np.zeros((5, 3)), np.zeros((5, 4))])
    with pytest.raises(ValueError, match="features"):
        ivector.baum_welch_stats(ubm, [np.zeros((5, 4))])
    with pytest.raises(ValueError, match="0 sample"):
        ivector.baum_welch_stats(ubm, [np.zeros((0, 3))])
    with pytest.raises(ValueError, match="statistics"):
        tv.fit(ubm, stats=(np.zeros((2, 4)), np.zeros((2, 4, 5))))
    with pytest.raises(ValueError, match="not fitted"):
        ivector.TotalVariability(2).transform(stats=(np.zeros((1, 4)), np.zeros((1, 4, 3))))
    with pytest.raises(ValueError, match="not fitted"):
        ivector.TotalVariability(2).save(str(tmp_path / "tv.npz"))
    # save / load round trip of a model whose arrays were set by hand
    tv = ivector.TotalVariability(2, n_iter=3, seed=7, init_scale=0.2)
    tv._set_ubm(ubm)
    tv.T_, tv.objective_ = np.arange(24.0).reshape(4, 3, 2), np.array([1.0, 2.0, 3.0])
    tv.save(str(tmp_path / "tv.npz"))
    back = ivector.TotalVariability.load(str(tmp_path / "tv.npz"))
    assert (back.rank, back.n_iter, back.seed, back.init_scale) == (2, 3, 7, 0.2)
    assert np.array_equal(back.T_, tv.T_) and np.array_equal(back.objective_, tv.objective_) and np.array_equal(back.ubm_means_, ubm.means_)


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a gfx950 device the new surface raises as its neighbours do."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speech_signal_processing_amd import _lib, ivector
    c = IO.case("tiny")
    ubm = SimpleNamespace(weights_=c["w"], means_=c["mu"], covariances_=c["cv"])
    with pytest.raises(_lib.SspError):
        ivector.TotalVariability(3, n_iter=1).fit(ubm, stats=(c["nk"], c["sx"]))
    with pytest.raises(_lib.SspError):
        ivector.baum_welch_stats(ubm, [np.zeros((5, 3), dtype=np.float32)])
