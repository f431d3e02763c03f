"""i-vector extraction and total-variability training on the GPU (ssp_ivector_*, api.IvectorExtractor, ivector.TotalVariability) against
the float64 restatement of tests/ivector_oracle.py, on the smallest shapes at which each kernel can go wrong (IO.CASES), with T0 and with
T1 (one float64 EM iteration from T0: L is then conditioned as in use).  The statistics are the oracle's float64 ones, so the scorer's
rounding is not in the measurement.  Bounds: the project's parity metric 1e-4 for w, logdet, quad, A and C (an fp32 emulation of the same
steps gave <= 1.3e-5, the rest is room for the MFMA's summation order), 1e-5 relative for the objective, 1e-3 of max|T| after three
iterations."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import ivector_oracle as IO

pytestmark = pytest.mark.gpu

NAMES = list(IO.CASES)


@pytest.fixture(scope="module")
def ctx():
    from speech_signal_processing_amd import api
    return api.default_context()


def _extractor(ctx, c, tag):
    from speech_signal_processing_amd import api
    return api.IvectorExtractor(ctx, c["mu"], c["cv"], c[tag])


@pytest.mark.parametrize("tag", ["T0", "T1"])
@pytest.mark.parametrize("name", NAMES)
def test_extraction(ctx, name, tag):
    c = IO.case(name)
    want = c[tag + "_post"]
    got = _extractor(ctx, c, tag).extract(c["nk"], c["sx"], logdet=True, quad=True)
    K, D, R, U = c["shape"]
    assert got["w"].shape == (U, R) and got["w"].dtype == np.float32 and got["logdet"].shape == (U,) and got["quad"].shape == (U,)
    ew = np.abs(got["w"] - want["w"]).max(axis=1) / np.maximum(1.0, np.abs(want["w"]).max(axis=1))
    el = np.abs(got["logdet"] - want["logdet"]) / np.maximum(np.abs(want["logdet"]), 1e-30)
    eq = np.abs(got["quad"] - want["quad"]) / np.maximum(np.abs(want["quad"]), 1e-30)
    zero = ~c["nk"].any(axis=1)
    el[zero], eq[zero] = np.abs(got["logdet"][zero]), np.abs(got["quad"][zero])
    print("%s %s: w %.3g  logdet %.3g  quad %.3g" % (name, tag, ew.max(), el.max(), eq.max()))
    assert ew.max() <= 1e-4 and el.max() <= 1e-4 and eq.max() <= 1e-4
    # an utterance without frames: exact zeros
    for u in np.nonzero(zero)[0]:
        assert not got["w"][u].any() and got["logdet"][u] == 0.0 and got["quad"][u] == 0.0
    # without the optional outputs the call returns the array alone, same bits
    assert np.array_equal(_extractor(ctx, c, tag).extract(c["nk"], c["sx"]), got["w"])


@pytest.mark.parametrize("tag", ["T0", "T1"])
@pytest.mark.parametrize("name", NAMES)
def test_estep(ctx, name, tag):
    c = IO.case(name)
    want = c[tag + "_post"]
    ext = _extractor(ctx, c, tag)
    got = ext.estep(c["nk"], c["sx"])
    K, D, R, U = c["shape"]
    assert got["A"].shape == (K, R, R) and got["C"].shape == (K, D, R) and got["A"].dtype == np.float64
    ea = np.abs(got["A"] - want["A"]).max() / np.abs(want["A"]).max()
    ec = np.abs(got["C"] - want["C"]).max() / np.abs(want["C"]).max()
    eo = abs(got["objective"] - want["objective"]) / abs(want["objective"])
    print("%s %s: A %.3g  C %.3g  objective %.3g" % (name, tag, ea, ec, eo))
    assert ea <= 1e-4 and ec <= 1e-4 and eo <= 1e-5
    assert np.array_equal(got["A"], got["A"].transpose(0, 2, 1))
    # the same call again: the same bits (no atomics, every sum has a fixed shape)
    again = ext.estep(c["nk"], c["sx"])
    assert np.array_equal(again["A"], got["A"]) and np.array_equal(again["C"], got["C"]) and again["objective"] == got["objective"]


def test_training_follows_the_float64_iterations(ctx):
    from speech_signal_processing_amd import ivector
    c = IO.case("odd")
    K, D, R, U = c["shape"]
    ubm = SimpleNamespace(weights_=c["w"], means_=c["mu"], covariances_=c["cv"])
    tv = ivector.TotalVariability(rank=R, n_iter=3, seed=5, init_scale=0.1, ctx=ctx).fit(ubm, stats=(c["nk"], c["sx"]))
    want, want_obj = IO.em(c["mu"], c["cv"], c["T0"], c["nk"], c["sx"], 3)
    et = np.abs(tv.T_ - want).max() / np.abs(want).max()
    print("T after 3 iterations: %.3g   objective %s (oracle %s)" % (et, tv.objective_, want_obj))
    assert tv.T_.shape == (K, D, R) and tv.objective_.shape == (3,)
    assert et <= 1e-3
    assert (np.diff(tv.objective_) >= -1e-6 * np.abs(tv.objective_[:-1])).all()
    # transform from the same statistics: the i-vectors under T_
    w = tv.transform(stats=(c["nk"], c["sx"]))
    ref = IO.posterior(c["mu"], c["cv"], tv.T_, c["nk"], c["sx"])[0]
    assert (np.abs(w - ref).max(axis=1) <= 1e-4 * np.maximum(1.0, np.abs(ref).max(axis=1))).all()


@pytest.mark.parametrize("name", ["odd", "chunks"])
def test_slabs_and_position_do_not_change_an_utterance(ctx, name):
    c = IO.case(name)
    K, D, R, U = c["shape"]
    ext = _extractor(ctx, c, "T1")
    one = ext.extract(c["nk"], c["sx"], logdet=True, quad=True)
    assert ext.last_slab == U
    per_utt = 4 * (R * (R + 1) // 2 + K + K * D + 2 * R)
    ext.set_workspace(per_utt * (U // 3))  # at least three slabs
    cut = ext.extract(c["nk"], c["sx"], logdet=True, quad=True)
    assert 1 <= ext.last_slab <= U // 3
    ext.set_workspace(0)  # one utterance always runs
    single = ext.extract(c["nk"], c["sx"], logdet=True, quad=True)
    assert ext.last_slab == 1
    for k in ("w", "logdet", "quad"):
        assert np.array_equal(cut[k], one[k]) and np.array_equal(single[k], one[k]), k
    # the E-step under slabs: float64 sums of the slabs' accumulators, still within the bound and the same bits every time
    a = ext.estep(c["nk"], c["sx"])
    b = ext.estep(c["nk"], c["sx"])
    want = c["T1_post"]
    assert np.array_equal(a["A"], b["A"]) and np.array_equal(a["C"], b["C"])
    assert np.abs(a["A"] - want["A"]).max() <= 1e-4 * np.abs(want["A"]).max() and np.abs(a["C"] - want["C"]).max() <= 1e-4 * np.abs(want["C"]).max()
    ext.set_workspace(1 << 30)
    # utterance 0 alone, and at another place of a shuffled batch
    alone = ext.extract(c["nk"][:1], c["sx"][:1], logdet=True, quad=True)
    perm = np.roll(np.arange(U), 5)
    moved = ext.extract(c["nk"][perm], c["sx"][perm], logdet=True, quad=True)
    for k in ("w", "logdet", "quad"):
        assert np.array_equal(alone[k][0], one[k][0]), k
        assert np.array_equal(moved[k], one[k][perm]), k


def test_a_non_finite_utterance_is_answered_alone(ctx):
    c = IO.case("odd")
    ext = _extractor(ctx, c, "T1")
    bad, zeroed = 4, c["sx"].copy()
    zeroed[bad] = 0.0
    nkz = c["nk"].copy()
    nkz[bad] = 0.0
    want = ext.extract(nkz, zeroed, logdet=True, quad=True)
    for value in (np.nan, np.inf):
        sx = c["sx"].copy()
        sx[bad, 3, 2] = value
        with pytest.raises(ValueError, match="utterance %d" % bad):
            ext.extract(c["nk"], sx)
        with pytest.raises(ValueError, match="utterance %d" % bad):
            ext.estep(c["nk"], sx)
        got = ext.extract(c["nk"], sx, logdet=True, quad=True, check=False)
        assert np.isnan(got["w"][bad]).all() and np.isnan(got["logdet"][bad]) and np.isnan(got["quad"][bad])
        keep = np.arange(len(sx)) != bad
        for k in ("w", "logdet", "quad"):
            assert np.array_equal(got[k][keep], want[k][keep]), k
        r = ext.estep(c["nk"], sx, check=False)
        assert np.isnan(r["A"]).all() and np.isnan(r["C"]).all() and np.isnan(r["objective"])
    nk = c["nk"].copy()
    nk[bad, 0] = np.nan
    got = ext.extract(nk, c["sx"], check=False)
    assert np.isnan(got[bad]).all() and np.array_equal(got[keep], want["w"][keep])


def test_argument_errors_leave_the_ctx_usable(ctx):
    from speech_signal_processing_amd import _lib, api
    lib = _lib.load()
    c = IO.case("rank1")
    K, D, R, U = c["shape"]
    mu, cv = np.ascontiguousarray(c["mu"]), np.ascontiguousarray(c["cv"])
    h = C.c_void_p()
    T = np.zeros((K, D, 257))
    assert lib.ssp_ivector_create(ctx._h, K, D, 257, mu.ctypes.data, cv.ctypes.data, T.ctypes.data, C.byref(h)) == _lib.SSP_ERR_UNSUPPORTED
    assert not h.value
    for k, d, r in ((0, D, 1), (K, 0, 1), (K, D, 0)):
        assert lib.ssp_ivector_create(ctx._h, k, d, r, mu.ctypes.data, cv.ctypes.data, T.ctypes.data, C.byref(h)) == _lib.SSP_ERR_INVALID
    for arr, at, value in ((cv, (1, 2), 0.0), (cv, (1, 2), -1.0), (cv, (1, 2), np.inf), (mu, (0, 0), np.nan)):
        broken = arr.copy()
        broken[at] = value
        with pytest.raises(ValueError, match="covariance|mean"):
            api.IvectorExtractor(ctx, broken if arr is mu else mu, broken if arr is cv else cv, c["T0"])
    Tn = c["T0"].copy()
    Tn[2, 1, 0] = np.nan
    with pytest.raises(ValueError, match="T"):
        api.IvectorExtractor(ctx, mu, cv, Tn)
    ext = _extractor(ctx, c, "T0")
    with pytest.raises(ValueError, match="T"):
        ext.set_T(Tn)
    with pytest.raises(ValueError, match="at least one"):
        ext.extract(c["nk"][:0], c["sx"][:0])
    assert lib.ssp_ivector_extract(ext._h, c["nk"].ctypes.data, c["sx"].ctypes.data, 0, None, None, None, None) == _lib.SSP_ERR_INVALID
    # the handle kept its T and the ctx works
    w = ext.extract(c["nk"], c["sx"])
    assert np.abs(w - c["T0_post"]["w"]).max() <= 1e-4 * max(1.0, np.abs(c["T0_post"]["w"]).max())


def test_end_to_end_from_features(ctx):
    """S = 4 speakers with a fixed w_true each, K = 16, D = 13, R = 8, six utterances of 200 frames per speaker: baum_welch_stats ->
    fit(n_iter=5) -> transform(normalize=True) -> centroids from three utterances per speaker -> d_vector.identify on the other three.
    Seed 0 of the recipe: the float64 oracle pipeline alone identifies all twelve with a top-2 cosine margin of 0.185 (>= 0.05 asked)."""
    from speech_signal_processing_amd import api, d_vector, ivector
    o = IO.end_to_end(0)
    lab, enrol = o["labels"], o["is_enrol"]
    assert (o["pred"] == lab[~enrol]).all() and o["margin"].min() >= 0.05
    r = o["recipe"]
    ubm = SimpleNamespace(weights_=r["w"], means_=r["mu"], covariances_=r["cv"])
    Xs = [X.astype(np.float32) for X in r["Xs"]]
    nk, sx = ivector.baum_welch_stats(ubm, Xs, ctx=ctx)
    onk, osx = IO.stats(r["w"], r["mu"], r["cv"], [X.astype(np.float64) for X in Xs])
    assert np.abs(nk - onk).max() <= 1e-3 * onk.max()
    tv = ivector.TotalVariability(rank=8, n_iter=5, seed=5, ctx=ctx).fit(ubm, stats=(nk, sx))
    assert (np.diff(tv.objective_) >= -1e-6 * np.abs(tv.objective_[:-1])).all()
    E = tv.transform(Xs, normalize=True)
    assert E.shape == (24, 8) and E.dtype == np.float32 and np.abs(np.linalg.norm(E, axis=1) - 1.0).max() <= 1e-5
    cent = np.asarray(api.centroids(ctx, E[enrol], lab[enrol].astype(np.int32), 4))
    who = d_vector.identify(E[~enrol], cent)
    print("identified", who, "truth", lab[~enrol])
    assert np.array_equal(who, lab[~enrol])
