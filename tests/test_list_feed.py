"""List-fed entry points (ssp_mfcc_run_list, ssp_gmm_score_list; api.mfcc_run_list, GmmScorer.score_list): every result is bit-equal to
the flat path on the concatenation of the same list, in the same process — for every plan family, input and output type, list shape,
slice size and thread count — and the reference-shaped callers routed through them (GMM_UBM.extract_feature, score_matrix) return what
the concatenating recipe returned."""
import ctypes as C
import threading
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssp():
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import api
    return pkg, api


PLANS = {
    "sidekit_cmvn_d1": lambda pkg: pkg.preset_sidekit(fs=16000, delta_order=1, cmvn=1),   # GMM_UBM.extract_feature's plan
    "sidekit_39": lambda pkg: pkg.preset_sidekit(fs=16000, delta_order=2),
    "inrepo": lambda pkg: pkg.preset_inrepo(),
    "librosa_2048": lambda pkg: pkg.preset_librosa(),                                      # the two-pass top_db path
}


def _plan(ssp, name):
    pkg, api = ssp
    return api.MfccPlan(api.default_context(), PLANS[name](pkg))


def _flat(api, plan, sigs, out_dtype):
    flat, lens = api.flatten_signals(sigs)
    seg = api.Segments.from_lengths(plan.ctx, lens)
    fseg = plan.frame_segments(seg)
    return np.asarray(plan.run(flat, seg, fseg), dtype=out_dtype), fseg.offsets


def _check(api, plan, sigs, out_dtype=np.float64):
    want, woff = _flat(api, plan, sigs, out_dtype)
    got, fseg = api.mfcc_run_list(plan, sigs, out_dtype=out_dtype)
    assert got.dtype == np.dtype(out_dtype) and got.shape == want.shape
    assert np.array_equal(fseg.offsets, woff)
    assert np.array_equal(got, want, equal_nan=True)
    return got


def _sigs(rng, lens, dtype):
    if dtype == np.int16:
        return [rng.integers(-8000, 8000, n).astype(np.int16) for n in lens]
    return [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in lens]


@pytest.mark.parametrize("plan_name", list(PLANS))
@pytest.mark.parametrize("in_dtype", [np.float32, np.int16])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64])
def test_ragged_list_equals_flat(ssp, plan_name, in_dtype, out_dtype):
    _, api = ssp
    rng = np.random.default_rng(3)
    sigs = _sigs(rng, [int(v) for v in rng.integers(300, 40000, 37)], in_dtype)
    _check(api, _plan(ssp, plan_name), sigs, out_dtype)


@pytest.mark.parametrize("plan_name", list(PLANS))
def test_list_shapes(ssp, plan_name):
    _, api = ssp
    plan = _plan(ssp, plan_name)
    rng = np.random.default_rng(4)
    short = 1500 if plan.cfg.frame_mode == 2 else 100   # (centred framing needs more than n_fft / 2 samples: the flat path refuses less)
    for dt in (np.float32, np.int16):
        _check(api, plan, _sigs(rng, [16000], dt))                                   # one utterance
        _check(api, plan, _sigs(rng, [0, 5000, short, 12000, 0], dt))                # a zero-length one and a short one (< a frame)
    if plan.cfg.frame_mode == 2:
        with pytest.raises(ValueError):                                              # ... and the flat path's refusal, unchanged
            api.mfcc_run_list(plan, _sigs(rng, [5000, 100], np.int16))
    got, fseg = api.mfcc_run_list(plan, [])                                          # an empty list
    assert got.shape == (0, plan.d_out) and fseg.n == 0


def test_many_slices_reuse_every_ring_slot(ssp, monkeypatch):
    _, api = ssp
    monkeypatch.setenv("SSP_HOST_SLICE_MB", "1")
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(8000, 40000, 90)]
    for name in PLANS:
        plan = _plan(ssp, name)
        for dt in (np.float32, np.int16):
            sigs = _sigs(rng, lens, dt)
            for od in (np.float32, np.float64):
                _check(api, plan, sigs, od)


@pytest.mark.parametrize("threads", ["1", "16"])
def test_thread_counts(ssp, monkeypatch, threads):
    _, api = ssp
    monkeypatch.setenv("SSP_HOST_SLICE_MB", "1")
    monkeypatch.setenv("SSP_HOST_THREADS", threads)
    rng = np.random.default_rng(6)
    lens = [int(v) for v in rng.integers(8000, 40000, 60)]
    plan = _plan(ssp, "sidekit_cmvn_d1")
    _check(api, plan, _sigs(rng, lens, np.int16))                                    # sliced
    _check(api, plan, _sigs(rng, lens[:5], np.float32))                              # one piece


def test_strided_and_mixed_inputs(ssp):
    _, api = ssp
    plan = _plan(ssp, "sidekit_cmvn_d1")
    rng = np.random.default_rng(7)
    base = [rng.integers(-8000, 8000, 2 * n).astype(np.int16) for n in (9000, 17000, 400)]
    strided = [b[::2] for b in base]                                                 # non-contiguous views
    assert not strided[0].flags.c_contiguous
    _check(api, plan, strided)
    col = (0.1 * rng.standard_normal((12000, 2))).astype(np.float32)[:, :1]          # a (n, 1) column of a wider array
    _check(api, plan, [col, strided[1]])
    mixed = [strided[0], (0.3 * rng.standard_normal(7000)).astype(np.float64), strided[2]]  # int16 + float64: the float32 rule
    _check(api, plan, mixed)


def test_2000_utterances_of_3s_take_the_sliced_path(ssp):
    _, api = ssp
    rng = np.random.default_rng(8)
    sigs = [rng.integers(-8000, 8000, 48000).astype(np.int16) for _ in range(2000)]
    assert 48000 * 2000 * 4 >= 2 * (64 << 20)                                        # above two default slices
    plan = _plan(ssp, "sidekit_cmvn_d1")
    _check(api, plan, sigs, np.float64)
    _check(api, plan, sigs, np.float32)


# ----------------------------------------------------------------------------------------- GMM scoring
def _scorer(api, rng, S=10, K=16, D=26):
    w = rng.dirichlet(4 * np.ones(K), size=S + 1)
    mu = 0.6 * rng.standard_normal((S + 1, K, D))
    cov = rng.uniform(0.5, 2.0, (S + 1, K, D))
    return api.GmmScorer(api.default_context(), w, mu, cov, has_ubm=True)


def _rows(rng, n, D=26, lo=50, hi=600, dtype=np.float64):
    return [rng.standard_normal((int(t), D)).astype(dtype) for t in rng.integers(lo, hi, n)]


@pytest.mark.parametrize("precision", [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_score_list_equals_score(ssp, precision, dtype):
    _, api = ssp
    rng = np.random.default_rng(9)
    sc = _scorer(api, rng)
    feats = _rows(rng, 300, dtype=dtype) + [np.zeros((0, 26), dtype)]
    fseg = api.Segments.from_lengths(sc.ctx, [len(f) for f in feats])
    want = sc.score(np.ascontiguousarray(np.vstack(feats), dtype=np.float32), fseg, precision=precision)
    got = sc.score_list(feats, precision=precision)
    assert np.array_equal(got["scores"], want["scores"], equal_nan=True)
    assert np.array_equal(got["argmax"], want["argmax"])


@pytest.mark.parametrize("precision", [0, 2])
def test_score_list_through_the_row_ring(ssp, monkeypatch, precision):
    _, api = ssp
    monkeypatch.setenv("SSP_HOST_SLICE_MB", "1")
    rng = np.random.default_rng(10)
    sc = _scorer(api, rng)
    feats = _rows(rng, 200, lo=200, hi=500)
    assert sum(len(f) for f in feats) * 26 * 4 >= 3 * (1 << 20)                      # above two slices: feed_rows
    fseg = api.Segments.from_lengths(sc.ctx, [len(f) for f in feats])
    want = sc.score(np.ascontiguousarray(np.vstack(feats), dtype=np.float32), fseg, precision=precision)
    got = sc.score_list(feats, precision=precision)
    assert np.array_equal(got["scores"], want["scores"], equal_nan=True)
    assert np.array_equal(got["argmax"], want["argmax"])


# ----------------------------------------------------------------------------------------- routed reference-shaped callers
def test_extract_feature_equals_the_concatenating_recipe(ssp):
    pkg, api = ssp
    from speech_signal_processing_amd import GMM_UBM
    rng = np.random.default_rng(11)
    x = [rng.integers(-8000, 8000, int(n)).astype(np.int16) for n in rng.integers(4000, 48000, 60)]
    y = list(rng.integers(0, 5, len(x)))
    feature, y2 = GMM_UBM.extract_feature(x, y)
    plan = GMM_UBM._feature_plan('MFCC', 16000, 1)
    flat, lens = api.flatten_signals(x)
    seg = api.Segments.from_lengths(plan.ctx, lens)
    fseg = plan.frame_segments(seg)
    feats = np.asarray(plan.run(flat, seg, fseg), dtype=np.float64)
    old = [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(len(lens))]
    assert y2 is y and len(feature) == len(old)
    for a, b in zip(feature, old):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    train, feature3, _ = GMM_UBM.extract_feature(x, y, is_train=True)
    for a, b in zip(feature3, old):
        assert np.array_equal(a, b)


def test_score_matrix_equals_the_stacking_recipe(ssp):
    _, api = ssp
    from speech_signal_processing_amd import GMM_UBM
    rng = np.random.default_rng(12)
    K, D, S = 8, 26, 6

    def gm(seed):
        r = np.random.default_rng(seed)
        return types.SimpleNamespace(covariance_type="diag", weights_=r.dirichlet(4 * np.ones(K)), means_=0.5 * r.standard_normal((K, D)),
                                     covariances_=r.uniform(0.5, 2.0, (K, D)))
    models, ubm = [gm(s) for s in range(S)], gm(99)
    feats = _rows(rng, 120, D=D)
    pred, am = GMM_UBM.score_matrix(models, ubm, feats)
    ctx = api.default_context()
    scorer = api.GmmScorer.from_sklearn(ctx, models, ubm)
    fseg = api.Segments.from_lengths(ctx, [len(f) for f in feats])
    r = scorer.score(np.ascontiguousarray(np.vstack(feats), dtype=np.float32), fseg, scores=True, argmax=True)
    sc = np.asarray(r["scores"], dtype=np.float64)
    assert np.array_equal(pred, sc[:, 1:] - sc[:, :1]) and np.array_equal(am, np.asarray(r["argmax"]).astype(np.int64))
    pred0, am0 = GMM_UBM.score_matrix(models, ubm, [])
    assert pred0.shape == (0, S) and am0.shape == (0,)


# ----------------------------------------------------------------------------------------- error paths
def test_error_paths_leave_the_ctx_working(ssp):
    from speech_signal_processing_amd import _lib
    _, api = ssp
    lib = _lib.load()
    plan = _plan(ssp, "sidekit_cmvn_d1")
    ctx = plan.ctx
    rng = np.random.default_rng(13)
    sigs = _sigs(rng, [9000, 12000], np.int16)
    want, _ = _flat(api, plan, sigs, np.float64)
    table, keep, typ = api.list_table(sigs)
    seg = api.Segments.from_lengths(ctx, [9000, 12000])
    fseg = plan.frame_segments(seg)
    out = np.empty((fseg.total, plan.d_out), np.float64)
    bad_tab = np.array([table[0], 0], dtype=np.uintp)
    seg1 = api.Segments.from_lengths(ctx, [9000])
    seg_off = api.Segments(ctx, np.array([5, 9005, 21005], np.int64))
    run = lib.ssp_mfcc_run_list
    cases = [
        run(plan._h, seg._h, fseg._h, None, 1, out.ctypes.data, 1, 0, None),                     # null table
        run(plan._h, seg._h, fseg._h, bad_tab.ctypes.data, 1, out.ctypes.data, 1, 0, None),      # null pointer, non-empty utterance
        run(plan._h, seg1._h, fseg._h, table.ctypes.data, 1, out.ctypes.data, 1, 0, None),       # counts differ
        run(plan._h, seg_off._h, fseg._h, table.ctypes.data, 1, out.ctypes.data, 1, 0, None),    # segments not at sample 0
        run(plan._h, seg._h, fseg._h, table.ctypes.data, 2, out.ctypes.data, 1, 0, None),        # bad sample type
        run(plan._h, seg._h, fseg._h, table.ctypes.data, 1, out.ctypes.data, 5, 0, None),        # bad out type
        run(None, seg._h, fseg._h, table.ctypes.data, 1, out.ctypes.data, 1, 0, None),           # null plan
    ]
    assert cases == [_lib.SSP_ERR_INVALID] * len(cases)
    assert b"ssp_mfcc_run_list" in lib.ssp_last_error()
    # a zero-length utterance may have a null pointer
    z = np.array([table[0], 0, table[1]], dtype=np.uintp)
    segz = api.Segments.from_lengths(ctx, [9000, 0, 12000])
    fsegz = plan.frame_segments(segz)
    outz = np.empty((fsegz.total, plan.d_out), np.float64)
    assert run(plan._h, segz._h, fsegz._h, z.ctypes.data, 1, outz.ctypes.data, 1, 0, None) == 0
    want_z, _ = _flat(api, plan, [sigs[0], np.zeros(0, np.int16), sigs[1]], np.float64)
    assert np.array_equal(outz, want_z)
    got, _ = api.mfcc_run_list(plan, sigs)
    assert np.array_equal(got, want)

    sc = _scorer(api, rng)
    feats = _rows(rng, 5)
    rt, rkeep, rtyp = api.list_table(feats, "rows")
    gseg = api.Segments.from_lengths(sc.ctx, [len(f) for f in feats])
    s_out, a_out = np.empty((5, sc.n_models), np.float32), np.empty(5, np.int32)
    bad_rows = rt.copy()
    bad_rows[2] = 0
    g = lib.ssp_gmm_score_list
    gcases = [
        g(sc._h, None, 1, sc.D, gseg._h, s_out.ctypes.data, a_out.ctypes.data, 0, None),
        g(sc._h, bad_rows.ctypes.data, 1, sc.D, gseg._h, s_out.ctypes.data, a_out.ctypes.data, 0, None),
        g(sc._h, rt.ctypes.data, 3, sc.D, gseg._h, s_out.ctypes.data, a_out.ctypes.data, 0, None),
        g(sc._h, rt.ctypes.data, 1, 0, gseg._h, s_out.ctypes.data, a_out.ctypes.data, 0, None),
        g(sc._h, rt.ctypes.data, 1, sc.D, gseg._h, s_out.ctypes.data, a_out.ctypes.data, 9, None),
        g(None, rt.ctypes.data, 1, sc.D, gseg._h, s_out.ctypes.data, a_out.ctypes.data, 0, None),
    ]
    assert gcases == [_lib.SSP_ERR_INVALID] * len(gcases)
    want_g = sc.score(np.ascontiguousarray(np.vstack(feats), dtype=np.float32), gseg)
    got_g = sc.score_list(feats)
    assert np.array_equal(got_g["scores"], want_g["scores"]) and np.array_equal(got_g["argmax"], want_g["argmax"])
    with pytest.raises(ValueError):
        sc.score_list([np.zeros((3, sc.D + 1))])


# ----------------------------------------------------------------------------------------- two contexts, two threads
def test_two_contexts_on_two_threads_through_the_list_paths(ssp, monkeypatch):
    pkg, api = ssp
    monkeypatch.setenv("SSP_HOST_SLICE_MB", "1")
    rng = np.random.default_rng(14)
    sigs = _sigs(rng, [int(v) for v in rng.integers(4000, 40000, 80)], np.int16)
    feats_in = _rows(rng, 150)
    S, K, D = 8, 16, 26
    w, mu, cov = rng.dirichlet(4 * np.ones(K), size=S + 1), 0.6 * rng.standard_normal((S + 1, K, D)), rng.uniform(0.5, 2.0, (S + 1, K, D))

    def job(tag, out):
        try:
            ctx = api.Context(0)
            plan = api.MfccPlan(ctx, pkg.preset_sidekit(fs=16000, delta_order=1, cmvn=1))
            sc = api.GmmScorer(ctx, w, mu, cov, has_ubm=True)
            res = []
            for _ in range(3):
                f64, _ = api.mfcc_run_list(plan, sigs)
                f32, _ = api.mfcc_run_list(plan, sigs[:3], out_dtype=np.float32)
                r = sc.score_list(feats_in, precision=1)
                res += [f64, f32, r["scores"], r["argmax"]]
            out[tag] = res
        except Exception as e:  # pragma: no cover
            out[tag] = e

    alone = {}
    job("alone", alone)
    assert not isinstance(alone["alone"], Exception), alone["alone"]
    both = {}
    th = [threading.Thread(target=job, args=(t, both)) for t in ("a", "b")]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for t in ("a", "b"):
        assert not isinstance(both[t], Exception), both[t]
        assert len(both[t]) == len(alone["alone"])
        for x, y in zip(both[t], alone["alone"]):
            assert np.array_equal(x, y, equal_nan=True)
