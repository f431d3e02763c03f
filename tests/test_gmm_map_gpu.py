"""GPU tests of MAP-adapted GMM-UBM models and the top-C fast scorer (run with -m gpu on an MI355X): ssp_gmm_em_stats_shared,
gmm_train.map_adapt, api.MapScorer / ssp_gmm_map_*, and their GMM_UBM surface, against the float64 restatement tests/map_oracle.py.

Shapes: the smallest at which the kernels can go wrong.  K 8 / 64 / 70 / 512 (one chunk, exactly one, a padded second, eight);
D 13 / 26 / 39 / 47; C 1 / 5 / 8; S 1 / 3 / 65 (65 crosses a 64-speaker tile); ragged utterances of 1, 63, 64, 65, 129, 298 frames (one and
two scoring blocks, a part block) and an empty one, about 2500 frames.  Inputs as the scorer's accuracy note in include/ssp.h asks
(|mu| / sigma about 1): UBM means N(0, 1), variances in [0.5, 1.5], Dirichlet(5) weights, speaker means the UBM's plus
0.3 N(0, 1), the frames of utterance u drawn from the model of speaker u mod S (so that the top-2 margins are clear ones).  The oracle of a case is computed once and shared by the tests of that case."""
import ctypes as C

import numpy as np
import pytest

import map_oracle as MO

pytestmark = pytest.mark.gpu

LENS = [1, 63, 64, 65, 129, 298, 0, 298, 200, 130, 77, 298, 256, 128, 300, 191]
#        K   D  C   S
CASES = [(8, 13, 8, 1), (64, 26, 5, 3), (70, 39, 1, 65), (512, 47, 8, 3), (512, 39, 5, 65)]
GAP = 1e-3          # nats: selections and arg-max are held exact above it (the fp32 expanded form errs by 4.1e-5 nats at most on these inputs)
ATOL, RTOL = 2e-4, 1e-4
_CASE = {}


@pytest.fixture(scope="module")
def env():
    from speech_signal_processing_amd import api, _lib
    return api, _lib, api.default_context()


def make_inputs(K, D, S, seed, lens=LENS):
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(5 * np.ones(K))
    mu = rng.standard_normal((K, D))
    cv = rng.uniform(0.5, 1.5, (K, D))
    sm = mu[None] + 0.3 * rng.standard_normal((S, K, D))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    k = rng.choice(K, size=int(off[-1]), p=w)
    who = np.repeat(np.arange(len(lens)) % S, lens)   # utterance u is spoken by speaker u mod S: its top-2 margin is a clear one
    X = (sm[who, k] + np.sqrt(cv[k]) * rng.standard_normal((int(off[-1]), D))).astype(np.float32)
    return {"w": w, "mu": mu, "cv": cv, "sm": sm, "off": off, "X": X, "lens": list(lens)}


def case(env, K, D, Ck, S):
    """inputs, the device's answer (one call, every output) and the oracle of one case, computed once"""
    key = (K, D, Ck, S)
    if key not in _CASE:
        api, _lib, ctx = env
        g = make_inputs(K, D, S, 1000 * K + 10 * D + S)
        sc = api.MapScorer(ctx, g["w"], g["mu"], g["cv"], g["sm"])
        seg = api.Segments.from_lengths(ctx, g["lens"])
        g["got"] = sc.score(g["X"], seg, top_c=Ck, diff=True, ubm=True, argmax=True, idx=True)
        g["own"] = MO.topc_scores(g["w"], g["mu"], g["cv"], g["sm"], g["X"], g["off"], Ck)                      # the oracle's own selection
        g["ref"] = MO.topc_scores(g["w"], g["mu"], g["cv"], g["sm"], g["X"], g["off"], Ck, idx=g["got"]["idx"])  # ... and the device's imposed
        g["sc"], g["seg"] = sc, seg
        _CASE[key] = g
    return _CASE[key]


def ids(cases):
    return ["K%d-D%d-C%d-S%d" % c for c in cases]


# ===================================================================================================== 1. shared statistics
@pytest.mark.parametrize("K", [64, 512])
def test_shared_stats_are_the_batch_calls_bits(env, K):
    """ssp_gmm_em_stats_shared = ssp_gmm_em_stats_batch with the parameters repeated, bit for bit (K = 64: the fused kernel, K = 512: the
    log-sum-exp pass + eight chunks): M = 3 ragged ranges out of order, two of them overlapping, host and device features; a poisoned
    speaker turns only its own outputs NaN."""
    import torch
    api, _lib, ctx = env
    rng = np.random.default_rng(K)
    D = 39
    g = make_inputs(K, D, 1, 7 + K, lens=[1100])
    X, w, mu, cv = g["X"], g["w"], g["mu"], g["cv"]
    off, cnt = np.array([400, 3, 350], np.int64), np.array([65, 300, 700], np.int64)   # rows [350, 1050) hold [400, 465)
    rep = api.gmm_em_stats_batch(ctx, np.stack([w] * 3), np.stack([mu] * 3), np.stack([cv] * 3), X, off, cnt)
    for feats in (X, torch.from_numpy(X).cuda()):
        st = api.gmm_em_stats_shared(ctx, w, mu, cv, feats, off, cnt)
        for key in ("nk", "sx", "sxx", "loglik_sum"):
            assert st[key].shape == rep[key].shape and np.array_equal(st[key], rep[key]), key
    assert np.isfinite(rep["nk"]).all() and np.allclose(rep["nk"].sum(1), cnt, rtol=1e-4)
    bad = X.copy()
    bad[100, 5] = np.nan   # inside speaker 1's rows [3, 303) only
    st = api.gmm_em_stats_shared(ctx, w, mu, cv, bad, off, cnt)
    for key in ("nk", "sx", "sxx", "loglik_sum"):
        assert np.isnan(st[key][1]).all(), key
        assert np.array_equal(st[key][[0, 2]], rep[key][[0, 2]]), key
    again = api.gmm_em_stats_shared(ctx, w, mu, cv, X, off, cnt)   # nothing of the NaNs stays behind
    assert all(np.array_equal(again[key], rep[key]) for key in rep)
    with pytest.raises(ValueError, match="ssp_gmm_em_stats_shared: model 2"):
        api.gmm_em_stats_shared(ctx, w, mu, cv, X, off, np.array([65, 300, 900]))
    with pytest.raises(NotImplementedError):
        api.gmm_em_stats_shared(ctx, np.ones(1), np.zeros((1, 48)), np.ones((1, 48)), np.zeros((10, 48), np.float32), [0], [10])


# ===================================================================================================== 2. map_adapt
class _Model:
    """a fitted model as sklearn pickles it, for the surface calls"""
    covariance_type = "diag"
    reg_covar = 1e-6

    def __init__(self, w, mu, cv):
        self.weights_, self.means_, self.covariances_ = w, mu, cv
        self.precisions_cholesky_ = 1.0 / np.sqrt(cv)
        self.precisions_ = 1.0 / cv


@pytest.mark.parametrize("adapt", ["m", "mw", "mwv"])
def test_map_adapt_against_the_oracle(env, adapt):
    """gmm_train.map_adapt = the oracle's formulas on the oracle's statistics, within what the statistics' own tolerances allow.
    The device statistics are held to the existing parity rule (tests/test_gmm_em_batch.py, tests/test_gpu_parity.py), unchanged:
    |d nk| <= e_n = 1e-4 (nk + max nk), |d sx| <= e_x = 1e-4 (|sx| + max |sx|), |d sxx| <= e_xx likewise.  Through the formulas, with
    r the relevance factor and N = nk + r - e_n:
      mu^ = (sx + r mu) / (nk + r)                    |d mu^| <= b_m = (e_x + |mu^| e_n) / N
      cv^ = (sxx + r (cv + mu^2)) / (nk + r) - mu^^2  |d cv^| <= (e_xx + (cv^ + mu^^2) e_n) / N + 2 |mu^| b_m + b_m^2
      w~  = (nk^2 / T + r w) / (nk + r)               |d w~|  <= b_u = e_n (2 nk / T + w~) / N;  w^ = w~ / sum w~:
                                                      |d w^|  <= (b_u + w^ sum b_u) / (sum w~ - sum b_u)
    Under 'm' weights_ and covariances_ are the UBM's arrays exactly."""
    from speech_signal_processing_amd.gmm_train import map_adapt
    api, _lib, ctx = env
    K, D, r = 16, 26, 16.0
    g = make_inputs(K, D, 3, 77, lens=[5, 700, 1800])
    w, mu, cv = g["w"], g["mu"], g["cv"]
    rng = np.random.default_rng(3)
    Xs = []
    for s in range(3):   # every speaker's frames come from ITS means
        n = g["lens"][s]
        k = rng.choice(K, size=n, p=w)
        Xs.append((g["sm"][s][k] + np.sqrt(cv[k]) * rng.standard_normal((n, D))).astype(np.float32))
    ubm = _Model(w, mu, cv)
    gms = map_adapt(ubm, Xs, relevance_factor=r, adapt=adapt)
    assert len(gms) == 3
    for s, (gm, X) in enumerate(zip(gms, Xs)):
        T = len(X)
        nk, sx, sxx = MO.stats(w, mu, cv, X)
        w2, m2, v2 = MO.adapt_from_stats(w, mu, cv, nk, sx, sxx, T, r, adapt)
        e_n = 1e-4 * (nk + nk.max())
        e_x = 1e-4 * (np.abs(sx) + np.abs(sx).max())
        e_xx = 1e-4 * (np.abs(sxx) + np.abs(sxx).max())
        N = (nk + r - e_n)[:, None]
        b_m = (e_x + np.abs(m2) * e_n[:, None]) / N
        err = np.abs(gm.means_ - m2)
        print("[measured] map_adapt %s speaker %d: means err %.3e (bound min %.3e)" % (adapt, s, err.max(), b_m.min()))
        assert (err <= b_m).all(), (adapt, s, float((err / b_m).max()))
        if "w" in adapt:
            wt = (nk * nk / T + r * w) / (nk + r)
            b_u = e_n * (2 * nk / T + wt) / N[:, 0]
            b_w = (b_u + w2 * b_u.sum()) / (wt.sum() - b_u.sum())
            assert (np.abs(gm.weights_ - w2) <= b_w).all() and abs(gm.weights_.sum() - 1.0) <= 1e-12
        else:
            assert gm.weights_ is ubm.weights_ or np.array_equal(gm.weights_, w)
        if "v" in adapt:
            b_v = (e_xx + (v2 + m2 * m2) * e_n[:, None]) / N + 2 * np.abs(m2) * b_m + b_m * b_m
            assert (np.abs(gm.covariances_ - v2) <= b_v).all() and (gm.covariances_ >= 1e-6).all()
        else:
            assert np.array_equal(gm.covariances_, cv)
        assert np.array_equal(gm.precisions_cholesky_, 1.0 / np.sqrt(gm.covariances_))
        assert np.array_equal(gm.precisions_, gm.precisions_cholesky_ ** 2)
        assert gm.converged_ is True and gm.n_iter_ == 1 and gm.n_components == K
    if adapt == "m":
        assert all(np.array_equal(gm.weights_, w) and np.array_equal(gm.covariances_, cv) for gm in gms)
    import pickle
    back = pickle.loads(pickle.dumps(gms))   # (save_models / load_models: ordinary pickles)
    assert all(np.array_equal(a.means_, b.means_) for a, b in zip(gms, back))
    bad = [x.copy() for x in Xs]
    bad[2][17, 3] = np.inf
    with pytest.raises(ValueError, match=r"speaker 2.*row 17"):
        map_adapt(ubm, bad, relevance_factor=r, adapt=adapt)


# ===================================================================================================== 3. selection
@pytest.mark.parametrize("K,D,Ck,S", CASES, ids=ids(CASES))
def test_selection(env, K, D, Ck, S):
    """On every frame whose oracle gap lp_(C) - lp_(C+1) is >= 1e-3 nats the selected SET is the oracle's; where every neighbouring
    difference among the C + 1 best is >= 1e-3 (map_oracle.rank_gap) the rank ORDER is the oracle's too, and on the frames in between
    the device's order is one the oracle's values allow (non-increasing within 1e-3): no frame above the gap escapes.  At most 1 % of
    the frames lie under the gap — a condition on the inputs, asserted."""
    g = case(env, K, D, Ck, S)
    idx, own = np.asarray(g["got"]["idx"]), g["own"]
    assert idx.shape == (g["off"][-1], Ck) and idx.dtype == np.int32
    sure = own["gap"] >= GAP
    print("[measured] selection K %d C %d: %.3f %% of frames under the gap, %.3f %% under the rank gap" % (
        K, Ck, 100 * (1 - sure.mean()), 100 * (own["rank_gap"] < GAP).mean()))
    assert (~sure).mean() <= 0.01, "inputs: too many frames under the gap"
    assert (idx >= 0).all() and (idx < K).all()
    assert (np.sort(idx, 1)[sure] == np.sort(own["idx"], 1)[sure]).all()
    ranked = own["rank_gap"] >= GAP
    assert (idx[ranked] == own["idx"][ranked]).all()
    vals = np.take_along_axis(own["lp"], idx.astype(np.int64), 1)
    assert (np.diff(vals, axis=1)[sure] <= GAP).all()
    assert all(len(set(row)) == Ck for row in idx[~sure])   # (even under the gap: C distinct mixtures)


# ===================================================================================================== 4. scores, 5. arg-max
@pytest.mark.parametrize("K,D,Ck,S", CASES, ids=ids(CASES))
def test_scores_and_argmax(env, K, D, Ck, S):
    """diff_out and ubm_out against the oracle evaluated with the device's own idx_out: atol 2e-4, rtol 1e-4 (the lp error, 4.1e-5 nats at
    most, is common to L_s and L_ubm and largely cancels; delta's D-term fp32 dot is about 1e-5; log-sum-exp is 1-Lipschitz and the mean
    a mean: 2e-4 is twice the un-cancelled worst case 2 x 4.1e-5 + 1e-5, rounded up).  The arg-max is exact wherever the oracle's top-2
    margin exceeds 1e-3, which at least 99 % of the utterances do (asserted)."""
    g = case(env, K, D, Ck, S)
    got, ref = g["got"], g["ref"]
    full = np.array(g["lens"]) > 0
    assert got["diff"].shape == (len(g["lens"]), S) and got["diff"].dtype == np.float32
    d_err = np.abs(got["diff"][full] - ref["diff"][full])
    u_err = np.abs(got["ubm"][full] - ref["ubm"][full])
    print("[measured] scores K %d D %d C %d S %d: diff err %.3e (max |diff| %.3e), ubm err %.3e" % (
        K, D, Ck, S, d_err.max(), np.abs(ref["diff"][full]).max(), u_err.max()))
    assert (d_err <= ATOL + RTOL * np.abs(ref["diff"][full])).all()
    assert (u_err <= ATOL + RTOL * np.abs(ref["ubm"][full])).all()
    assert np.isnan(got["diff"][~full]).all() and np.isnan(got["ubm"][~full]).all() and (got["argmax"][~full] == 0).all()
    if S > 1:
        top = np.sort(ref["diff"][full], 1)
        clear = top[:, -1] - top[:, -2] > GAP
        assert clear.mean() >= 0.99, "inputs: too many utterances inside the margin"
        assert (got["argmax"][full][clear] == ref["diff"][full].argmax(1)[clear]).all()
    else:
        assert (got["argmax"] == 0).all()
    assert (got["argmax"][full] == np.asarray(got["diff"])[full].argmax(1)).all()   # numpy's first-index rule on the device's own row


# ===================================================================================================== 6. the pin
def test_full_selection_is_the_dense_scorer(env):
    """K = 8, C = 8: diff_out = scores[:, 1:] - scores[:, :1] of GmmScorer at precision 0 on the same models within the score tolerance,
    equal arg-max; and the same through GMM_UBM.score_matrix(..., top_c=8) against top_c=None"""
    from speech_signal_processing_amd import GMM_UBM
    api, _lib, ctx = env
    K, D, S = 8, 13, 3
    g = make_inputs(K, D, S, 99)
    sc = api.MapScorer(ctx, g["w"], g["mu"], g["cv"], g["sm"])
    seg = api.Segments.from_lengths(ctx, g["lens"])
    got = sc.score(g["X"], seg, top_c=K)
    dense = api.GmmScorer(ctx, np.stack([g["w"]] * (S + 1)), np.concatenate([g["mu"][None], g["sm"]]), np.stack([g["cv"]] * (S + 1)))
    r = dense.score(g["X"], seg, precision=0)
    want = r["scores"][:, 1:].astype(np.float64) - r["scores"][:, :1]
    full = np.array(g["lens"]) > 0
    err = np.abs(got["diff"][full] - want[full])
    print("[measured] pin: max |diff - dense| %.3e" % err.max())
    assert (err <= ATOL + RTOL * np.abs(want[full])).all()
    assert np.array_equal(got["argmax"], r["argmax"])
    ubm = _Model(g["w"], g["mu"], g["cv"])
    models = [_Model(g["w"], m, g["cv"]) for m in g["sm"]]
    feats = [g["X"][g["off"][u]:g["off"][u + 1]].astype(np.float64) for u in range(len(g["lens"]))]
    p8, a8 = GMM_UBM.score_matrix(models, ubm, feats, top_c=8)
    pd, ad = GMM_UBM.score_matrix(models, ubm, feats)
    assert p8.shape == pd.shape and p8.dtype == pd.dtype and a8.dtype == ad.dtype
    assert (np.abs(p8[full] - pd[full]) <= ATOL + RTOL * np.abs(pd[full])).all() and np.array_equal(a8, ad)
    assert np.isnan(p8[~full]).all() and np.array_equal(p8[full], got["diff"][full].astype(np.float64))   # score_list = score on the stacked rows
    sc.close()


# ===================================================================================================== 7. non-finite and empty utterances
@pytest.mark.parametrize("K,D,Ck,S", [(70, 39, 5, 65), (8, 13, 8, 3)], ids=ids([(70, 39, 5, 65), (8, 13, 8, 3)]))
def test_nonfinite_rows_and_determinism(env, K, D, Ck, S):
    """a bad frame: its utterance's diff row and ubm NaN, arg-max 0, its idx row -1; an empty utterance likewise; every other utterance
    bit-identical to the call on clean rows; a second identical call returns identical bits; host and device features agree"""
    import torch
    from speech_signal_processing_amd import GMM_UBM
    api, _lib, ctx = env
    g = make_inputs(K, D, S, 5 + K)
    sc = api.MapScorer(ctx, g["w"], g["mu"], g["cv"], g["sm"])
    seg = api.Segments.from_lengths(ctx, g["lens"])
    kw = dict(top_c=Ck, diff=True, ubm=True, argmax=True, idx=True)
    clean = sc.score(g["X"], seg, **kw)
    X = g["X"].copy()
    off = g["off"]
    spots = {3: (off[3] + 64, 2, np.nan), 5: (off[5] + 297, D - 1, np.inf), 0: (off[0], 0, -np.inf)}   # a second block's first frame, a last frame, T = 1
    for u, (f, d, v) in spots.items():
        X[f, d] = v
    got = sc.score(X, seg, **kw)
    again = sc.score(X, seg, **kw)
    dev = sc.score(torch.from_numpy(X).cuda(), seg, **kw)
    for key in ("diff", "ubm", "argmax", "idx"):
        assert np.array_equal(got[key], again[key], equal_nan=True), key
        assert np.array_equal(got[key], dev[key].cpu().numpy(), equal_nan=True), key
    hit = np.zeros(len(g["lens"]), bool)
    hit[list(spots)] = True
    hit |= np.array(g["lens"]) == 0
    assert np.isnan(got["diff"][hit]).all() and np.isnan(got["ubm"][hit]).all() and (got["argmax"][hit] == 0).all()
    for key in ("diff", "ubm", "argmax"):
        assert np.array_equal(got[key][~hit], clean[key][~hit]), key
    assert np.isfinite(got["diff"][~hit]).all()
    bad_rows = np.array([f for f, _, _ in spots.values()])
    assert (got["idx"][bad_rows] == -1).all()
    keep = np.ones(len(X), bool)
    keep[bad_rows] = False
    assert np.array_equal(got["idx"][keep], clean["idx"][keep])
    models = [_Model(g["w"], m, g["cv"]) for m in g["sm"]]
    feats = [X[off[u]:off[u + 1]] for u in range(len(g["lens"]))]
    with pytest.raises(ValueError, match="utterance 0 .and 2 more."):
        GMM_UBM.score_matrix(models, _Model(g["w"], g["mu"], g["cv"]), feats, top_c=Ck)
    sc.close()


# ===================================================================================================== 8. raw-ABI error codes
def test_raw_abi_error_codes(env):
    api, _lib, ctx = env
    lib = ctx._lib
    K, D, S = 8, 13, 2
    g = make_inputs(K, D, S, 123, lens=[40, 70])
    w0 = g["w"].copy()
    w0[[1, 4, 6]] = 0.0   # three mixtures that do not exist: five remain
    w0 /= w0.sum()

    def pack(K_, D_, w, mu, cv, S_, sm):
        h = C.c_void_p()
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (w, mu, cv, sm)]
        rc = lib.ssp_gmm_map_pack(ctx._h, K_, D_, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, S_, arrs[3].ctypes.data, C.byref(h))
        return rc, h

    assert pack(K, D, g["w"], g["mu"], g["cv"], 0, g["sm"])[0] == _lib.SSP_ERR_INVALID             # S < 1
    assert pack(K, D, -g["w"], g["mu"], g["cv"], S, g["sm"])[0] == _lib.SSP_ERR_INVALID            # a negative weight
    assert pack(K, D, 0 * g["w"], g["mu"], g["cv"], S, g["sm"])[0] == _lib.SSP_ERR_INVALID         # all zero
    assert pack(K, D, g["w"], g["mu"], 0 * g["cv"], S, g["sm"])[0] == _lib.SSP_ERR_INVALID         # a covariance that is not > 0
    assert pack(1, 48, np.ones(1), np.zeros((1, 48)), np.ones((1, 48)), 1, np.zeros((1, 1, 48)))[0] == _lib.SSP_ERR_UNSUPPORTED   # D > 47
    rc, h = pack(K, D, w0, g["mu"], g["cv"], S, g["sm"])
    assert rc == _lib.SSP_OK and h.value
    seg = api.Segments.from_lengths(ctx, g["lens"])
    X = g["X"]
    diff = np.full((2, S), 7.0, np.float32)

    def score(Ck, idx=None):
        return lib.ssp_gmm_map_score(h, X.ctypes.data, seg._h, Ck, diff.ctypes.data, None, None, None if idx is None else idx.ctypes.data,
                                     _lib.HOST, None)

    assert score(0) == _lib.SSP_ERR_INVALID and score(-3) == _lib.SSP_ERR_INVALID            # C < 1
    assert score(6) == _lib.SSP_ERR_INVALID                                                    # more than the five mixtures of non-zero weight
    assert b"non-zero weight" in lib.ssp_last_error()
    assert score(9) == _lib.SSP_ERR_UNSUPPORTED                                                # C > 8
    assert (diff == 7.0).all()                                                                 # nothing was written
    idx = np.empty((110, 5), np.int32)
    assert score(5, idx) == _lib.SSP_OK                                                        # the handle and its ctx stay usable
    assert np.isfinite(diff).all() and not np.isin(idx, [1, 4, 6]).any()                       # zero-weight mixtures are never selected
    assert (np.sort(idx, 1) == np.array([0, 2, 3, 5, 7])).all()
    ref = MO.topc_scores(w0, g["mu"], g["cv"], g["sm"], X, g["off"], 5, idx=idx)
    assert (np.abs(diff - ref["diff"]) <= ATOL + RTOL * np.abs(ref["diff"])).all()
    assert lib.ssp_gmm_map_destroy(h) == _lib.SSP_OK
    with pytest.raises(ValueError):            # the object layer maps the codes as its neighbours do
        api.MapScorer(ctx, g["w"], g["mu"], g["cv"], g["sm"]).score(X, seg, top_c=0)
    with pytest.raises(NotImplementedError):
        api.MapScorer(ctx, g["w"], g["mu"], g["cv"], g["sm"]).score(X, seg, top_c=9)


# ===================================================================================================== 9. surface
def test_from_sklearn_refuses_models_that_are_not_mean_adapted(env):
    from speech_signal_processing_amd.gmm_train import map_adapt
    api, _lib, ctx = env
    g = make_inputs(8, 13, 2, 31, lens=[400, 500])
    ubm = _Model(g["w"], g["mu"], g["cv"])
    Xs = [g["X"][:400], g["X"][400:]]
    good = map_adapt(ubm, Xs, adapt="m")
    mw = map_adapt(ubm, Xs, adapt="mw")
    with pytest.raises(ValueError, match=r"model 1: weights_"):
        api.MapScorer.from_sklearn(ctx, [good[0], mw[1]], ubm)
    sc = api.MapScorer.from_sklearn(ctx, good, ubm)
    assert (sc.S, sc.K, sc.D) == (2, 8, 13)
    sc.close()


def test_gmm_ubm_map_adapted_end_to_end(env, capsys):
    """GMM_UBM.GMM(adapt='map', top_c=5) on 4 synthetic speakers: the UBM is the one adapt=None trains, the speaker models are its
    mean-adapted copies, and the training utterances are classified as their own speakers"""
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
    acc_train, acc = GMM_UBM.GMM(train, x_train, y_train, x_test, y_test, n_components=K, random_state=0, adapt="map", top_c=5)
    assert "train acc" in capsys.readouterr().out
    assert acc_train == 1.0 and acc >= 0.75
    gmms, ubm = GMM_UBM.GMM.last_model
    ubm_ref = GaussianMixture(n_components=K, covariance_type="diag", random_state=0).fit(np.vstack([train[s] for s in sorted(train)]))
    assert np.array_equal(ubm.means_, ubm_ref.means_) and np.array_equal(ubm.weights_, ubm_ref.weights_)
    assert len(gmms) == S and all(np.array_equal(gm.covariances_, ubm.covariances_) and np.array_equal(gm.weights_, ubm.weights_) for gm in gmms)
    assert not np.array_equal(gmms[0].means_, ubm.means_)
    dense = GMM_UBM.score_matrix(gmms, ubm, x_train)[1]   # the same models through the dense path agree on who spoke
    assert np.array_equal(dense, np.array(y_train))
    with pytest.raises(ValueError, match="adapt"):
        GMM_UBM.GMM(train, x_train, y_train, x_test, y_test, n_components=K, adapt="mean")
