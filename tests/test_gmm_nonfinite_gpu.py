"""Non-finite feature rows through the GMM scorer and the EM kernels, held to the contract of include/ssp.h (ssp_gmm_score,
ssp_gmm_em_stats, ssp_gmm_em_stats_batch): a bad frame (any entry NaN or +-inf) is NaN under every model, its utterance's scores are NaN
with arg-max 0, a model trained on it has NaN statistics — and nobody else changes: not the other utterance of the same wave piece, not
the other lane half, not the float64 piece sums, not the compact re-scoring matrix, not the other models of an EM batch launch.

References: oracle.ref_cpu (float64; tests/test_gmm_nonfinite_host.py holds it to the same rules) and the same call on the cleaned batch.
Score rule: |gpu - ref| <= 1e-4 |ref| on utterance scores, rtol = atol = 2e-4 on per-frame log-likelihoods (tools/fuzz_scoring.py).
Every batch's clean utterances have a float64 top-2 margin above 10 x that score tolerance (asserted), so the arg-max of every precision
is the oracle's and a changed arg-max is a changed neighbour, not a close call."""
import numpy as np
import pytest

from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

BAD = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
SCORE_RTOL = 1e-4
LL_TOL = 2e-4

# (K, D, models, UBM): NQ 4 with the 64-frame piece granule | the reference shape | three 32-mixture tiles, the last padded | NQ 32 with the
# 32-frame granule (no bf16 image: precision 0 only)
MODELS = [(16, 13, 4, True), (64, 39, 5, True), (70, 47, 3, False), (5, 100, 2, False)]
MODEL_IDS = ["K16_D13", "K64_D39", "K70_D47", "K5_D100"]
# 694 frames in three 256-frame workgroups: a 1-frame and an empty utterance, lengths around the 32 / 64-frame granules
LENS = [70, 1, 0, 64, 65, 31, 33, 300, 2, 128]
OFFS = np.concatenate([[0], np.cumsum(LENS)])
# first / last frame of an utterance (135, 199; 264, 563), the 1-frame utterance (70), the frames just before and after the empty one
# (70, 71), global index = 0 / 31 / 32 / 63 mod 64 (0, 64, 320; 351; 352; 63, 383), 255 / 256, the batch's last frame (693)
POSITIONS = [0, 63, 64, 69, 70, 71, 134, 135, 199, 255, 256, 264, 320, 351, 352, 383, 563, 564, 693]
# seeds at which the margin precondition holds (a seed that does not is changed, never the limit)
SEEDS = {"K16_D13": 100, "K64_D39": 100, "K70_D47": 100, "K5_D100": 100, "many": 200, "auto": 202, "e2e": 415}


def make_models(K, D, M, ubm, rng):
    """weights, means, covariances (M, ...): speaker means 0.2 sigma from the UBM's (without a UBM: from a common centre)"""
    w = rng.dirichlet(5 * np.ones(K))
    mu = rng.standard_normal((K, D))
    cov = rng.uniform(0.5, 2.0, (K, D))
    n_spk = M - 1 if ubm else M
    mus = ([mu] if ubm else []) + [mu + 0.2 * np.sqrt(cov) * rng.standard_normal((K, D)) for _ in range(n_spk)]
    return np.stack([w] * M), np.stack(mus), np.stack([cov] * M)


def make_batch(w, mus, cov, ubm, lens, rng):
    """utterance u speaks as speaker u mod S: frames around that model's component means"""
    first = 1 if ubm else 0
    S = len(mus) - first
    out = []
    for u, n in enumerate(lens):
        comp = rng.choice(w.shape[1], size=n, p=w[0])
        out.append((mus[first + u % S][comp] + 0.5 * np.sqrt(cov[0][comp]) * rng.standard_normal((n, mus.shape[2]))).astype(np.float32))
    return out


def oracle_loglik(w, mus, cov, X):
    return np.stack([O.gmm_score_samples(w[m], mus[m], cov[m], X) for m in range(len(mus))]) if len(X) else np.zeros((len(mus), 0))


def oracle_scores(ll, lens):
    off = np.concatenate([[0], np.cumsum(lens)])
    with np.errstate(all="ignore"):
        return np.array([ll[:, off[u]:off[u + 1]].mean(axis=1) if lens[u] else np.full(ll.shape[0], np.nan) for u in range(len(lens))])


def margins_and_argmax(scores, ubm):
    """float64 top-2 margin and arg-max of score - score_ubm over the speaker models, per utterance"""
    d = scores[:, 1:] - scores[:, :1] if ubm else scores
    srt = np.sort(d, axis=1)
    return srt[:, -1] - srt[:, -2], d.argmax(axis=1)


def check_precondition(scores, ubm, lens):
    nz = np.asarray(lens) > 0
    margin, am = margins_and_argmax(scores[nz], ubm)
    tol = SCORE_RTOL * np.abs(scores[nz]).max(axis=1)
    worst = int((margin / tol).argmin())
    assert (margin > 10 * tol).all(), "top-2 margin %.3g within 10 x the score tolerance %.3g: change the seed" % (margin[worst], tol[worst])
    full = np.zeros(len(lens), dtype=np.int64)
    full[nz] = am
    return full


_CASES = {}


def sweep_case(name):
    """models, the sweep batch and its float64 reference, built once per model shape"""
    if name not in _CASES:
        K, D, M, ubm = MODELS[MODEL_IDS.index(name)]
        rng = np.random.default_rng(SEEDS[name])
        w, mus, cov = make_models(K, D, M, ubm, rng)
        feats = make_batch(w, mus, cov, ubm, LENS, rng)
        X = np.vstack(feats)
        ll = oracle_loglik(w, mus, cov, X)
        sc = oracle_scores(ll, LENS)
        am = check_precondition(sc, ubm, LENS)
        _CASES[name] = dict(K=K, D=D, M=M, ubm=ubm, w=w, mus=mus, cov=cov, X=X, ll=ll, scores=sc, argmax=am)
    return _CASES[name]


@pytest.fixture(scope="module")
def api():
    from speech_signal_processing_amd import api
    return api


def plant(X, frame, D, kind, k):
    """one bad entry at `frame`; the column rotates over 0, D - 1 and the middle"""
    Xb = X.copy()
    Xb[frame, (0, D - 1, D // 2)[k % 3]] = BAD[kind]
    return Xb


def utt_of(frame, offs=OFFS):
    return int(np.searchsorted(offs, frame, side="right")) - 1


def check_call(r, clean, ref_ll, ref_sc, ref_am, lens, bad_frames, precision, what):
    """rules 1 to 3 of the contract on one call's result `r` (host arrays) against the clean call `clean` and the float64 reference of
    the CLEAN batch (frames are independent: the bad batch's reference is the clean one with NaN at the bad frames)"""
    offs = np.concatenate([[0], np.cumsum(lens)])
    bad_frames = np.asarray(sorted(bad_frames), dtype=np.int64)
    bad_utts = np.unique(np.searchsorted(offs, bad_frames, side="right") - 1)
    nz = np.asarray(lens) > 0
    good = nz.copy()
    good[bad_utts] = False
    exact = precision in (0, 2)
    if "loglik" in r:
        ll = np.asarray(r["loglik"])
        fin = np.ones(ll.shape[1], dtype=bool)
        fin[bad_frames] = False
        assert np.isnan(ll[:, ~fin]).all(), (what, "bad frame not NaN under every model", ll[:, ~fin])
        assert np.isfinite(ll[:, fin]).all(), (what, "a clean frame is not finite", np.flatnonzero(~np.isfinite(ll).all(axis=0)))
        if exact:
            assert np.array_equal(ll[:, fin], np.asarray(clean["loglik"])[:, fin]), (what, "a clean frame's log-likelihood changed")
        if precision != 2:
            np.testing.assert_allclose(ll[:, fin], ref_ll[:, fin], rtol=LL_TOL, atol=LL_TOL, err_msg=str(what))
    sc, am = np.asarray(r["scores"]), np.asarray(r["argmax"])
    assert np.isnan(sc[bad_utts]).all(), (what, "bad utterance's scores", sc[bad_utts])
    assert (am[bad_utts] == 0).all(), (what, "bad utterance's arg-max", am[bad_utts])
    if exact:
        assert np.array_equal(sc[good], np.asarray(clean["scores"])[good]), (what, "a clean utterance's scores changed")
        assert np.array_equal(am[good], np.asarray(clean["argmax"])[good]), (what, "a clean utterance's arg-max changed")
    if precision != 2:
        assert np.array_equal(am[good], ref_am[good]), (what, "arg-max differs from precision 0's", am[good], ref_am[good])
        err = np.abs(sc[good] - ref_sc[good])
        assert (err <= SCORE_RTOL * np.abs(ref_sc[good])).all(), (what, "score rule", float((err / np.abs(ref_sc[good])).max()))
    else:  # bf16x3 alone: the arg-max is not promised against close calls, but the margins here are 10 x the tolerance
        assert np.array_equal(am[good], ref_am[good]), (what, "arg-max", am[good], ref_am[good])


# ------------------------------------------------------------------------------------------------- the position sweep
# (no bf16 image above D = 64: precision 0 is the only path there, ssp_gmm_score answers SSP_ERR_UNSUPPORTED to the others)
SWEEP = [(name, p) for name, shape in zip(MODEL_IDS, MODELS) for p in ((0, 1, 2, 3) if shape[1] <= 64 else (0,))]


@pytest.mark.parametrize("name,precision", SWEEP, ids=["%s_p%d" % np_ for np_ in SWEEP])
def test_position_sweep_one_bad_entry_per_call(api, name, precision):
    c = sweep_case(name)
    ctx = api.default_context()
    sc = api.GmmScorer(ctx, c["w"], c["mus"], c["cov"], has_ubm=c["ubm"])
    seg = api.Segments.from_lengths(ctx, LENS)
    # precision 0's arg-max on the clean batch is the oracle's (the margins are 10 x the tolerance)
    a0 = np.asarray(sc.score(c["X"], seg, precision=0)["argmax"])
    nz = np.asarray(LENS) > 0
    assert np.array_equal(a0[nz], c["argmax"][nz])
    for loglik in (False, True):
        clean = sc.score(c["X"], seg, loglik=loglik, precision=precision)
        n_clean = sc.last_rescored
        check_call(clean, clean, c["ll"], c["scores"], a0, LENS, [], precision, (name, precision, loglik, "clean"))
        k = 0
        for frame in POSITIONS:
            for kind in BAD:
                Xb = plant(c["X"], frame, c["D"], kind, k)
                k += 1
                with np.errstate(all="ignore"):   # the reference of the bad frame itself: NaN under every model
                    assert np.isnan(oracle_loglik(c["w"], c["mus"], c["cov"], Xb[frame:frame + 1])).all()
                r = sc.score(Xb, seg, loglik=loglik, precision=precision)
                what = (name, "precision", precision, "loglik", loglik, "frame", frame, kind)
                check_call(r, clean, c["ll"], c["scores"], a0, LENS, [frame], precision, what)
                # listing: the bad utterance is one more than the clean call lists.  A call with loglik scores the matrix in one pass
                # without a host wait (tests/test_gpu_stream_order.py::test_gmm_score holds it to that) and lists nothing at any precision
                if precision in (1, 3) and not loglik:
                    n = sc.last_rescored
                    assert 1 <= n <= 1 + n_clean, (what, "last_rescored", n, "clean call", n_clean)
                else:
                    assert sc.last_rescored == 0, what


# ------------------------------------------------------------------------------------------------- many bad utterances
def _many_case(key, n_utt, lo, hi):
    if key not in _CASES:
        K, D, M, ubm = MODELS[0]
        rng = np.random.default_rng(SEEDS[key])
        w, mus, cov = make_models(K, D, M, ubm, rng)
        lens = [int(v) for v in rng.integers(lo, hi + 1, n_utt)]
        X = np.vstack(make_batch(w, mus, cov, ubm, lens, rng))
        ll = oracle_loglik(w, mus, cov, X)
        sc = oracle_scores(ll, lens)
        am = check_precondition(sc, ubm, lens)
        _CASES[key] = dict(K=K, D=D, M=M, ubm=ubm, w=w, mus=mus, cov=cov, X=X, ll=ll, scores=sc, argmax=am, lens=lens,
                           offs=np.concatenate([[0], np.cumsum(lens)]), rng=rng)
    return _CASES[key]


def _plant_many(c, utts, rng):
    """one bad entry in every utterance of `utts`: frame, column and kind drawn per utterance"""
    Xb = c["X"].copy()
    kinds = list(BAD.values())
    frames = []
    for i, u in enumerate(utts):
        f = int(c["offs"][u] + rng.integers(0, c["lens"][u]))
        Xb[f, int(rng.integers(0, c["D"]))] = kinds[i % 3]
        frames.append(f)
    return Xb, frames


@pytest.mark.parametrize("precision", [0, 1, 2, 3])
def test_a_bad_frame_in_every_second_of_600_utterances(api, precision):
    """half of the candidate lists carry count -1 (every model), the re-scoring launch's block tables mix them with clean close calls"""
    c = _many_case("many", 600, 5, 80)
    ctx = api.default_context()
    sc = api.GmmScorer(ctx, c["w"], c["mus"], c["cov"], has_ubm=c["ubm"])
    seg = api.Segments.from_lengths(ctx, c["lens"])
    a0 = np.asarray(sc.score(c["X"], seg, precision=0)["argmax"])
    assert np.array_equal(a0, c["argmax"])
    Xb, frames = _plant_many(c, range(1, 600, 2), np.random.default_rng(5))
    for loglik in (False, True):
        clean = sc.score(c["X"], seg, loglik=loglik, precision=precision)
        n_clean = sc.last_rescored
        r = sc.score(Xb, seg, loglik=loglik, precision=precision)
        n = sc.last_rescored
        check_call(r, clean, c["ll"], c["scores"], a0, c["lens"], frames, precision, ("many", precision, loglik))
        if precision in (1, 3) and not loglik:
            assert 300 <= n <= 300 + n_clean, (n, n_clean)
        else:
            assert n == 0, (precision, loglik, n)


# ------------------------------------------------------------------------------------------------- precision = "auto"
@pytest.mark.parametrize("n_bad", [12, 1100])
def test_precision_auto_with_few_and_with_mostly_bad_utterances(api, n_bad):
    """1200 utterances (AUTO_MIN_UTTS is 1024: below it the call is plain precision 0): whichever of 1 and 0 the call chooses, bad rows
    are NaN with arg-max 0 and everybody else keeps precision 0's arg-max"""
    c = _many_case("auto", 1200, 5, 40)
    ctx = api.default_context()
    sc = api.GmmScorer(ctx, c["w"], c["mus"], c["cov"], has_ubm=c["ubm"])
    seg = api.Segments.from_lengths(ctx, c["lens"])
    utts = np.sort(np.random.default_rng(n_bad).choice(1200, size=n_bad, replace=False))
    Xb, frames = _plant_many(c, utts, np.random.default_rng(6))
    r0 = sc.score(Xb, seg, precision=0)
    r = sc.score(Xb, seg, precision="auto")
    used = sc.last_auto["precision_used"]
    assert used in (0, 1), used
    am, s = np.asarray(r["argmax"]), np.asarray(r["scores"])
    assert np.array_equal(am, np.asarray(r0["argmax"]))
    good = np.ones(1200, dtype=bool)
    good[utts] = False
    assert np.isnan(s[utts]).all() and (am[utts] == 0).all()
    assert np.array_equal(am[good], c["argmax"][good])
    err = np.abs(s[good] - c["scores"][good])
    assert (err <= SCORE_RTOL * np.abs(c["scores"][good])).all(), float((err / np.abs(c["scores"][good])).max())


# ------------------------------------------------------------------------------------------------- routes
def test_every_route_gives_the_same_bits(api, monkeypatch):
    """device tensors, host arrays, host arrays in slices, scratch-bounded batches and score_list on float64 matrices (1e300 narrows to
    +inf: a bad frame) — bit-equal at precision 0 and 2, arg-max-equal at precision 1"""
    import torch
    c = sweep_case("K64_D39")
    D = c["D"]
    X64 = c["X"].astype(np.float64)
    bad = {3: (100, 0, np.nan), 6: (231, D - 1, -np.inf), 9: (693, D // 2, 1e300)}   # utterance: (frame, column, value)
    for f, col, v in bad.values():
        X64[f, col] = v
    with np.errstate(over="ignore"):
        X = X64.astype(np.float32)
    assert np.isposinf(X[693, D // 2])
    frames = [f for f, _, _ in bad.values()]
    hctx, tctx = api.default_context(), api.default_context(torch_stream=True)
    hsc = api.GmmScorer(hctx, c["w"], c["mus"], c["cov"], has_ubm=True)
    tsc = api.GmmScorer(tctx, c["w"], c["mus"], c["cov"], has_ubm=True)
    hseg, tseg = api.Segments.from_lengths(hctx, LENS), api.Segments.from_lengths(tctx, LENS)
    Xd = torch.from_numpy(X).cuda()
    mats = [X64[OFFS[u]:OFFS[u + 1]] for u in range(len(LENS))]
    nz = np.asarray(LENS) > 0
    a0 = None
    for prec in (0, 2, 1):
        clean = hsc.score(c["X"], hseg, precision=prec)
        dev = tsc.score(Xd, tseg, precision=prec)
        dev = {k: v.cpu().numpy() for k, v in dev.items()}
        check_call(dev, clean, c["ll"], c["scores"], c["argmax"], LENS, frames, prec, ("device", prec))
        if a0 is None:
            a0 = dev["argmax"]
        routes = {"host": hsc.score(X, hseg, precision=prec), "score_list": hsc.score_list(mats, precision=prec)}
        monkeypatch.setenv("SSP_GMM_SCRATCH_BYTES", str(c["M"] * 8 * 12))   # room for 12 piece sums per batch
        routes["bounded scratch"] = hsc.score(X, hseg, precision=prec)
        monkeypatch.delenv("SSP_GMM_SCRATCH_BYTES")
        for route, r in routes.items():
            if prec == 1:
                assert np.array_equal(np.asarray(r["argmax"])[nz], a0[nz]), (route, prec)
                assert np.isnan(np.asarray(r["scores"])[[3, 6, 9]]).all(), (route, prec)
            else:
                assert np.array_equal(np.asarray(r["scores"])[nz], dev["scores"][nz], equal_nan=True), (route, prec)
                assert np.array_equal(np.asarray(r["argmax"])[nz], dev["argmax"][nz]), (route, prec)
    # ---- host arrays in slices: 1-MiB slices on a batch above 2 MiB, built by repeating the batch (bad rows on both sides of every border)
    REP = 24
    Xr = np.tile(X, (REP, 1))
    lens_r = LENS * REP
    assert Xr.nbytes > 2 * (1 << 20)
    per_slice = (1 << 20) // (D * 4)
    offs_r = np.concatenate([[0], np.cumsum(lens_r)])
    bad_r = np.flatnonzero(~np.isfinite(Xr).all(axis=1))
    assert (bad_r < per_slice - 694).any() and (bad_r > per_slice).any()   # whole utterances per slice: the first border lies in between
    hseg_r, tseg_r = api.Segments.from_lengths(hctx, lens_r), api.Segments.from_lengths(tctx, lens_r)
    Xrd = torch.from_numpy(Xr).cuda()
    nz_r = np.asarray(lens_r) > 0
    bad_u = np.unique(np.searchsorted(offs_r, bad_r, side="right") - 1)
    for prec in (0, 2, 1):
        dev = {k: v.cpu().numpy() for k, v in tsc.score(Xrd, tseg_r, precision=prec).items()}
        whole = hsc.score(Xr, hseg_r, precision=prec)
        monkeypatch.setenv("SSP_HOST_SLICE_MB", "1")
        sliced = hsc.score(Xr, hseg_r, precision=prec)
        monkeypatch.delenv("SSP_HOST_SLICE_MB")
        assert np.isnan(dev["scores"][bad_u]).all() and (dev["argmax"][bad_u] == 0).all()
        for route, r in (("host whole", whole), ("host sliced", sliced)):
            assert np.isnan(r["scores"][bad_u]).all() and (r["argmax"][bad_u] == 0).all(), (route, prec)
            assert np.array_equal(r["argmax"][nz_r], dev["argmax"][nz_r]), (route, prec)
            if prec != 1:
                assert np.array_equal(r["scores"][nz_r], dev["scores"][nz_r], equal_nan=True), (route, prec)
        # every repeat of the batch: the clean utterances keep the oracle's arg-max
        ref_am = np.tile(c["argmax"], REP)
        good = nz_r.copy()
        good[bad_u] = False
        assert np.array_equal(sliced["argmax"][good], ref_am[good]), prec


# ------------------------------------------------------------------------------------------------- EM statistics
def _bits_equal(a, b):
    return (np.array_equal(a["nk"], b["nk"]) and np.array_equal(a["sx"], b["sx"]) and np.array_equal(a["sxx"], b["sxx"])
            and a["loglik_sum"] == b["loglik_sum"])


@pytest.mark.parametrize("K,D", [(3, 1), (64, 39), (70, 47), (5, 60)], ids=["K3_D1", "K64_D39", "K70_D47", "K5_D60_valu"])
def test_em_stats_with_a_bad_frame_are_all_nan_and_leave_nothing_behind(api, K, D):
    """both MFMA families (fused log-sum-exp for K <= 64, gmm_em_lse_mfma_kernel's for K > 64) and the VALU path (D > 47)"""
    rng = np.random.default_rng(40 + K)
    n = 64 * 5 + 37
    w, mu, cov = rng.dirichlet(5 * np.ones(K)), rng.standard_normal((K, D)), rng.uniform(0.5, 2.0, (K, D))
    X = (mu[rng.choice(K, size=n, p=w)] + rng.standard_normal((n, D))).astype(np.float32)
    ctx = api.default_context()
    before = api.gmm_em_stats(ctx, w, mu, cov, X)
    nk, sx, sxx, ll = O.gmm_em_stats(w, mu, cov, X)
    assert abs(before["loglik_sum"] - ll) <= 2e-5 * max(1.0, abs(ll))
    assert np.allclose(before["nk"], nk, rtol=2e-4, atol=2e-4 * max(1.0, nk.max()))
    k = 0
    for frame in (0, 63, 64, 319, 320, n - 1):
        for kind in BAD:
            Xb = plant(X, frame, D, kind, k)
            k += 1
            with np.errstate(all="ignore"):
                ref = O.gmm_em_stats(w, mu, cov, Xb)
            assert not any(np.isfinite(v).any() for v in ref)
            st = api.gmm_em_stats(ctx, w, mu, cov, Xb)
            what = (K, D, frame, kind)
            assert np.isnan(st["nk"]).all() and np.isnan(st["sx"]).all() and np.isnan(st["sxx"]).all(), what
            assert np.isnan(st["loglik_sum"]), (what, st["loglik_sum"])
            after = api.gmm_em_stats(ctx, w, mu, cov, X)   # grow-only scratch of the same context: nothing of the bad call is left in it
            assert _bits_equal(before, after), what


def test_em_batch_poisons_only_the_models_whose_rows_hold_the_bad_frame(api):
    """M = 4 over 1000 rows: model 0 rows 300..500, model 1 rows 0..200, model 2 rows 450..700 (overlaps model 0 on 450..500), model 3
    rows 700..1000; rows 200..300 are a gap"""
    rng = np.random.default_rng(77)
    M, K, D = 4, 16, 13
    w = rng.dirichlet(5 * np.ones(K), M)
    mu = rng.standard_normal((M, K, D))
    cov = rng.uniform(0.5, 2.0, (M, K, D))
    X = rng.standard_normal((1000, D)).astype(np.float32)
    off, cnt = np.array([300, 0, 450, 700]), np.array([200, 200, 250, 300])
    ctx = api.default_context()
    clean = api.gmm_em_stats_batch(ctx, w, mu, cov, X, off, cnt)
    single = [api.gmm_em_stats(ctx, w[m], mu[m], cov[m], X[off[m]:off[m] + cnt[m]]) for m in range(M)]
    for m in range(M):   # the header's K <= 64 promise, and the oracle
        assert _bits_equal({k: clean[k][m] for k in ("nk", "sx", "sxx", "loglik_sum")}, single[m]), m
        ll = O.gmm_em_stats(w[m], mu[m], cov[m], X[off[m]:off[m] + cnt[m]])[3]
        assert abs(clean["loglik_sum"][m] - ll) <= 2e-5 * abs(ll)
    k = 0
    for row, poisoned in ((100, {1}), (250, set()), (470, {0, 2}), (199, {1}), (200, set()), (299, set()), (300, {0}), (999, {3})):
        for kind in BAD:
            Xb = plant(X, row, D, kind, k)
            k += 1
            st = api.gmm_em_stats_batch(ctx, w, mu, cov, Xb, off, cnt)
            for m in range(M):
                what = (row, kind, "model", m)
                if m in poisoned:
                    assert np.isnan(st["nk"][m]).all() and np.isnan(st["sx"][m]).all() and np.isnan(st["sxx"][m]).all(), what
                    assert np.isnan(st["loglik_sum"][m]), what
                else:
                    got = {key: st[key][m] for key in ("nk", "sx", "sxx", "loglik_sum")}
                    assert _bits_equal(got, {key: clean[key][m] for key in got}), what
                    assert _bits_equal(got, single[m]), what


# ------------------------------------------------------------------------------------------------- the sklearn-shaped Python layer
def test_python_layer_raises_value_error_like_sklearn(api):
    from speech_signal_processing_amd import GMM_UBM, gmm_train
    rng = np.random.default_rng(9)
    K, D, n = 4, 6, 300
    centres = 3.0 * rng.standard_normal((K, D))
    X = (centres[rng.integers(0, K, n)] + rng.standard_normal((n, D))).astype(np.float32)
    kw = dict(n_components=K, random_state=3, max_iter=20)
    fresh = gmm_train.GaussianMixture(**kw).fit(X)
    for kind, v in BAD.items():
        Xb = X.copy()
        Xb[123, 2] = v
        gm = gmm_train.GaussianMixture(**kw)
        with pytest.raises(ValueError, match=r"row 123\b"):
            gm.fit(Xb)
        assert not hasattr(gm, "weights_") and not hasattr(gm, "converged_"), kind
        gm.fit(X)   # the next clean fit: the bits of a fit on a fresh object
        for attr in ("weights_", "means_", "covariances_", "lower_bound_", "n_iter_", "converged_"):
            assert np.array_equal(getattr(gm, attr), getattr(fresh, attr)), (kind, attr)
        with pytest.raises(ValueError, match=r"row 123\b"):
            fresh.score_samples(Xb)
        with pytest.raises(ValueError, match="NaN, infinity"):
            fresh.score(Xb)
        # fit_many: the bad model in the middle of the list is named, no model comes back
        with pytest.raises(ValueError, match=r"model 1\b.*row 123\b"):
            gmm_train.fit_many([X[:200], Xb, X[100:]], **kw)
        # score_matrix (GMM, identify_language and identify_with_confidence go through it)
        feats = [X[:50].astype(np.float64), Xb[100:150].astype(np.float64), np.zeros((0, D)), X[200:].astype(np.float64)]
        with pytest.raises(ValueError, match=r"utterance 1\b"):
            GMM_UBM.score_matrix([fresh, fresh], fresh, feats)
        with pytest.raises(ValueError, match=r"utterance 0\b"):
            GMM_UBM.identify_with_confidence([fresh, fresh], fresh, feats[1])
    ref = np.array(fresh.score_samples(X))
    assert np.isfinite(ref).all() and np.isfinite(fresh.score(X))
    many = gmm_train.fit_many([X[:200], X, X[100:]], **kw)
    assert np.array_equal(many[1].means_, fresh.means_)
    pred, am = GMM_UBM.score_matrix([fresh, many[0]], fresh, [X[:50], np.zeros((0, D)), X[200:]])   # an empty utterance keeps its NaN row
    assert np.isnan(pred[1]).all() and am[1] == 0 and np.isfinite(pred[[0, 2]]).all()
    # the library calls themselves stay IEEE: NaN, no exception
    Xb = X.copy()
    Xb[5, 0] = np.nan
    ctx = api.default_context()
    st = api.gmm_em_stats(ctx, fresh.weights_, fresh.means_, fresh.covariances_, Xb)
    assert np.isnan(st["loglik_sum"])
    sc = api.GmmScorer.from_sklearn(ctx, [fresh, fresh], fresh)
    r = sc.score_list([Xb[:50], X[50:]])
    assert np.isnan(r["scores"][0]).all() and r["argmax"][0] == 0 and np.isfinite(r["scores"][1]).all()


# ------------------------------------------------------------------------------------------------- end to end
def test_a_silent_stretch_travels_from_the_front_end_to_the_scorer(api):
    """a 700-sample zeroed stretch (longer than one 400-sample window) is a digitally silent frame: the sidekit dialect hands it on as
    NaN rows, delta spreads them, scale keeps them in place — and the scorer answers that utterance with a NaN row, score_matrix with
    ValueError"""
    from speech_signal_processing_amd import GMM_UBM
    rng = np.random.default_rng(SEEDS["e2e"])
    sigs = [(0.3 * rng.standard_normal(16000)).astype(np.float32) for _ in range(5)]
    sigs[2][6000:6700] = 0.0
    feats, _ = GMM_UBM.extract_feature(sigs, list(range(5)))
    D = feats[0].shape[1]
    for u, f in enumerate(feats):
        rows = ~np.isfinite(f).all(axis=1)
        assert rows.any() == (u == 2), (u, int(rows.sum()))
    assert 0 < (~np.isfinite(feats[2]).all(axis=1)).sum() < feats[2].shape[0]
    K, S = 8, 3
    w = rng.dirichlet(5 * np.ones(K))
    mu, cov = rng.standard_normal((K, D)), rng.uniform(0.5, 2.0, (K, D))
    mus = np.stack([mu] + [mu + 0.2 * np.sqrt(cov) * rng.standard_normal((K, D)) for _ in range(S)])
    ws, covs = np.stack([w] * (S + 1)), np.stack([cov] * (S + 1))
    ok = [u for u in range(5) if u != 2]
    ref = np.array([[O.gmm_score(w, m, cov, feats[u].astype(np.float32)) for m in mus] for u in ok])
    ref_am = check_precondition(ref, True, [f.shape[0] for f in (feats[u] for u in ok)])
    sc = api.GmmScorer(api.default_context(), ws, mus, covs, has_ubm=True)
    r = sc.score_list(feats)
    assert np.isnan(r["scores"][2]).all() and r["argmax"][2] == 0
    assert np.array_equal(r["argmax"][ok], ref_am)
    assert (np.abs(r["scores"][ok] - ref) <= SCORE_RTOL * np.abs(ref)).all()

    class Mdl:  # duck-typed fitted GaussianMixture
        covariance_type = "diag"

        def __init__(self, m):
            self.weights_, self.means_, self.covariances_ = w, m, cov
    with pytest.raises(ValueError, match=r"utterance 2\b"):
        GMM_UBM.score_matrix([Mdl(m) for m in mus[1:]], Mdl(mus[0]), feats)
    pred, am = GMM_UBM.score_matrix([Mdl(m) for m in mus[1:]], Mdl(mus[0]), [feats[u] for u in ok])
    assert np.array_equal(am, ref_am)
