"""Randomised shapes for the scoring / training / matching kernels against the float64 oracle.  Run on the GPU box."""
import sys, time, numpy as np
sys.path.insert(0, '.')
from speech_signal_processing_amd import api
from oracle import ref_cpu as O
# the derived bound of a float32 DTW against float64 (tests/dtw_cases.py band(), restated; tests/test_dtw_instances_host.py holds the two
# to each other)
dtw_band = lambda r, c, dim, ref: 1.01 * (r + c + (1 if dim == 1 else dim + 3)) * 2.0 ** -24 * abs(ref)
# the derived bound of one float32 dense layer against float64, per output element (tests/dense_cases.py band_of(), restated for one
# layer; tests/test_dense_instances_host.py holds that one): d_in accumulations and the bias add, 2^-23 each, on sum |x| |w| + |b|
dense_band = lambda X, W, b: 1.01 * (W.shape[0] + 1) * 2.0 ** -23 * (np.abs(X.astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64)))

# the one rule of the EM instance suite (tests/em_cases.py compare(), restated: this tool imports nothing from tests/;
# tests/test_em_instances_host.py holds the two to each other).  Float64 oracle; yardstick: a float32 restatement of the kernels' formula
# (em_pack's image, one product at a time, float32 log-sum-exp); errors normalised by the sum of the magnitudes a statistic is made of.
# Returns the largest of the four ratios error / limit: above 1 is a failure.
# ---- em_rule begin
def em_rule(w, mu, cov, X, nk, sx, sxx, ll, n_tiles_cap):
    w, mu, cov = (np.asarray(a, dtype=np.float64) for a in (w, mu, cov))
    X = np.asarray(X, dtype=np.float32)
    (K, D), n = mu.shape, len(X)
    X64 = X.astype(np.float64)
    lp = O.gmm_log_prob(w, mu, cov, X64)
    mx = lp.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(lp - mx).sum(axis=1, keepdims=True)))[:, 0]
    resp = np.exp(lp - lse[:, None])
    aug = np.concatenate([X64, X64 * X64, np.ones((n, 1))], axis=1)
    ref, den = resp.T @ aug, resp.T @ np.abs(aug) + 2.0 ** -100 * np.abs(aug).sum(axis=0)[None, :]
    P = 1.0 / cov
    c = np.log(w) - 0.5 * D * np.log(2.0 * np.pi)
    for d in range(D):
        c = c + (0.5 * np.log(P[:, d]) - 0.5 * mu[:, d] * mu[:, d] * P[:, d])
    W = np.zeros(((K + 63) // 64 * 64, 2 * D + 1))   # with the padded mixtures of the image: constant -1e30
    W[:, 2 * D] = -1.0e30
    W[:K] = np.concatenate([mu * P, -0.5 * P, c[:, None]], axis=1)
    W = W.astype(np.float32)
    a32 = np.concatenate([X, X * X, np.ones((n, 1), np.float32)], axis=1)
    acc = np.zeros((n, len(W)), dtype=np.float32)
    for j in range(2 * D + 1):
        acc = acc + a32[:, j:j + 1] * W[None, :, j]
    m32 = acc.max(axis=1, keepdims=True)
    l32 = m32[:, 0] + np.log(np.exp(acc - m32).sum(axis=1, dtype=np.float32))
    emu = np.exp(acc - l32[:, None]).astype(np.float64)[:, :K].T @ a32.astype(np.float64)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v)))) if np.size(v) else 0.0
    e = lambda v: np.abs(v - ref) / den
    n_tiles = (n + 63) // 64
    G = min(n_tiles, n_tiles_cap)
    L = 64 * ((n_tiles + G - 1) // G)
    got = np.concatenate([sx, sxx, np.asarray(nk)[:, None]], axis=1).astype(np.float64)
    lim_max = 8.0 * float(e(emu).max()) + 2.0 ** -20 + L * 2.0 ** -24
    ratios = [float(e(got).max()) / lim_max, abs(float(got[:, -1].sum()) - n) / (n * lim_max)]
    rows = ref[:, -1] >= 8.0
    if int(rows.sum()) >= 4:
        ratios.append(rms(e(got)[rows]) / (3.0 * rms(e(emu)[rows]) + 2.0 ** -22))
    dl = l32.astype(np.float64) - lse
    ratios.append(abs(float(ll) - float(lse.sum())) / (8.0 * max(abs(float(dl.sum())), np.sqrt(n) * rms(dl)) + 2.0 ** -22 * float((np.abs(lse) + 1).sum())))
    return max(ratios)
# ---- em_rule end
em_chunks = lambda K: (K + 63) // 64   # the walker cap as csrc/gmm_em.hip takes it: 2 CUs' worth, shared among the chunks when batched

ctx = api.default_context()
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 30
# non-finite rows (include/ssp.h, ssp_gmm_score / ssp_gmm_em_stats): with probability 1/4 a GMM or EM case carries ONE bad entry — NaN, +inf
# or -inf — drawn from a stream of its own, so the shapes of a seed stay what they were
rng_bad = np.random.default_rng([0x6ad, int(sys.argv[1]) if len(sys.argv) > 1 else 0])
BAD_VALUES = (np.nan, np.inf, -np.inf)
verbose = '-v' in sys.argv
import torch
ctx_num_cu = torch.cuda.get_device_properties(0).multi_processor_count   # the walker cap of the EM kernels
t_start = time.time()
for case in range(n_cases):
    # ---- GMM scoring
    K = int(rng.choice([1, 2, 5, 16, 31, 32, 33, 64, 100, 257]))
    D = int(rng.choice([1, 2, 7, 13, 26, 39, 40, 64, 65, 100]))
    M = int(rng.integers(1, 6))
    has_ubm = bool(rng.integers(0, 2)) and M >= 2
    lens = [int(x) for x in rng.choice([0, 1, 2, 63, 64, 65, 255, 256, 257, 1000], int(rng.integers(1, 7)))]
    if verbose:
        print(case, "gmm", K, D, M, has_ubm, lens, flush=True)
    w = rng.dirichlet(5 * np.ones(K), M)
    mu = rng.standard_normal((M, K, D))
    cov = rng.uniform(0.5, 2.0, (M, K, D))
    X = rng.standard_normal((sum(lens), D)).astype(np.float32)
    seg = api.Segments.from_lengths(ctx, lens)
    sc = api.GmmScorer(ctx, w, mu, cov, has_ubm=has_ubm)
    off = np.concatenate([[0], np.cumsum(lens)])
    bad_f = bad_u = -1
    Xc = X
    if rng_bad.random() < 0.25 and len(X):
        bad_f = int(rng_bad.integers(0, len(X)))
        bad_u = int(np.searchsorted(off, bad_f, side="right")) - 1
        X = X.copy()
        X[bad_f, int(rng_bad.integers(0, D))] = BAD_VALUES[int(rng_bad.integers(0, 3))]
        if verbose:
            print(case, "gmm bad entry: frame", bad_f, "utterance", bad_u, flush=True)
    for prec in ((0, 1) if D <= 64 else (0,)):
        r = sc.score(X, seg, loglik=True, scores=True, argmax=True, precision=prec)
        ll = np.asarray(r["loglik"])
        ok = np.arange(len(X)) != bad_f
        for m in range(M):
            ref = O.gmm_score_samples(w[m], mu[m], cov[m], Xc) if len(X) else np.zeros(0)
            assert np.allclose(ll[m][ok], ref[ok], rtol=2e-4, atol=2e-4), (case, "loglik", K, D, m, prec, np.abs(ll[m][ok] - ref[ok]).max())
        for u, L in enumerate(lens):
            if L == 0 or u == bad_u:
                continue
            refs = np.array([O.gmm_score(w[m], mu[m], cov[m], X[off[u]:off[u + 1]]) for m in range(M)])
            assert np.allclose(np.asarray(r["scores"])[u], refs, rtol=2e-4, atol=2e-4), (case, "score", u, prec)
        if bad_f >= 0:
            # rule 1: NaN exactly in the bad frame's column; rule 2: the bad utterance's row is NaN, arg-max 0; rule 3: nobody else moves
            # (precision 0: bit for bit against the same call on the clean batch; precision 1: the tolerances above, and the fp32 arg-max)
            assert np.isnan(ll[:, bad_f]).all() and np.isfinite(ll[:, ok]).all(), (case, "bad frame", K, D, prec, bad_f)
            assert np.isnan(np.asarray(r["scores"])[bad_u]).all() and np.asarray(r["argmax"])[bad_u] == 0, (case, "bad utterance", prec, bad_u)
            rc = sc.score(Xc, seg, loglik=True, scores=True, argmax=True, precision=0)
            good = (np.array(lens) > 0) & (np.arange(len(lens)) != bad_u)
            if prec == 0:
                assert np.array_equal(ll[:, ok], np.asarray(rc["loglik"])[:, ok]), (case, "a clean frame changed", K, D)
                assert np.array_equal(np.asarray(r["scores"])[good], np.asarray(rc["scores"])[good]), (case, "a clean utterance changed", K, D)
            # (the arg-max promise of precision 1 belongs to calls without loglik: those list the close calls and the bad utterance)
            rf = r if prec == 0 else sc.score(X, seg, precision=prec)
            assert np.isnan(np.asarray(rf["scores"])[bad_u]).all() and np.asarray(rf["argmax"])[bad_u] == 0, (case, "bad utterance", prec, bad_u)
            assert np.array_equal(np.asarray(rf["argmax"])[good], np.asarray(rc["argmax"])[good]), (case, "a clean arg-max changed", prec)
            assert prec == 0 or M - int(has_ubm) < 2 or sc.last_rescored >= 1, (case, "bad utterance not listed", prec)
    X = Xc
    # ---- the split-precision modes keep the fp32 path's arg-max (proven band: precision 1; calibrated band: 3), speakers a hair apart
    if D <= 64 and M - int(has_ubm) >= 2 and sum(lens) > 0:
        mu2 = mu.copy()
        for m in range(int(has_ubm) + 1, M):
            mu2[m] = mu2[int(has_ubm)] * (1.0 + 10.0 ** rng.uniform(-7, -2) * rng.standard_normal((K, D)))
        sc2 = api.GmmScorer(ctx, np.repeat(w[:1], M, 0), mu2, np.repeat(cov[:1], M, 0), has_ubm=has_ubm)
        a0 = np.asarray(sc2.score(X, seg, precision=0)["argmax"])
        for prec in (1, 3):
            a1 = np.asarray(sc2.score(X, seg, precision=prec)["argmax"])
            nz = np.array(lens) > 0
            assert np.array_equal(a0[nz], a1[nz]), (case, "gmm split-precision arg-max", prec, K, D, M)
    # ---- cosine
    N, S, d = int(rng.choice([1, 31, 32, 33, 500])), int(rng.choice([1, 2, 31, 32, 33, 129, 300])), int(rng.choice([1, 3, 64, 128, 255, 256, 257, 512]))
    if verbose:
        print(case, "cos", N, S, d, flush=True)
    Cn = rng.standard_normal((S, d)).astype(np.float32)
    Xc = rng.standard_normal((N, d)).astype(np.float32)
    rc = api.cosine_identify(ctx, Xc, Cn, dist=True)
    refd = O.cosine_matrix(Xc, Cn)
    assert np.abs(np.asarray(rc["dist"]) - refd).max() < 2e-5, (case, "cos", N, S, d)
    # arg-min: exact unless the two best are within float noise
    am = np.asarray(rc["argmin"])
    srt = np.sort(refd, axis=1)
    clear = (srt[:, 1] - srt[:, 0] > 1e-5) if S > 1 else np.ones(N, bool)
    assert (am[clear] == refd.argmin(1)[clear]).all(), (case, "argmin")
    if d <= 256:  # split precision (bf16x3; the cascade with a bf16 sweep in front): the fp32 path's arg-min on every row, close calls included
        Cc = Cn.copy()
        if S >= 2:
            Cc[1::2] = Cc[0::2][: len(Cc[1::2])] * (1.0 + 10.0 ** rng.uniform(-8, -2) * rng.standard_normal(Cc[1::2].shape).astype(np.float32))
        a0 = np.asarray(api.cosine_identify(ctx, Xc, Cc)["argmin"])
        for prec in (1, 2):
            assert np.array_equal(a0, np.asarray(api.cosine_identify(ctx, Xc, Cc, precision=prec)["argmin"])), (case, "cosine split-precision arg-min", prec, N, S, d)
    # ---- dense
    Nn, di, un = int(rng.choice([1, 5, 127, 128, 129, 300])), int(rng.choice([1, 2, 31, 32, 33, 100, 1274])), int(rng.choice([1, 3, 127, 128, 129, 256]))
    if verbose:
        print(case, "dense", Nn, di, un, flush=True)
    Xd = rng.standard_normal((Nn, di)).astype(np.float32)
    Wd = (rng.standard_normal((di, un)) / np.sqrt(di)).astype(np.float32)
    bd = rng.standard_normal(un).astype(np.float32)
    relu_d = bool(rng.integers(0, 2))
    yd = api.dense_forward(ctx, Xd, np.ascontiguousarray(Wd.T), bd, relu=relu_d)
    err_d = np.abs(yd - O.dense_net_forward(Xd, [(Wd, bd, 'relu' if relu_d else 'linear')]))
    assert (err_d <= dense_band(Xd, Wd, bd)).all(), (case, "dense", Nn, di, un, relu_d, float((err_d / dense_band(Xd, Wd, bd)).max()))
    # ---- EM statistics
    Ke, De, ne = int(rng.choice([1, 3, 64, 65, 130])), int(rng.choice([1, 5, 13, 39, 47, 48, 64])), int(rng.choice([1, 63, 64, 65, 1000, 5000]))
    if verbose:
        print(case, "em", Ke, De, ne, flush=True)
    we = rng.dirichlet(5 * np.ones(Ke)); mue = rng.standard_normal((Ke, De)); cve = rng.uniform(0.5, 2.0, (Ke, De))
    Xe = rng.standard_normal((ne, De)).astype(np.float32)
    if rng_bad.random() < 0.25:   # a bad entry: every statistic is NaN, and the clean call right after it is untouched by it
        Xb = Xe.copy()
        Xb[int(rng_bad.integers(0, ne)), int(rng_bad.integers(0, De))] = BAD_VALUES[int(rng_bad.integers(0, 3))]
        sb = api.gmm_em_stats(ctx, we, mue, cve, Xb)
        assert all(np.isnan(sb[k]).all() for k in ("nk", "sx", "sxx")) and np.isnan(sb["loglik_sum"]), (case, "em bad entry", Ke, De, ne)
    st = api.gmm_em_stats(ctx, we, mue, cve, Xe)
    nk, sx, sxx, ll = O.gmm_em_stats(we, mue, cve, Xe)
    assert abs(st["loglik_sum"] - ll) <= 2e-5 * max(1.0, abs(ll)), (case, "em ll", Ke, De, ne)
    assert np.allclose(st["nk"], nk, rtol=2e-4, atol=2e-4 * max(1.0, nk.max())), (case, "em nk")
    assert np.allclose(st["sx"], sx, rtol=2e-4, atol=2e-4 * max(1.0, np.abs(sx).max())), (case, "em sx")
    assert np.allclose(st["sxx"], sxx, rtol=2e-4, atol=2e-4 * max(1.0, np.abs(sxx).max())), (case, "em sxx")
    # ---- EM statistics under the instance suite's rule: own shapes, every model its own draw, the single call and (D <= 47) the batched one
    Kr, Dr, nr = int(rng.choice([1, 5, 33, 64, 65, 129, 300])), int(rng.choice([1, 3, 13, 16, 31, 39, 47, 48, 64])), int(rng.choice([1, 64, 65, 209, 1000, 40000]))
    if verbose:
        print(case, "em rule", Kr, Dr, nr, flush=True)
    wr = rng.dirichlet(5 * np.ones(Kr)); cvr = rng.uniform(0.5, 2.0, (Kr, Dr)); mur = rng.standard_normal((Kr, Dr))
    Xr = (mur[rng.choice(Kr, nr, p=wr)] + rng.standard_normal((nr, Dr))).astype(np.float32)
    st = api.gmm_em_stats(ctx, wr, mur, cvr, Xr)
    ratio = em_rule(wr, mur, cvr, Xr, st["nk"], st["sx"], st["sxx"], st["loglik_sum"], 2 * ctx_num_cu)
    assert ratio <= 1.0, (case, "em rule single", Kr, Dr, nr, ratio)
    if Dr <= 47:
        Xp = np.concatenate([np.full((5, Dr), 50.0, np.float32), Xr])
        sb = api.gmm_em_stats_batch(ctx, wr[None], mur[None], cvr[None], Xp, [5], [nr])
        cap = 2 * ctx_num_cu if em_chunks(Kr) == 1 else max(1, 2 * ctx_num_cu // em_chunks(Kr))
        ratio = em_rule(wr, mur, cvr, Xr, sb["nk"][0], sb["sx"][0], sb["sxx"][0], sb["loglik_sum"][0], cap)
        assert ratio <= 1.0, (case, "em rule batch", Kr, Dr, nr, ratio)
    # ---- DTW
    dim = int(rng.choice([1, 1, 2, 13]))
    ql = [int(x) for x in rng.choice([1, 2, 63, 64, 65, 200, 700], int(rng.integers(1, 4)))]
    tl = [int(x) for x in rng.choice([1, 3, 255, 256, 257, 300, 1100, 2100], int(rng.integers(1, 4)))]
    if verbose:
        print(case, "dtw", dim, ql, tl, flush=True)
    mk = lambda L: (rng.standard_normal((L, dim)) if dim > 1 else rng.standard_normal(L)).astype(np.float32)
    Q, T = [mk(L) for L in ql], [mk(L) for L in tl]
    got = api.dtw_distances(ctx, Q, T)
    ref = np.array([[O.dtw_distance(q, t) for t in T] for q in Q])
    tol = np.array([[dtw_band(len(q), len(t), dim, ref[a, b]) for b, t in enumerate(T)] for a, q in enumerate(Q)])  # the derived float32 bound
    assert (np.abs(got - ref) <= tol).all(), (case, "dtw", dim, ql, tl, float((np.abs(got - ref) / tol).max()))
print("fuzz_scoring OK: %d cases, %.1f s" % (n_cases, time.time() - t_start))
