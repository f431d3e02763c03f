"""Restatement in float64 numpy of MAP adaptation of a diagonal GMM-UBM (Reynolds, Quatieri, Dunn 2000) and of top-C fast scoring of
mean-adapted speaker models, for the tests of gmm_train.map_adapt and api.MapScorer.  Test code only: the package never imports it.
The reference has neither (it trains every speaker's mixture independently, GMM_UBM.py:158-170, and scores every mixture,
GMM_UBM.py:181-197); all quantities are sklearn's (mixture/_gaussian_mixture.py:453-512).

    lp_k(x)   = log w_k + log N(x; mu_k, diag cv_k)                     weighted log-probability of mixture k under the UBM
    resp_k(x) = exp(lp_k(x) - logsumexp_k lp_k(x))
    n = sum_t resp, Ex = sum_t resp x / n, Exx = sum_t resp x^2 / n,  alpha = n / (n + r)
      'm'  mu^ = alpha Ex + (1 - alpha) mu
      'w'  w^  = alpha n / T + (1 - alpha) w, renormalised to sum 1
      'v'  cv^ = alpha Exx + (1 - alpha) (cv + mu^2) - mu^^2, floored at reg_covar   (mu^: the model's own mean, adapted or not)
    a mixture with n = 0 keeps the UBM's values.

    T(x) = the C mixtures of largest lp_k(x), of equal values the lower index first
    delta_{s,k}(x) = x . a_{s,k} - b_{s,k},  a = (mu_s - mu) P,  b = 1/2 sum_d (mu_s^2 - mu^2) P,  P = 1 / cv
    L_ubm(x) = logsumexp_{k in T} lp_k,  L_s(x) = logsumexp_{k in T} (lp_k + delta_{s,k})
    diff[u, s] = mean_t (L_s - L_ubm),  ubm[u] = mean_t L_ubm"""
import numpy as np


def weighted_log_prob(w, mu, cv, X):
    """lp (T, K) float64; a zero weight gives -inf (the mixture does not exist)"""
    w, mu, cv, X = (np.asarray(v, dtype=np.float64) for v in (w, mu, cv, X))
    P = 1.0 / cv
    D = mu.shape[1]
    quad = (X * X) @ P.T - 2.0 * X @ (mu * P).T + (mu * mu * P).sum(1)[None]
    with np.errstate(divide="ignore"):
        return np.log(w)[None] - 0.5 * (D * np.log(2.0 * np.pi) - np.log(P).sum(1)[None] + quad)


def _lse(a, axis):
    m = a.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def responsibilities(w, mu, cv, X):
    lp = weighted_log_prob(w, mu, cv, X)
    return np.exp(lp - _lse(lp, 1)[:, None])


def stats(w, mu, cv, X):
    """(nk (K,), sx (K, D), sxx (K, D)) of the rows X under the model"""
    X = np.asarray(X, dtype=np.float64)
    r = responsibilities(w, mu, cv, X)
    return r.sum(0), r.T @ X, r.T @ (X * X)


def adapt_from_stats(w, mu, cv, nk, sx, sxx, T, relevance_factor=16.0, adapt="m", reg_covar=1e-6):
    """the adaptation formulas on given statistics of ONE speaker -> (weights, means, covariances); what ``adapt`` leaves out is the UBM's"""
    w, mu, cv, nk, sx, sxx = (np.asarray(v, dtype=np.float64) for v in (w, mu, cv, nk, sx, sxx))
    r = float(relevance_factor)
    K = w.shape[0]
    alpha = np.zeros(K)
    Ex, Exx = mu.copy(), cv + mu * mu
    for k in range(K):
        if nk[k] > 0.0:
            alpha[k] = 0.0 if np.isinf(r) else (1.0 if r == 0.0 else nk[k] / (nk[k] + r))
            Ex[k] = sx[k] / nk[k]
            Exx[k] = sxx[k] / nk[k]
    a = alpha[:, None]
    m_new = a * Ex + (1.0 - a) * mu if "m" in adapt else mu
    w_new = w
    if "w" in adapt:
        w_new = alpha * nk / float(T) + (1.0 - alpha) * w
        w_new = w_new / w_new.sum()
    v_new = cv
    if "v" in adapt:
        v_new = np.maximum(a * Exx + (1.0 - a) * (cv + mu * mu) - m_new ** 2, reg_covar)
        v_new[nk == 0.0] = cv[nk == 0.0]  # (kept, not recomputed: (cv + mu^2) - mu^2 rounds)
    return w_new, m_new, v_new


def map_adapt(w, mu, cv, X, relevance_factor=16.0, adapt="m", reg_covar=1e-6):
    nk, sx, sxx = stats(w, mu, cv, X)
    return adapt_from_stats(w, mu, cv, nk, sx, sxx, len(X), relevance_factor, adapt, reg_covar)


def select(lp, C):
    """-> (idx (T, C) in rank order, gap (T,) = lp_(C) - lp_(C+1), +inf when C = K): larger value first, of equal values the lower index"""
    order = np.argsort(-lp, axis=1, kind="stable")
    srt = np.take_along_axis(lp, order, 1)
    gap = srt[:, C - 1] - srt[:, C] if C < lp.shape[1] else np.full(lp.shape[0], np.inf)
    return order[:, :C], gap


def rank_gap(lp, C):
    """the smallest difference between two neighbours among the C + 1 largest lp of every frame (the gap of ``select`` is the last of them):
    what decides whether the ORDER inside T(x) is resolved, not only its membership"""
    srt = -np.sort(-lp, axis=1)[:, :min(C + 1, lp.shape[1])]
    return (srt[:, :-1] - srt[:, 1:]).min(axis=1) if srt.shape[1] > 1 else np.full(lp.shape[0], np.inf)


def topc_scores(w, mu, cv, spk_means, X, offsets, C, idx=None):
    """-> dict(diff (U, S), ubm (U,), idx (F, C), gap (F,), rank_gap (F,), lp (F, K), frame_diff (F, S)).  ``idx``: a selection to impose (rows of -1 are
    ignored and replaced by the oracle's own); the gap is always that of the oracle's own selection.  An empty utterance: NaN."""
    w, mu, cv, X = (np.asarray(v, dtype=np.float64) for v in (w, mu, cv, X))
    sm = np.asarray(spk_means, dtype=np.float64)
    lp = weighted_log_prob(w, mu, cv, X)
    own, gap = select(lp, C)
    if idx is None:
        idx = own
    else:
        idx = np.where(np.asarray(idx) < 0, own, np.asarray(idx))
    P = 1.0 / cv
    lpT = np.take_along_axis(lp, idx, 1)                       # (F, C)
    lam = _lse(lpT, 1)
    F, S = X.shape[0], sm.shape[0]
    fd = np.empty((F, S))
    for s in range(S):
        a = (sm[s] - mu) * P                                   # (K, D)
        b = 0.5 * ((sm[s] ** 2 - mu ** 2) * P).sum(1)          # (K,)
        delta = np.einsum("fd,fcd->fc", X, a[idx]) - b[idx]    # (F, C)
        fd[:, s] = _lse(lpT + delta, 1) - lam
    off = np.asarray(offsets)
    U = len(off) - 1
    diff, ubm = np.full((U, S), np.nan), np.full(U, np.nan)
    for u in range(U):
        if off[u + 1] > off[u]:
            diff[u] = fd[off[u]:off[u + 1]].mean(0)
            ubm[u] = lam[off[u]:off[u + 1]].mean()
    return {"diff": diff, "ubm": ubm, "idx": idx, "gap": gap, "rank_gap": rank_gap(lp, C), "lp": lp, "frame_diff": fd}
