"""Float64 restatement of the i-vector model that specifies ssp_ivector_* (include/ssp.h), api.IvectorExtractor and
ivector.TotalVariability: numpy only, np.linalg.cholesky / solve, statistics from exact float64 responsibilities.  sidekit
(FactorAnalyser.total_variability / extract_ivectors) is not a dependency, so this file is the yardstick; tests/test_ivector_host.py holds
it to brute-force Gaussian conditioning and to EM's monotonicity."""
import functools

import numpy as np

# (K, D, R, U, frame lengths cycled over the utterances): the smallest shapes at which each kernel can go wrong
CASES = {
    "tiny": (5, 3, 3, 7, (40, 0, 1, 60)),          # everything below one tile; an empty utterance; a one-frame utterance
    "odd": (24, 13, 20, 37, (98, 30, 0, 298)),     # R and K no multiples of 16; the triangle length no multiple of the tile
    "chunks": (70, 39, 64, 65, (298, 98)),         # a padded second K chunk; U crosses a 64-row tile
    "lds": (8, 13, 256, 3, (298,)),                # the LDS limit
    "rank1": (8, 13, 1, 3, (50,)),                 # R = 1
    # beyond the issue's list: a GEMM's sum over k is cut into chunks of 1024, each one fma chain
    "long_k": (1030, 2, 3, 5, (40,)),              # K > 1024: the precision GEMM has a second chunk (K D > 1024: so has b's)
    "many_utts": (3, 2, 2, 1100, (5, 9)),          # U > 1024: the accumulator GEMMs have a second chunk
}


def recipe(K, D, R, lens, seed, w_true=None):
    """the synthetic recipe: a UBM, a decaying T_true and utterances drawn from the mixture with means mu + T_true w_true"""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(5 * np.ones(K))
    mu = rng.standard_normal((K, D))
    cv = rng.uniform(0.5, 2.0, (K, D))
    T_true = 0.9 * 0.85 ** np.arange(R) * rng.standard_normal((K, D, R))
    Xs, ws = [], []
    for u, n in enumerate(lens):
        wt = rng.standard_normal(R) if w_true is None else np.asarray(w_true[u], dtype=np.float64)
        k = rng.choice(K, size=n, p=w)
        Xs.append((mu + T_true @ wt)[k] + np.sqrt(cv[k]) * rng.standard_normal((n, D)))
        ws.append(wt)
    return {"w": w, "mu": mu, "cv": cv, "T_true": T_true, "Xs": Xs, "w_true": np.array(ws)}


def t0(K, D, R, seed=5, scale=0.1):
    return scale * np.random.default_rng(seed).standard_normal((K, D, R))


def responsibilities(w, mu, cv, X):
    lp = np.log(w)[None] - 0.5 * (np.log(2 * np.pi * cv).sum(axis=1)[None] + (((X[:, None, :] - mu[None]) ** 2) / cv[None]).sum(axis=2))
    lp -= lp.max(axis=1, keepdims=True)
    p = np.exp(lp)
    return p / p.sum(axis=1, keepdims=True)


def stats(w, mu, cv, Xs):
    """-> nk (U, K), sx (U, K, D); an utterance without frames has zeros"""
    K, D = mu.shape
    nk, sx = np.zeros((len(Xs), K)), np.zeros((len(Xs), K, D))
    for u, X in enumerate(Xs):
        if len(X):
            g = responsibilities(w, mu, cv, np.asarray(X, dtype=np.float64))
            nk[u], sx[u] = g.sum(axis=0), g.T @ X
    return nk, sx


def centred(mu, nk, sx):
    return sx - nk[:, :, None] * mu[None]


def precision_terms(cv, T):
    """-> P (K, R, R) = T_k' diag(1/cv_k) T_k and G (K, D, R) = diag(1/cv) T"""
    G = T / cv[:, :, None]
    return np.einsum("kdi,kdj->kij", G, T), G


def posterior(mu, cv, T, nk, sx):
    """-> w (U, R), logdet (U,), quad (U,), Linv (U, R, R)"""
    P, G = precision_terms(cv, T)
    R = T.shape[2]
    L = np.eye(R)[None] + np.einsum("uk,kij->uij", nk, P)
    b = np.einsum("ukd,kdr->ur", centred(mu, nk, sx), G)
    ch = np.linalg.cholesky(L)
    w = np.linalg.solve(L, b[:, :, None])[:, :, 0]
    logdet = 2.0 * np.log(np.diagonal(ch, axis1=1, axis2=2)).sum(axis=1)
    return w, logdet, (b * w).sum(axis=1), np.linalg.inv(L)


def estep(mu, cv, T, nk, sx):
    """-> A (K, R, R), C (K, D, R), objective"""
    w, logdet, quad, Linv = posterior(mu, cv, T, nk, sx)
    S = Linv + w[:, :, None] * w[:, None, :]
    A = np.einsum("uk,uij->kij", nk, S)
    C = np.einsum("ukd,ur->kdr", centred(mu, nk, sx), w)
    return A, C, float((-0.5 * logdet + 0.5 * quad).sum())


def mstep(A, C):
    """T_k = C_k A_k^-1; a mixture no utterance reached keeps a zero block"""
    T = np.zeros_like(C)
    for k in range(len(A)):
        if A[k].any():
            T[k] = np.linalg.solve(A[k], C[k].T).T
    return T


def em(mu, cv, T, nk, sx, n_iter):
    """-> (T after n_iter iterations, the objective of the T each iteration started from)"""
    obj = []
    for _ in range(n_iter):
        A, C, o = estep(mu, cv, T, nk, sx)
        obj.append(o)
        T = mstep(A, C)
    return T, np.array(obj)


def objective(mu, cv, T, nk, sx):
    _, logdet, quad, _ = posterior(mu, cv, T, nk, sx)
    return float((-0.5 * logdet + 0.5 * quad).sum())


def conditioned_mean(cv, T, nk_u, f_u):
    """the posterior mean of w by brute-force Gaussian conditioning on the stacked K D supervector: the per-mixture means
    y_k = f_k / n_k = T_k w + e_k, e_k ~ N(0, diag(cv_k) / n_k), w ~ N(0, I) -> E[w | y] = Ts' (Ts Ts' + Sigma)^-1 y (every n_k > 0)"""
    K, D, R = T.shape
    Ts = T.reshape(K * D, R)
    y = (f_u / nk_u[:, None]).reshape(K * D)
    Sigma = np.diag((cv / nk_u[:, None]).reshape(K * D))
    return Ts.T @ np.linalg.solve(Ts @ Ts.T + Sigma, y)


@functools.lru_cache(maxsize=None)
def case(name):
    """everything the tests share about a case, computed once: the recipe, the float64 statistics, T0, T1 (one float64 EM iteration
    from T0: L is then realistically conditioned) and the oracle's answers under both"""
    K, D, R, U, lens = CASES[name]
    r = recipe(K, D, R, [lens[u % len(lens)] for u in range(U)], seed=sum(map(ord, name)))
    nk, sx = stats(r["w"], r["mu"], r["cv"], r["Xs"])
    T0 = t0(K, D, R)
    T1, _ = em(r["mu"], r["cv"], T0, nk, sx, 1)
    out = {"mu": r["mu"], "cv": r["cv"], "w": r["w"], "nk": nk, "sx": sx, "T0": T0, "T1": T1, "shape": (K, D, R, U)}
    for tag, T in (("T0", T0), ("T1", T1)):
        w, logdet, quad, _ = posterior(r["mu"], r["cv"], T, nk, sx)
        A, C, obj = estep(r["mu"], r["cv"], T, nk, sx)
        out[tag + "_post"] = {"w": w, "logdet": logdet, "quad": quad, "A": A, "C": C, "objective": obj}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def cosine_identify(E, cent):
    """-> (argmin_j cosine distance, margin between the two smallest distances per row)"""
    En = E / np.linalg.norm(E, axis=1, keepdims=True)
    Cn = cent / np.linalg.norm(cent, axis=1, keepdims=True)
    d = 1.0 - En @ Cn.T
    s = np.sort(d, axis=1)
    return d.argmin(axis=1), s[:, 1] - s[:, 0]


def end_to_end(seed, S=4, K=16, D=13, R=8, per=6, frames=200, enrol=3, n_iter=5):
    """the float64 pipeline of the end-to-end test: statistics -> EM -> normalised i-vectors -> centroids of the first ``enrol``
    utterances per speaker -> cosine identification of the rest.  -> dict with the recipe, labels, predictions and the top-2 margins"""
    rng = np.random.default_rng(1000 + seed)
    spk_w = rng.standard_normal((S, R))
    labels = np.repeat(np.arange(S), per)
    r = recipe(K, D, R, [frames] * (S * per), seed=seed, w_true=spk_w[labels])
    nk, sx = stats(r["w"], r["mu"], r["cv"], r["Xs"])
    T, _ = em(r["mu"], r["cv"], t0(K, D, R), nk, sx, n_iter)
    E, _, _, _ = posterior(r["mu"], r["cv"], T, nk, sx)
    E = E / np.linalg.norm(E, axis=1, keepdims=True)
    is_enrol = (np.arange(S * per) % per) < enrol
    cent = np.stack([E[is_enrol & (labels == s)].mean(axis=0) for s in range(S)])
    pred, margin = cosine_identify(E[~is_enrol], cent)
    return {"recipe": r, "labels": labels, "is_enrol": is_enrol, "pred": pred, "margin": margin}
