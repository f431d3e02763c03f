"""Cases, references and the comparison rule of tests/test_gmm_full_host.py and tests/test_gmm_full_gpu.py: the full-covariance GMM entry
points (csrc/gmm_full.hip: ssp_gmm_full_em_stats, ssp_gmm_full_score) against float64.

The definitions are sklearn's (mixture/_gaussian_mixture.py, restated in include/ssp.h): a model is weights (K,), means (K, D) and the
upper-triangular precisions_cholesky U (K, D, D);  y = (x - mu) U,  lp = log w - (D log 2 pi + sum y^2) / 2 + sum log diag U,
lse = logsumexp_k lp,  resp = exp(lp - lse);  the statistics are taken about a shift c, x' = x - c.

Three evaluations of one model over frames X (float32):
  ref64      the definitions in float64 numpy, with the sums of magnitudes s[k] = sum_t resp_tk |a_t| |a_t|^T, a = [1, x'], that every
             entry of the block [[nk, sx], [sx^T, sxx]] is made of (cancellation inside sx and sxx does not hide an error), and
             A = sum_t |a_t| |a_t|^T.
  emu32      the YARDSTICK: the same formula in plain float32 — the image [-(mu - c) U ; U] and the constant formed in float64 and rounded
             to float32, the shift subtracted in float32, the D + 1 products of every y_j added one at a time in float32 (constant row
             first), the squares added one at a time, a float32 log-sum-exp and resp = exp(lp - lse) in float32, the sums over the frames
             in float64.
  emu32_alt  another legitimate order: columns reversed, the products added in exactly formed pairs rounded once per pair, exp2 / log2,
             resp = e / sum.  The host file holds it to HALF of every limit: the rule has room for a kernel and none for a fault.

The rule is tests/em_cases.py's, carried over to the block: den = s + 2^-100 A, e(v) = |v - ref64| / den per entry;
  max     max e(got) <= 8 max e(emu32) + 2^-20 + L 2^-24           L: the most frames one float32 accumulator adds (acc_frames restates
          the launcher of csrc/gmm_full.hip)
  rms     rms e(got) <= 3 rms e(emu32) + 2^-22                      over the mixtures with nk >= 8 (skipped below 4 such mixtures)
  loglik  |got - ref| <= 8 max(|sum_t d_t|, sqrt(n) rms_t d_t) + 2^-22 sum_t (|lse_ref[t]| + 1),  d = lse_emu32 - lse_ref
  mass    |sum_k nk - n| <= n (8 max e(emu32) + 2^-20 + L 2^-24)
The scorer's per-frame log-likelihood uses tests/gmm_cases.py's compare with ref64 and emu32 of this file.  The factors are the
project's; none is tuned on the code under test.  compare returns the measured ratios.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gmm_cases as GC  # noqa: E402  (the scorer's rule)

PAD_CONST = -1.0e30
LOG2E_F32 = np.float32(1.4426950408889634)
LN2_F32 = np.float32(0.6931471805599453)
MAX_D = 64
E_TILE, M_TILE, MIX_PER_WG, CAP_TILES = 256, 64, 4, 128   # csrc/gmm_full.hip: FG_TF, FG_MT, FG_MW, FG_CAP_TILES
NUM_CU_DEFAULT = 256
BUDGET_ENV = "SSP_GMM_FULL_SCRATCH_MB"
MAX_FACTOR, RMS_FACTOR = 8.0, 3.0
RMS_MIN_NK, RMS_MIN_MIX = 8.0, 4


# ------------------------------------------------------------------------------------------------- the launcher, restated
def slab_frames(n, K, budget_mb=256):
    slab = (budget_mb << 20) // (4 * K) // E_TILE * E_TILE
    return max(E_TILE, min(slab, (n + E_TILE - 1) // E_TILE * E_TILE))


def acc_frames(n, K, num_cu=NUM_CU_DEFAULT, budget_mb=256):
    """L of the rule: 64 ceil(n_tiles / G) of the largest slab, G = max(ceil(n_tiles / 128), min(n_tiles, 2 num_cu / ceil(K / 4)))"""
    ns = min(n, slab_frames(n, K, budget_mb))
    n_tiles = (ns + M_TILE - 1) // M_TILE
    want = max(1, 2 * num_cu // ((K + MIX_PER_WG - 1) // MIX_PER_WG))
    G = max((n_tiles + CAP_TILES - 1) // CAP_TILES, min(n_tiles, want))
    return M_TILE * ((n_tiles + G - 1) // G)


# ------------------------------------------------------------------------------------------------- references
def prec_chol_of(cov):
    """sklearn's _compute_precision_cholesky ('full') in numpy float64"""
    cov = np.asarray(cov, dtype=np.float64)
    out = np.empty_like(cov)
    for k in range(len(cov)):
        out[k] = np.linalg.inv(np.linalg.cholesky(cov[k])).T
    return np.triu(out)


def image64(w, mu, U, shift=None):
    """(B (K, D + 1, D), cst (K,)) in float64: row 0 = -(mu - c) U, rows 1.. = triu(U); a zero weight's constant is PAD_CONST"""
    w, mu, U = (np.asarray(a, dtype=np.float64) for a in (w, mu, U))
    K, D = mu.shape
    c = np.zeros(D) if shift is None else np.asarray(shift, dtype=np.float64)
    Ut = np.triu(U)
    B = np.concatenate([-np.einsum("kd,kdj->kj", mu - c[None], Ut)[:, None, :], Ut], axis=1)
    with np.errstate(divide="ignore"):
        cst = np.log(w) - 0.5 * D * np.log(2.0 * np.pi) + np.log(np.diagonal(Ut, axis1=1, axis2=2)).sum(axis=1)
    return B, np.where(w > 0, cst, PAD_CONST)


def _block(resp, a1):
    """(K, (D + 1)^2): sum_t resp_tk a_t a_t^T in float64, a = [1, x']"""
    n, W = a1.shape
    outer = (a1[:, :, None] * a1[:, None, :]).reshape(n, W * W)
    return np.asarray(resp, dtype=np.float64).T @ outer


def ref64_lp(w, mu, U, X):
    """(n, K) float64 weighted log-probabilities (_estimate_weighted_log_prob); a zero weight is -inf"""
    X64 = np.asarray(np.asarray(X, dtype=np.float32), dtype=np.float64)
    w, mu, U = (np.asarray(a, dtype=np.float64) for a in (w, mu, U))
    K, D = mu.shape
    Ut = np.triu(U)
    lp = np.empty((X64.shape[0], K))
    with np.errstate(divide="ignore"):
        for k in range(K):
            y = (X64 - mu[k]) @ Ut[k]
            lp[:, k] = np.log(w[k]) - 0.5 * (D * np.log(2.0 * np.pi) + (y * y).sum(axis=1)) + np.log(np.diag(Ut[k])).sum()
    return lp


def _lse64(lp):
    m = lp.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(lp - m).sum(axis=1, keepdims=True)))[:, 0]


def ref64(w, mu, U, X, shift=None):
    X64 = np.asarray(np.asarray(X, dtype=np.float32), dtype=np.float64)
    n, D = X64.shape
    lp = ref64_lp(w, mu, U, X)
    lse = _lse64(lp)
    resp = np.exp(lp - lse[:, None])
    c = np.zeros(D) if shift is None else np.asarray(shift, dtype=np.float64)
    a1 = np.concatenate([np.ones((n, 1)), X64 - c[None]], axis=1)
    block = _block(resp, a1)
    return dict(block=block, ll=float(lse.sum()), lse=lse, resp=resp, s=_block(resp, np.abs(a1)),
                A=(np.abs(a1)[:, :, None] * np.abs(a1)[:, None, :]).reshape(n, -1).sum(axis=0), n=n, nk=resp.sum(axis=0), D=D)


def _a1_f32(X, shift):
    X = np.asarray(X, dtype=np.float32)
    c = np.zeros(X.shape[1], np.float32) if shift is None else np.asarray(shift, dtype=np.float64).astype(np.float32)
    a1 = np.concatenate([np.ones((X.shape[0], 1), np.float32), X - c[None]], axis=1)
    assert a1.dtype == np.float32
    return a1


def emu32_lp(w, mu, U, X, shift=None):
    """(n, K) float32: lp by the yardstick's arithmetic"""
    B, cst = image64(w, mu, U, shift)
    B32, c32 = B.astype(np.float32), cst.astype(np.float32)
    a1 = _a1_f32(X, shift)
    K, W, D = B32.shape
    lp = np.empty((a1.shape[0], K), dtype=np.float32)
    for k in range(K):
        y = np.zeros((a1.shape[0], D), dtype=np.float32)
        for i in range(W):
            y = y + a1[:, i:i + 1] * B32[k, i][None, :]     # float32 product, float32 sum, one term at a time
        ss = np.zeros(a1.shape[0], dtype=np.float32)
        for j in range(D):
            ss = ss + y[:, j] * y[:, j]
        lp[:, k] = c32[k] - np.float32(0.5) * ss
    assert lp.dtype == np.float32
    return lp


def _lse32(lp):
    mx = lp.max(axis=1, keepdims=True)
    return mx[:, 0] + np.log(np.exp(lp - mx).sum(axis=1, dtype=np.float32))


def emu32(w, mu, U, X, shift=None):
    lp = emu32_lp(w, mu, U, X, shift)
    lse = _lse32(lp)
    resp = np.exp(lp - lse[:, None])
    assert lse.dtype == np.float32 and resp.dtype == np.float32
    a1 = _a1_f32(X, shift).astype(np.float64)
    return dict(block=_block(resp, a1), ll=float(lse.astype(np.float64).sum()), lse=lse)


def emu32_alt(w, mu, U, X, shift=None):
    B, cst = image64(w, mu, U, shift)
    B32, c32 = B.astype(np.float32).astype(np.float64), cst.astype(np.float32)
    a1 = _a1_f32(X, shift)
    a64 = a1.astype(np.float64)
    K, W, D = B32.shape
    lp = np.empty((a1.shape[0], K), dtype=np.float32)
    for k in range(K):
        y = np.zeros((a1.shape[0], D), dtype=np.float32)
        idx = list(range(W - 1, -1, -1))
        for i in range(0, W, 2):
            pair = a64[:, idx[i]:idx[i] + 1] * B32[k, idx[i]][None, :]          # products of float32 values: exact in float64
            if i + 1 < W:
                pair = pair + a64[:, idx[i + 1]:idx[i + 1] + 1] * B32[k, idx[i + 1]][None, :]
            y = (y.astype(np.float64) + pair).astype(np.float32)               # one rounding per pair
        y64 = y.astype(np.float64)
        ss = np.zeros(a1.shape[0], dtype=np.float32)
        js = list(range(D - 1, -1, -1))
        for j in range(0, D, 2):
            pair = y64[:, js[j]] ** 2 + (y64[:, js[j + 1]] ** 2 if j + 1 < D else 0.0)
            ss = (ss.astype(np.float64) + pair).astype(np.float32)
        lp[:, k] = c32[k] - np.float32(0.5) * ss
    mx = lp.max(axis=1, keepdims=True)
    e = np.exp2((lp - mx) * LOG2E_F32)
    tot = e.sum(axis=1, dtype=np.float32)
    resp = e / tot[:, None]
    lse = mx[:, 0] + np.log2(tot) * LN2_F32
    assert lse.dtype == np.float32 and resp.dtype == np.float32
    return dict(block=_block(resp, a64), ll=float(lse.astype(np.float64).sum()), lse=lse)


def evaluate(w, mu, U, X, shift=None):
    return dict(ref=ref64(w, mu, U, X, shift), emu=emu32(w, mu, U, X, shift), K=np.shape(mu)[0], D=np.shape(mu)[1])


def block_of(st):
    """the (K, (D + 1)^2) block and loglik_sum of an api result or of an emulation's dict"""
    if "block" in st:
        return np.asarray(st["block"], dtype=np.float64), float(st["ll"])
    nk, sx, sxx = (np.asarray(st[k], dtype=np.float64) for k in ("nk", "sx", "sxx"))
    K, D = sx.shape
    M = np.empty((K, D + 1, D + 1))
    M[:, 0, 0] = nk
    M[:, 0, 1:] = sx
    M[:, 1:, 0] = sx
    M[:, 1:, 1:] = sxx
    return M.reshape(K, -1), float(st["loglik_sum"])


# ------------------------------------------------------------------------------------------------- the comparison
def _norm_err(v, ref):
    den = ref["s"] + 2.0 ** -100 * ref["A"][None, :]
    err = np.abs(np.asarray(v, dtype=np.float64) - ref["block"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v)))) if np.size(v) else 0.0


def limits(ev, L):
    ref, emu = ev["ref"], ev["emu"]
    ee = _norm_err(emu["block"], ref)
    rows = ref["nk"] >= RMS_MIN_NK
    d = np.asarray(emu["lse"], dtype=np.float64) - ref["lse"]
    n = ref["n"]
    mx = MAX_FACTOR * float(ee.max()) + 2.0 ** -20 + L * 2.0 ** -24
    return dict(max=mx, rms=RMS_FACTOR * _rms(ee[rows]) + 2.0 ** -22, rms_rows=rows, rms_applies=int(rows.sum()) >= RMS_MIN_MIX,
                ll=MAX_FACTOR * max(abs(float(d.sum())), np.sqrt(n) * _rms(d)) + 2.0 ** -22 * float((np.abs(ref["lse"]) + 1).sum()),
                mass=n * mx, emu_max=float(ee.max()), emu_rms=_rms(ee[rows]))


def measure(got, ev, L, what="", scale=1.0):
    """the measured ratios of one result under the rule, every limit multiplied by ``scale`` (the host file: 0.5)"""
    ref = ev["ref"]
    block, ll = block_of(got)
    assert block.shape == ref["block"].shape, (what, block.shape, ref["block"].shape)
    if not (np.isfinite(block).all() and np.isfinite(ll)):
        raise AssertionError("%s: %d entries are not finite" % (what, int((~np.isfinite(block)).sum()) + int(not np.isfinite(ll))))
    lim = limits(ev, L)
    e = _norm_err(block, ref)
    res = dict(max_ratio=float(e.max()) / (scale * lim["max"]), max_err=float(e.max()),
               rms_ratio=(_rms(e[lim["rms_rows"]]) / (scale * lim["rms"])) if lim["rms_applies"] else None,
               ll_ratio=abs(ll - ref["ll"]) / (scale * lim["ll"]), ll_err=abs(ll - ref["ll"]),
               mass_ratio=abs(float(block[:, 0].sum()) - ref["n"]) / (scale * lim["mass"]),
               emu_max=lim["emu_max"], emu_rms=lim["emu_rms"], max_vs_emu=float(e.max()) / max(lim["emu_max"], 1e-300))
    res["worst"] = max(res["max_ratio"], res["rms_ratio"] or 0.0, res["ll_ratio"], res["mass_ratio"])
    k, j = np.unravel_index(int(np.argmax(e)), e.shape)
    res["message"] = ("%s: ratios to the limits: max %.3g (entry [%d, %d], e = %.3g, emu32 %.3g), rms %s, loglik %.3g (error %.3g), mass %.3g"
                      % (what, res["max_ratio"], k, j, res["max_err"], res["emu_max"],
                         "skipped" if res["rms_ratio"] is None else "%.3g" % res["rms_ratio"], res["ll_ratio"], res["ll_err"],
                         res["mass_ratio"]))
    return res


def compare(got, ev, L, what="", scale=1.0):
    res = measure(got, ev, L, what, scale)
    if res["worst"] > 1.0:
        raise AssertionError(res["message"])
    return res


# ------------------------------------------------------------------------------------------------- the scorer
def ref64_loglik(w, mus, Us, X):
    """(M, F) float64 score_samples of every model"""
    return np.stack([_lse64(ref64_lp(w[m], mus[m], Us[m], X)) for m in range(len(mus))])


def emu32_loglik(w, mus, Us, X):
    return np.stack([_lse32(emu32_lp(w[m], mus[m], Us[m], X)) for m in range(len(mus))])


def compare_loglik(got, ref, emu, what=""):
    return GC.compare(got, ref, emu, what)


# ------------------------------------------------------------------------------------------------- case builders
def draw_model(rng, K, D, spread=1.0):
    """weights (K,), means (K, D), covariances (K, D, D) with condition numbers of a few tens, precisions_cholesky (K, D, D)"""
    w = rng.dirichlet(5 * np.ones(K))
    mu = spread * rng.standard_normal((K, D))
    cov = np.empty((K, D, D))
    for k in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        cov[k] = (Q * rng.uniform(0.3, 2.5, D)[None, :]) @ Q.T
        cov[k] = 0.5 * (cov[k] + cov[k].T)
    return w, mu, cov, prec_chol_of(cov)


def draw_frames(rng, w, mu, cov, n):
    comp = rng.choice(len(w), size=n, p=w / w.sum())
    L = np.linalg.cholesky(cov)
    z = rng.standard_normal((n, mu.shape[1]))
    return (mu[comp] + np.einsum("nij,nj->ni", L[comp], z)).astype(np.float32)


_CACHE = {}


def em_case(K, D, n, offset=0.0, seed=0):
    """one model and n frames drawn from it; offset: a common offset of that many sigma in every column (means and frames alike), the
    shift of the call is then the offset"""
    key = (K, D, n, offset, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(5000 + 97 * K + 13 * D + n + seed)
        w, mu, cov, U = draw_model(rng, K, D)
        X = draw_frames(rng, w, mu, cov, n)
        shift = None
        if offset:
            off = offset * np.sqrt(np.mean(np.diagonal(cov, axis1=1, axis2=2))) * np.ones(D)
            mu = mu + off[None]
            X = (X.astype(np.float64) + off[None]).astype(np.float32)
            shift = off
        c = dict(name="K%d_D%d_n%d_off%g" % (K, D, n, offset), w=w, mu=mu, cov=cov, U=U, X=X, shift=shift, K=K, D=D, n=n)
        c["ev"] = evaluate(w, mu, U, X, shift)
        _CACHE[key] = c
    return _CACHE[key]


# every D at two (K, n) pairs; every K and every n at D = 39
EM_D = (1, 4, 13, 16, 17, 39, 40, 64)
EM_K = (1, 3, 64, 65, 130)
EM_N = (1, 63, 64, 65, 257, 5000)
EM_SHAPES = tuple([(3, D, 257) for D in EM_D] + [(5, D, 65) for D in EM_D] + [(K, 39, 130) for K in EM_K if K != 3]
                  + [(3, 39, n) for n in EM_N if n != 257])
CAP_SHAPE = (3, 13, 20000)   # past the 8192-frame accumulator cap; with the budget lowered to 1 MB also past the slab


def scorer_case(M, ubm, K=5, D=13, lens=(0, 1, 70, 300), seed=0):
    key = ("score", M, ubm, K, D, tuple(lens), seed)
    if key not in _CACHE:
        rng = np.random.default_rng(8000 + 10 * M + int(ubm) + D + seed)
        models = [draw_model(rng, K, D) for _ in range(M)]
        w = np.stack([m[0] for m in models])
        mus = np.stack([m[1] for m in models])
        covs = np.stack([m[2] for m in models])
        Us = np.stack([m[3] for m in models])
        feats = [draw_frames(rng, w[u % M], mus[u % M], covs[u % M], n) for u, n in enumerate(lens)]
        X = np.vstack(feats).astype(np.float32)
        ref_ll, emu_ll = ref64_loglik(w, mus, Us, X), emu32_loglik(w, mus, Us, X)
        _CACHE[key] = dict(w=w, mus=mus, covs=covs, Us=Us, X=X, lens=list(lens), M=M, ubm=ubm, K=K, D=D, ref_ll=ref_ll, emu_ll=emu_ll,
                           ref_sc=GC.utt_means(ref_ll, lens), emu_sc=GC.utt_means(emu_ll, lens, np.float32))
    return _CACHE[key]


def orientation_set(seed=2024, D=16, n_train=1500, n_utt=60, utt_len=10, rho=0.9):
    """three speakers with the SAME mean (0) and the same per-axis variances (1 - rho / D) whose covariances differ in orientation only:
    Sigma_s = I - rho u_s u_s^T with u_s = row s + 1 of the D x D Hadamard matrix / sqrt(D) — every speaker is COMPRESSED along its own
    oblique direction and isotropic elsewhere.  No direction is elongated, so a mixture of a few axis-aligned Gaussians has nothing to
    spread its means along (an elongated direction it would trace: a 4-component 'diag' model separates correlated PAIRS of axes
    perfectly), and every marginal is the same.  -> (train {label: (n_train, D)}, x_test list of (utt_len, D), y_test)"""
    H = np.array([[1.0]])
    while H.shape[0] < D:
        H = np.block([[H, H], [H, -H]])
    rng = np.random.default_rng(seed)
    chol = []
    for s in range(3):
        u = H[s + 1] / np.sqrt(D)
        chol.append(np.linalg.cholesky(np.eye(D) - rho * np.outer(u, u)))
    train = {s: (rng.standard_normal((n_train, D)) @ chol[s].T).astype(np.float32) for s in range(3)}
    y_test = [u % 3 for u in range(n_utt)]
    x_test = [(rng.standard_normal((utt_len, D)) @ chol[s].T).astype(np.float32) for s in y_test]
    return train, x_test, y_test


# ------------------------------------------------------------------------------------------------- golden fits
GOLDEN = os.path.join(HERE, "golden", "gmm_full.npz")
FIT_CASES = {"K5_D13": (5, 13, 3000, 11), "K3_D39": (3, 39, 6000, 12)}   # K, D, n, seed


def fit_data(name):
    """the frames and the given initial parameters of a golden fit case, drawn from its seed (the golden holds a checksum of X)"""
    K, D, n, seed = FIT_CASES[name]
    rng = np.random.default_rng(seed)
    w, mu, cov, _ = draw_model(rng, K, D, spread=0.8)
    X = draw_frames(rng, w, mu, cov, n)
    w0 = rng.dirichlet(20 * np.ones(K))
    mu0 = mu + 0.3 * rng.standard_normal((K, D))
    P0 = np.stack([np.linalg.inv(c * rng.uniform(0.8, 1.3)) for c in cov])
    P0 = 0.5 * (P0 + np.transpose(P0, (0, 2, 1)))
    return X, w0, mu0, P0


def prec_chol_from_precisions(P):
    """sklearn's _compute_precision_cholesky_from_precisions ('full')"""
    return np.stack([np.linalg.cholesky(p[::-1, ::-1])[::-1, ::-1] for p in np.asarray(P, dtype=np.float64)])


def m_step64(st, n, reg_covar, shift=None):
    """the M step of include/ssp.h in float64 numpy -> weights, means, covariances, precisions_cholesky"""
    nk = st["nk"] + 10 * np.finfo(np.float64).eps
    m = st["sx"] / nk[:, None]
    cov = st["sxx"] / nk[:, None, None] - m[:, :, None] * m[:, None, :] + reg_covar * np.eye(m.shape[1])[None]
    w = nk / n
    return w / w.sum(), (m if shift is None else m + shift[None]), cov, prec_chol_of(cov)


def stats_of(ev_or_emu, K, D):
    """nk, sx, sxx, loglik_sum from an emulation's block"""
    M = np.asarray(ev_or_emu["block"]).reshape(K, D + 1, D + 1)
    return dict(nk=M[:, 0, 0].copy(), sx=M[:, 0, 1:].copy(), sxx=M[:, 1:, 1:].copy(), loglik_sum=ev_or_emu["ll"])


def emu_fit(X, w0, mu0, P0, max_iter, reg_covar=1e-6, stats=emu32):
    """max_iter EM iterations (tol = 0) with `stats` in place of the kernel, about the global mean as gmm_train does"""
    n, D = X.shape
    K = len(w0)
    shift = np.asarray(X, dtype=np.float64).mean(axis=0)
    w, mu, U = np.asarray(w0, dtype=np.float64), np.asarray(mu0, dtype=np.float64), prec_chol_from_precisions(P0)
    cov = lower = None
    for _ in range(max_iter):
        st = stats_of(stats(w, mu, U, X, shift), K, D)
        w, mu, cov, U = m_step64(st, n, reg_covar, shift)
        lower = st["loglik_sum"] / n
    return dict(weights=w, means=mu, covariances=cov, precisions_cholesky=U, lower_bound=lower)


FIT_BLOCKS = ("weights", "means", "covariances", "precisions_cholesky")


def golden_fit(gold, prefix):
    """sklearn's fitted parameters of one golden fit (the covariances and the factors are stored as upper triangles)"""
    w, mu = np.asarray(gold[prefix + "_weights"]), np.asarray(gold[prefix + "_means"])
    K, D = mu.shape
    iu = np.triu_indices(D)
    cov, U = np.zeros((K, D, D)), np.zeros((K, D, D))
    cov[:, iu[0], iu[1]] = gold[prefix + "_covariances_triu"]
    cov = cov + np.triu(cov, 1).transpose(0, 2, 1)
    U[:, iu[0], iu[1]] = gold[prefix + "_precisions_cholesky_triu"]
    return dict(weights=w, means=mu, covariances=cov, precisions_cholesky=U, lower_bound=float(gold[prefix + "_lower_bound"]),
                n_iter=int(gold[prefix + "_n_iter"]))


def fit_deviation(fit, gold_fit):
    """max |fit - sklearn| per parameter block"""
    return {b: float(np.abs(np.asarray(fit[b]) - gold_fit[b]).max()) for b in FIT_BLOCKS}
