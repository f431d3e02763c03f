"""Cases, references and the one comparison rule of tests/test_gmm_instances_host.py and tests/test_gmm_instances_gpu.py: every compiled
instance of the GMM scorer (csrc/gmm.hip, launch_kernel_any) against float64, on and off the well-conditioned case.

Three evaluations of one case:
  ref64   oracle.ref_cpu.gmm_score_samples / gmm_score: float64, the truth.
  emu32   a float32 numpy restatement of the fp32 kernel's own formula: the packed image W of ssp_gmm_pack (float64, log2 units, rounded
          to float32), aug = [x, x^2, 1] formed in float32, the 2 D + 1 products added one at a time in float32 in the kernel's k order
          (packed column j is MFMA step j / 2, half j & 1: plain increasing j, the constant last), a float32 exp2 / log2 log-sum-exp and
          one multiply by ln 2.  It is the YARDSTICK: what float32 evaluation of this formula costs by reference arithmetic alone.
  got     the library.

The comparison (compare): over the finite entries of a case
  max   |got - ref64| <= 8 max|emu32 - ref64| + 2^-20 (|ref64| + 1)          per entry
  rms   rms(got - ref64) <= 3 rms(emu32 - ref64) + 2^-22 (rms|ref64| + 1)
Why 8 and 3: two float32 evaluations of the same formula that differ only in summation order and in 1-ulp exp2 / log2 have RMS errors
within a small factor of each other, their maxima over 1e4 .. 1e5 entries spread wider; the MFMA's two-product step can only round less
often than emu32 does; 2^-20 (|ref| + 1) is the project's own log-sum-exp allowance (gmm.hip, gmm_band_kernel).  The margins come from
that reasoning, not from a run: a ratio above them is a finding.

Precision 2 (bf16x3 alone) is held per entry to the bound of include/ssp.h (bf16x3_bound).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_cpu as O  # noqa: E402

LOG2E = 1.4426950408889634
LN2_F32 = np.float32(0.6931471805599453)
PAD_CONST = -1.0e30  # the constant of a padded mixture and of a zero-weight mixture in both packed images

# ---- the instance tables of csrc/gmm.hip, restated
NQ_TABLE = (4, 7, 10, 16, 24, 32)   # fp32: k-depth / 8 >= (2 D + 1) / 8; NQ 24 and 32 run one column tile per wave (32-frame pieces)
NK_TABLE = (1, 2, 3, 4, 5, 6, 8)    # bf16x3: k-depth / 16 >= 2 D / 16


def pick_nq(D):
    need = (2 * D + 1 + 7) // 8
    return next((v for v in NQ_TABLE if v >= need), -1)


def pick_nk(D):
    need = (2 * D + 15) // 16
    return next((v for v in NK_TABLE if v >= need), 0)


def piece_granule(D, bf16):
    return 64 if (bf16 or pick_nq(D) <= 16) else 32


SWEEP_D = (1, 8, 9, 15, 16, 17, 24, 25, 27, 28, 32, 33, 39, 40, 41, 48, 49, 56, 57, 63, 64, 65, 95, 96, 127)
SWEEP_K = (1, 5, 31, 32, 33, 64, 70)
# empty utterances first, in the middle and last; 31 / 32 / 33 and 63 / 64 / 65 put both piece granules on their edges; 129 spans pieces
SWEEP_LENS = (0, 1, 31, 32, 33, 0, 63, 64, 65, 2, 129, 0)


def sweep_shape(D):
    """(K, M, has_ubm) of the sweep case at feature width D: K rotates, M = 3 with a UBM alternates with M = 2 without"""
    i = SWEEP_D.index(D)
    return SWEEP_K[i % len(SWEEP_K)], (3 if i % 2 == 0 else 2), i % 2 == 0


# ------------------------------------------------------------------------------------------------- references
def pack_w(w, mu, cov):
    """ssp_gmm_pack's image of ONE model in float64: (K, 2 D + 1), log2 units, the constant in the last column accumulated over d in
    the library's order; a zero weight's constant is PAD_CONST"""
    w, mu, cov = (np.asarray(a, dtype=np.float64) for a in (w, mu, cov))
    K, D = mu.shape
    P = 1.0 / cov
    W = np.empty((K, 2 * D + 1))
    W[:, :D] = mu * P * LOG2E
    W[:, D:2 * D] = -0.5 * P * LOG2E
    with np.errstate(divide="ignore"):
        c = np.log(w) - 0.5 * D * np.log(2.0 * np.pi)
    for d in range(D):
        c = c + (0.5 * np.log(P[:, d]) - 0.5 * mu[:, d] * mu[:, d] * P[:, d])
    W[:, 2 * D] = np.where(w > 0, c * LOG2E, PAD_CONST)
    return W


def emu32_loglik(w, mus, cov, X):
    """(M, F) float32: the fp32 kernel's formula in float32 numpy, see the module docstring"""
    X = np.asarray(X, dtype=np.float32)
    M, K, D = np.shape(mus)
    out = np.empty((M, X.shape[0]), dtype=np.float32)
    aug = np.concatenate([X, X * X, np.ones((X.shape[0], 1), np.float32)], axis=1)
    assert aug.dtype == np.float32
    for m in range(M):
        W = pack_w(w[m], mus[m], cov[m]).astype(np.float32)
        acc = np.zeros((X.shape[0], K), dtype=np.float32)
        for j in range(2 * D + 1):
            acc = acc + aug[:, j:j + 1] * W[None, :, j]   # float32 product, float32 sum, one term at a time
        assert acc.dtype == np.float32
        mx = acc.max(axis=1, keepdims=True)
        s = np.exp2(acc - mx).sum(axis=1, dtype=np.float32)
        out[m] = (mx[:, 0] + np.log2(s)) * LN2_F32
    assert out.dtype == np.float32
    return out


def ref64_loglik(w, mus, cov, X):
    """(M, F) float64: the oracle's score_samples under every model (a zero weight is log 0 = -inf there: no contribution)"""
    X = np.asarray(X, dtype=np.float32)
    with np.errstate(divide="ignore"):
        return np.stack([O.gmm_score_samples(w[m], mus[m], cov[m], X) for m in range(len(mus))])


def utt_means(ll, lens, dtype=np.float64):
    """(U, M): per-utterance mean of (M, F) per-frame values in float64, rounded to `dtype`; an empty utterance is a NaN row"""
    off = np.concatenate([[0], np.cumsum(lens)])
    out = np.full((len(lens), ll.shape[0]), np.nan)
    for u, n in enumerate(lens):
        if n:
            out[u] = np.asarray(ll[:, off[u]:off[u + 1]], dtype=np.float64).mean(axis=1)
    return out.astype(dtype)


def ref64_scores(w, mus, cov, X, lens):
    """(U, M) float64 by the oracle's gmm_score (= the mean of its score_samples)"""
    X = np.asarray(X, dtype=np.float32)
    off = np.concatenate([[0], np.cumsum(lens)])
    out = np.full((len(lens), len(mus)), np.nan)
    with np.errstate(divide="ignore"):
        for u, n in enumerate(lens):
            if n:
                out[u] = [O.gmm_score(w[m], mus[m], cov[m], X[off[u]:off[u + 1]]) for m in range(len(mus))]
    return out


def exponent_magnitude(w, mus, cov, X):
    """(M, F) float64: max_k (sum_d |x mu P| + x^2 P / 2 + |c_k|) in nats over the mixtures with a weight — the sum of the magnitudes of
    the terms a mixture's exponent is made of"""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((len(mus), X.shape[0]))
    for m in range(len(mus)):
        W = pack_w(w[m], mus[m], cov[m]) / LOG2E
        D = X.shape[1]
        mag = np.abs(X) @ np.abs(W[:, :D]).T + (X * X) @ np.abs(W[:, D:2 * D]).T + np.abs(W[None, :, 2 * D])
        out[m] = mag[:, np.asarray(w[m]) > 0].max(axis=1)
    return out


def emu32_forward_bound(w, mus, cov, X, ref):
    """(M, F): rigorous forward bound on |emu32 - ref64|.  Each of the 2 D + 1 terms carries the rounding of W, of the product (x^2: two)
    and of at most 2 D + 1 partial sums: (2 D + 4) 2^-24 <= 4 D 2^-23 of the sum of the terms' magnitudes (D = 1: 6 <= 8); the
    log-sum-exp is 1-Lipschitz in the max norm over the mixtures and costs a few ulp of its own (2^-20 (|ref| + 1))."""
    D = np.shape(mus)[2]
    return 4 * D * 2.0 ** -23 * 1.01 * exponent_magnitude(w, mus, cov, X) + 2.0 ** -20 * (np.abs(ref) + 1)


def bf16x3_bound(w, mus, cov, X, ref):
    """(M, F): the per-frame bound of include/ssp.h on the bf16x3 path's log-likelihood,
       eps S(x_t) + 2^-20 (|ref| + 1) + 2^-24 max_k |c_k|,  eps = 3.01 2^-18 + 8 D 2^-23 1.01,
    S(x) = sum_d |x_d| max|mu P|_d + x_d^2 max(P / 2)_d with the maxima over every mixture of every model, as gmm_band_kernel takes them
    (ssp_gmm_pack's table); the last term is the float32 rounding of the mixture constant (the accumulator's initial value)."""
    mus, cov = np.asarray(mus, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    D = mus.shape[2]
    P = 1.0 / cov
    A = (np.abs(mus) * P).reshape(-1, D).max(axis=0)
    B = (0.5 * P).reshape(-1, D).max(axis=0)
    S = np.abs(X) @ A + (X * X) @ B
    eps = 3.01 * 2.0 ** -18 + 8 * D * 2.0 ** -23 * 1.01
    cmax = np.empty(len(mus))
    for m in range(len(mus)):
        c = pack_w(w[m], mus[m], cov[m])[:, 2 * D] / LOG2E
        cmax[m] = np.abs(c[np.asarray(w[m]) > 0]).max()
    return eps * S[None, :] + 2.0 ** -20 * (np.abs(ref) + 1) + 2.0 ** -24 * cmax[:, None]


# ------------------------------------------------------------------------------------------------- the comparison
MAX_FACTOR, RMS_FACTOR = 8.0, 3.0


def entry_tolerance(ref, emu):
    """per-entry limit of the max rule over the finite entries of `ref` (same shape as ref; NaN where ref is NaN)"""
    ref = np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    e = np.abs(np.asarray(emu, dtype=np.float64) - ref)[fin]
    return MAX_FACTOR * (e.max() if e.size else 0.0) + 2.0 ** -20 * (np.abs(ref) + 1)


def compare(got, ref, emu, what=""):
    """The one rule of both test files.  Entries where ref is NaN (empty utterances) are left out: the caller checks them.  Returns the
    measured ratios {max_ratio, rms_ratio: error over its limit; max_vs_emu, rms_vs_emu: error over emu32's own} and raises
    AssertionError when a ratio exceeds 1."""
    got, ref, emu = (np.asarray(a, dtype=np.float64) for a in (got, ref, emu))
    assert got.shape == ref.shape == emu.shape, (what, got.shape, ref.shape, emu.shape)
    fin = np.isfinite(ref)
    assert fin.any(), (what, "no finite reference entry")
    assert np.isfinite(emu[fin]).all(), (what, "emu32 is not finite where ref64 is")
    g, r, e = got[fin], ref[fin], emu[fin]
    if not np.isfinite(g).all():
        raise AssertionError("%s: %d of %d entries are not finite where the reference is" % (what, int((~np.isfinite(g)).sum()), g.size))
    err, eerr = np.abs(g - r), np.abs(e - r)
    tol = MAX_FACTOR * eerr.max() + 2.0 ** -20 * (np.abs(r) + 1)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))  # noqa: E731
    rms_tol = RMS_FACTOR * rms(eerr) + 2.0 ** -22 * (rms(r) + 1)
    res = dict(max_ratio=float((err / tol).max()), rms_ratio=rms(err) / rms_tol, max_err=float(err.max()), rms_err=rms(err),
               emu_max_err=float(eerr.max()), emu_rms_err=rms(eerr),
               max_vs_emu=float(err.max() / max(eerr.max(), 1e-300)), rms_vs_emu=rms(err) / max(rms(eerr), 1e-300))
    if res["max_ratio"] > 1.0 or res["rms_ratio"] > 1.0:
        raise AssertionError("%s: max error %.3e is %.2f x its limit, rms error %.3e is %.2f x its limit (emu32: max %.3e rms %.3e)"
                             % (what, res["max_err"], res["max_ratio"], res["rms_err"], res["rms_ratio"], res["emu_max_err"],
                                res["emu_rms_err"]))
    return res


def compare_bound(got, ref, bound, what=""):
    """precision 2: every finite-reference entry within `bound`; returns the largest error / bound"""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    fin = np.isfinite(ref)
    if not np.isfinite(got[fin]).all():
        raise AssertionError("%s: entries are not finite where the reference is" % (what,))
    ratio = float((np.abs(got[fin] - ref[fin]) / bound[fin]).max())
    if ratio > 1.0:
        raise AssertionError("%s: bf16x3 error is %.2f x the bound of include/ssp.h" % (what, ratio))
    return ratio


# ------------------------------------------------------------------------------------------------- case builders
def _finish(name, w, mus, cov, ubm, feats, lens, **extra):
    """the three evaluations of a case, computed once"""
    X = np.vstack(feats).astype(np.float32) if len(feats) else np.zeros((0, mus.shape[2]), np.float32)
    ref_ll = ref64_loglik(w, mus, cov, X)
    emu_ll = emu32_loglik(w, mus, cov, X)
    c = dict(name=name, w=w, mus=mus, cov=cov, ubm=ubm, X=X, lens=list(lens), M=mus.shape[0], K=mus.shape[1], D=mus.shape[2],
             ref_ll=ref_ll, emu_ll=emu_ll, ref_sc=utt_means(ref_ll, lens), emu_sc=utt_means(emu_ll, lens, np.float32))
    c.update(extra)
    return c


def _draw_models(rng, K, D, M, spread):
    """every model its own weights, means and covariances: speaker means `spread` sigma from a common base"""
    base = rng.standard_normal((K, D))
    w = rng.dirichlet(5 * np.ones(K), M)
    cov = rng.uniform(0.5, 2.0, (M, K, D))
    mus = base[None] + spread * np.sqrt(cov) * rng.standard_normal((M, K, D))
    return w, mus, cov


def _draw_frames(rng, w, mu, cov, n, noise=1.0):
    comp = rng.choice(len(w), size=n, p=w / w.sum())
    return (mu[comp] + noise * np.sqrt(cov[comp]) * rng.standard_normal((n, mu.shape[1]))).astype(np.float32)


def margins(sc, ubm):
    """float64 top-2 margin, arg-max and the indices (into the model axis) of the two best, per utterance of a finite (U, M) matrix"""
    first = 1 if ubm else 0
    d = sc[:, first:] - sc[:, :1] if ubm else sc
    order = np.argsort(-d, axis=1, kind="stable")
    best, second = order[:, 0], order[:, 1]
    rows = np.arange(len(d))
    return d[rows, best] - d[rows, second], best, first + best, first + second


def argmax_tolerance(c):
    """(U, M): what a score may be off by at ANY precision under test — the comparison's per-entry limit (precision 0 / 1) or the mean
    over the utterance's frames of the bf16x3 bound (precision 2), whichever is larger"""
    tol = entry_tolerance(c["ref_sc"], c["emu_sc"])
    if pick_nk(c["D"]):
        tol = np.maximum(tol, utt_means(bf16x3_bound(c["w"], c["mus"], c["cov"], c["X"], c["ref_ll"]), c["lens"]))
    return tol


def construction_ok(c):
    """the sweep's construction conditions: every non-empty utterance's float64 top-2 margin exceeds twice the tolerance of its two
    scores, and the true speaker wins.  Returns (ok, share of non-empty utterances left out of the arg-max check)"""
    nz = np.asarray(c["lens"]) > 0
    sc, tol = c["ref_sc"][nz], argmax_tolerance(c)[nz]
    margin, best, i1, i2 = margins(sc, c["ubm"])
    rows = np.arange(len(sc))
    clear = margin > 2 * (tol[rows, i1] + tol[rows, i2])
    wins = best == c["speaker"][nz]
    return bool(clear.all() and wins.all()), float(1.0 - clear.mean())


_CACHE = {}


def sweep_case(D):
    """The instance sweep's case at feature width D.  Utterance u is spoken by speaker u mod S, its frames drawn from that speaker's own
    model at half its spread; the speakers sit 3 / sqrt(D) + 0.5 sigma apart per entry so that even the 1-frame utterance is decided.
    The seed is the first of 1000 D, 1000 D + 1, ... at which the construction conditions hold (construction_ok: the host file asserts
    them) — the seed moves, never a limit."""
    key = ("sweep", D)
    if key in _CACHE:
        return _CACHE[key]
    K, M, ubm = sweep_shape(D)
    first = 1 if ubm else 0
    S = M - first
    spread = 3.0 / np.sqrt(D) + 0.5
    for seed in range(1000 * D, 1000 * D + 200):
        rng = np.random.default_rng(seed)
        w, mus, cov = _draw_models(rng, K, D, M, spread)
        speaker = np.array([u % S for u in range(len(SWEEP_LENS))])
        feats = [_draw_frames(rng, w[first + speaker[u]], mus[first + speaker[u]], cov[first + speaker[u]], n, noise=0.5)
                 for u, n in enumerate(SWEEP_LENS)]
        c = _finish("sweep_D%d" % D, w, mus, cov, ubm, feats, SWEEP_LENS, seed=seed, speaker=speaker)
        if construction_ok(c)[0]:
            nz = np.asarray(SWEEP_LENS) > 0
            am = np.zeros(len(SWEEP_LENS), dtype=np.int64)
            am[nz] = margins(c["ref_sc"][nz], ubm)[1]
            c["ref_am"] = am
            _CACHE[key] = c
            return c
    raise AssertionError("no seed in 200 gives sweep case D = %d its margins" % D)


def shifted_models(c, sigmas):
    """The teeth mutation: one mean entry (dimension 0) of one mixture of the first speaker model moved by `sigmas` standard deviations.
    The mixture is the one that explains most frames of that speaker's utterances.  Returns the means array (the rest of c stays)."""
    m = 1 if c["ubm"] else 0
    lp = O.gmm_log_prob(c["w"][m], c["mus"][m], c["cov"][m], c["X"])
    off = np.concatenate([[0], np.cumsum(c["lens"])])
    own = np.concatenate([np.arange(off[u], off[u + 1]) for u in range(len(c["lens"])) if c["speaker"][u] == 0]).astype(np.int64)
    k = int(np.bincount(lp[own].argmax(axis=1), minlength=c["K"]).argmax())
    mus = c["mus"].copy()
    mus[m, k, 0] += sigmas * np.sqrt(c["cov"][m, k, 0])
    return mus


# ---- off the easy case: D in (39, 13), K in (16, 64, 257), M = 2 without a UBM, the sweep's lengths
HARD_LENS = (0, 1, 33, 64, 65, 0, 129, 2)
HARD_KINDS = ("uncentred10", "uncentred30", "uncentred100", "wide_cov", "skewed_w", "outliers", "identical")
HARD_SHAPES = tuple((K, D) for D in (39, 13) for K in (16, 64, 257))


def hard_case(kind, K, D):
    key = (kind, K, D)
    if key in _CACHE:
        return _CACHE[key]
    M = 2
    rng = np.random.default_rng(70000 + 1000 * HARD_KINDS.index(kind) + 2 * K + D)
    w, mus, cov = _draw_models(rng, K, D, M, 0.3)
    extra = {}
    noise = 1.0
    if kind.startswith("uncentred"):
        # every feature column has a large common offset, |mu| / sigma = ratio: the expansion's terms are ratio^2 larger than their sum
        ratio = float(kind[len("uncentred"):])
        sign = rng.choice([-1.0, 1.0], D)
        mus = ratio * sign * np.sqrt(cov) + np.sqrt(cov) * rng.standard_normal((M, K, D))
        extra["ratio"] = ratio
    elif kind == "wide_cov":
        cov = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), (M, K, D)))
    elif kind == "skewed_w":
        w = np.maximum(rng.dirichlet(0.02 * np.ones(K), M), 1e-300)
        w = w / w.sum(axis=1, keepdims=True)
    elif kind == "identical":
        # K identical mixtures with equal weights: log-sum-exp of K equal exponents, the answer is the single Gaussian's log density
        w = np.full((M, K), 1.0 / K)
        mus = np.repeat(mus[:, :1], K, axis=1)
        cov = np.repeat(cov[:, :1], K, axis=1)
    if kind == "outliers":
        # 50 sigma of the widest mixture (cov <= 2) from the farthest mean, in every dimension: |ll| is 0.5 D 50^2 2 / cov, about 8e4 at D = 39
        reach = np.abs(mus).max() + 50.0 * np.sqrt(2.0)
        feats = [(reach * rng.choice([-1.0, 1.0], (n, D)) * rng.uniform(1.0, 1.05, (n, D))).astype(np.float32) for n in HARD_LENS]
    else:
        feats = [_draw_frames(rng, w[u % M], mus[u % M], cov[u % M], n, noise) for u, n in enumerate(HARD_LENS)]
    c = _finish("%s_K%d_D%d" % (kind, K, D), w, mus, cov, False, feats, HARD_LENS, **extra)
    if kind == "identical":
        single = np.stack([O.gmm_log_prob(np.ones(1), mus[m, :1], cov[m, :1], c["X"])[:, 0] for m in range(M)])
        assert np.abs(c["ref_ll"] - single).max() <= 1e-9 * (np.abs(single).max() + 1)   # lp + log K with lp carrying log (1 / K)
    if kind == "outliers":
        z = np.abs(c["X"][:, None, None, :].astype(np.float64) - mus[None]) / np.sqrt(cov[None])
        assert z.min() >= 50.0
        assert np.isfinite(c["ref_ll"]).all()
    _CACHE[key] = c
    return c


def late_dominant_case(D):
    """K = 70: the frames belong to mixture 69, which sits in the padded last row tile (mixtures 64 .. 69 + 26 pads), and every other
    mixture is more than 300 nats below it: the running sum of two tiles is rescaled to nothing when the third arrives"""
    key = ("late", D)
    if key in _CACHE:
        return _CACHE[key]
    K, M = 70, 2
    rng = np.random.default_rng(6900 + D)
    w, mus, cov = _draw_models(rng, K, D, M, 0.3)
    mus[:, 69] += 15.0 * np.sqrt(cov[:, 69]) * rng.choice([-1.0, 1.0], D)   # (the same way in both models)
    feats = [(mus[u % M, 69] + 0.5 * np.sqrt(cov[u % M, 69]) * rng.standard_normal((n, D))).astype(np.float32) for u, n in enumerate(HARD_LENS)]
    c = _finish("late_dominant_K70_D%d" % D, w, mus, cov, False, feats, HARD_LENS)
    for m in range(M):
        lp = O.gmm_log_prob(w[m], mus[m], cov[m], c["X"])
        assert (lp[:, 69] - np.delete(lp, 69, axis=1).max(axis=1) > 300.0).all()
    _CACHE[key] = c
    return c


# ---- zero weights: M = 3 with a UBM at D = 13, model 1 carries the zeros (renormalised), models 0 and 2 are untouched
ZERO_PATTERNS = {
    "one_in_the_middle_K64": (64, (37,)),
    "one_lane_half_of_the_first_tile_K64": (64, tuple(k for k in range(32) if (k >> 2) % 2 == 0)),   # 0-3, 8-11, 16-19, 24-27
    "first_tile_K64": (64, tuple(range(32))),
    "a_later_tile_K96": (96, tuple(range(32, 64))),
    "last_tile_K70": (70, tuple(range(64, 70))),
}


def zero_weight_case(name):
    """(case with the zeros, weights before the zeros)"""
    key = ("zero", name)
    if key in _CACHE:
        return _CACHE[key]
    K, zeros = ZERO_PATTERNS[name]
    D, M = 13, 3
    rng = np.random.default_rng(1300 + sorted(ZERO_PATTERNS).index(name))
    w0, mus, cov = _draw_models(rng, K, D, M, 0.5)
    w = w0.copy()
    w[1, list(zeros)] = 0.0
    w[1] /= w[1].sum()
    # frames of every model, the zeroed mixtures' own neighbourhoods among them (drawn with the weights before the zeros)
    feats = [_draw_frames(rng, w0[u % M], mus[u % M], cov[u % M], n) for u, n in enumerate(SWEEP_LENS)]
    c = _finish("zero_" + name, w, mus, cov, True, feats, SWEEP_LENS, zeros=zeros)
    assert np.isfinite(c["ref_ll"]).all() and np.isfinite(c["emu_ll"]).all()
    _CACHE[key] = (c, w0)
    return _CACHE[key]
