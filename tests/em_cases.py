"""Cases, references and the one comparison rule of tests/test_em_instances_host.py, tests/test_em_instances_isa.py and
tests/test_em_instances_gpu.py: every compiled kernel of the EM statistics (csrc/gmm_em.hip: ssp_gmm_em_stats, ssp_gmm_em_stats_batch,
ssp_gmm_em_stats_shared) against float64, on every route, on and off the well-conditioned case.

Three evaluations of one model over frames X (float32):
  ref64      oracle.ref_cpu.gmm_em_stats (float64, the truth) with the per-frame lse and resp it is made of, and two sums of magnitudes:
             s[k,j] = sum_t resp[t,k] |aug[t,j]| with aug = [x, x^2, 1] — what each entry of the K x (2 D + 1) block [sx, sxx, nk] is made
             of, so that cancellation inside sx does not hide an error — and A[j] = sum_t |aug[t,j]|.
  emu32      the YARDSTICK: em_pack's image restated (A = mu P, B = -P / 2, c accumulated over d in the library's order, nats; float64
             rounded to float32; a padded mixture's c is -1e30), aug formed in float32, the 2 D + 1 products added one at a time in float32
             in increasing column order with the constant last, a float32 log-sum-exp and resp = exp(lp - lse) in float32, the sums over
             the frames in float64.  It is what float32 evaluation of this formula costs by reference arithmetic alone.
  emu32_alt  the same formula in another order: columns reversed, the products added in exactly formed pairs rounded once per pair (the
             shape of the two-product MFMA step), exp2 / log2, resp = e / sum.  "A different legitimate float32 kernel": the host file
             holds it to half of every limit, so the rule has room for a kernel and none for a fault.

The rule (compare).  den = s + 2^-100 A[j]; e(v) = |v - ref64| / den per entry of the block.  The second term of den is there because a
float32 exp flushes a responsibility below 2^-126 to zero: without it a mixture that owns nothing has normalised error 1 and the rule is
vacuous (seen with weights drawn from dirichlet(0.02)).
  max     max e(got) <= 8 max e(emu32) + 2^-20 + L 2^-24          over every entry
          L = 64 ceil(n_tiles / G), G = min(n_tiles, cap): the largest number of frames one accumulator adds in float32 (walk_cap
          restates how gmm_em.hip takes cap from the number of compute units)
  rms     rms e(got) <= 3 rms e(emu32) + 2^-22                     over the entries of the mixtures with nk_ref >= 8; skipped (and said
          so in the result) when fewer than 4 mixtures qualify: mixtures with less than a frame's worth of mass do not average, two correct
          float32 evaluations differ there by more than this limit
  loglik  |got - ref| <= 8 max(|sum_t d_t|, sqrt(n) rms_t d_t) + 2^-22 sum_t (|lse_ref[t]| + 1),  d = lse_emu32 - lse_ref
  mass    |sum_k nk - n| <= n (8 max e(emu32) + 2^-20 + L 2^-24)
Why 8 and 3 and 2^-20: they are tests/gmm_cases.py's.  Two float32 evaluations of one formula that differ in summation order and in the
last bit of exp / log have RMS errors within a small factor of each other, their maxima over 1e3 .. 1e5 entries spread wider; the MFMA's
two-product step can only round less often than emu32 does; 2^-20 is the project's log-sum-exp allowance (gmm.hip, gmm_band_kernel) and
also covers __expf and __logf, whose relative error grows with the size of the argument.  None of these numbers is measured on the code
under test: a ratio above 1 is a finding.  compare returns the measured ratios so that they can be written down.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_cpu as O  # noqa: E402

PAD_CONST = -1.0e30          # the constant of a padded mixture in em_pack's image
LOG2E_F32 = np.float32(1.4426950408889634)
LN2_F32 = np.float32(0.6931471805599453)
EM_TF, EM_KC = 64, 64        # frames per tile, mixtures per chunk (gmm_em.hip)
NUM_CU_DEFAULT = 256         # MI355X; the GPU file passes the device's own count
MAX_D, MAX_D_MFMA = 64, 47   # ssp_gmm_em_stats; the MFMA kernels and with them the batched entry points

# ---- the 18 kernels gmm_em.hip compiles (3 VALU / helper + 6 + 6 MFMA accumulation + 3; tests/test_em_instances_isa.py reads the names)
INSTANCES = tuple(
    [("gmm_em_lse_kernel",), ("gmm_em_acc_kernel",), ("gmm_em_lse_mfma_kernel",)]
    + [("gmm_em_acc_mfma_kernel", nct, fuse) for nct in (1, 2, 3) for fuse in (True, False)]
    + [("gmm_em_acc_mfma_seg_kernel", nct, fuse) for nct in (1, 2, 3) for fuse in (True, False)]
    + [("gmm_em_lse_mfma_seg_kernel",), ("gmm_em_reduce_kernel",), ("gmm_em_reduce_seg_kernel",)])

ENTRIES = ("single", "batch", "shared")


def nct_of(D):
    return (2 * D + 1 + 31) // 32


def route_of(entry, K, D, env=()):
    """the kernels of gmm_em.hip that one call runs (the dispatch of ssp_gmm_em_stats / em_stats_batch_impl restated); env: the names of
    the set switches among SSP_EM_NO_MFMA, SSP_EM_NO_FUSE (read by the single call alone).  None: the call raises NotImplementedError."""
    assert entry in ENTRIES
    nct = nct_of(D)
    if entry == "single":
        if D > MAX_D:
            return None
        mfma = nct <= 3 and "SSP_EM_NO_MFMA" not in env
        fuse = mfma and K <= EM_KC and "SSP_EM_NO_FUSE" not in env
        if fuse:
            return (("gmm_em_acc_mfma_kernel", nct, True), ("gmm_em_reduce_kernel",))
        if mfma:
            return (("gmm_em_lse_mfma_kernel",), ("gmm_em_acc_mfma_kernel", nct, False), ("gmm_em_reduce_kernel",))
        return (("gmm_em_lse_kernel",), ("gmm_em_acc_kernel",), ("gmm_em_reduce_kernel",))
    if nct > 3:
        return None
    if K <= EM_KC:
        return (("gmm_em_acc_mfma_seg_kernel", nct, True), ("gmm_em_reduce_seg_kernel",))
    return (("gmm_em_lse_mfma_seg_kernel",), ("gmm_em_acc_mfma_seg_kernel", nct, False), ("gmm_em_reduce_seg_kernel",))


def single_routes(K, D):
    """(label, env names) of every route the single call has at this shape"""
    r = [("default", ())]
    if D <= MAX_D_MFMA:
        if K <= EM_KC:
            r.append(("no_fuse", ("SSP_EM_NO_FUSE",)))
        r.append(("no_mfma", ("SSP_EM_NO_MFMA",)))
    return r


def walk_cap(entry, K, num_cu=NUM_CU_DEFAULT):
    """the largest number of persistent walkers per mixture chunk, as gmm_em.hip takes it from the number of compute units"""
    chunks = (K + EM_KC - 1) // EM_KC
    if entry == "single" or chunks == 1:
        return 2 * num_cu
    return max(1, 2 * num_cu // chunks)


def acc_frames(n, cap):
    """L of the rule: 64 ceil(n_tiles / G), G = min(n_tiles, cap)"""
    n_tiles = (n + EM_TF - 1) // EM_TF
    G = min(n_tiles, cap)
    return EM_TF * ((n_tiles + G - 1) // G)


# ------------------------------------------------------------------------------------------------- references
def em_image(w, mu, cov, pad_const=PAD_CONST):
    """em_pack's image of one model in float64: (Kp, 2 D + 1) = (A, B, c), Kp = K rounded up to 64"""
    w, mu, cov = (np.asarray(a, dtype=np.float64) for a in (w, mu, cov))
    K, D = mu.shape
    Kp = (K + EM_KC - 1) // EM_KC * EM_KC
    P = 1.0 / cov
    W = np.zeros((Kp, 2 * D + 1))
    W[:K, :D] = mu * P
    W[:K, D:2 * D] = -0.5 * P
    c = np.log(w) - 0.5 * D * np.log(2.0 * np.pi)
    for d in range(D):
        c = c + (0.5 * np.log(P[:, d]) - 0.5 * mu[:, d] * mu[:, d] * P[:, d])
    W[:K, 2 * D] = c
    W[K:, 2 * D] = pad_const
    return W


def _aug32(X, x2_shift=False):
    X = np.asarray(X, dtype=np.float32)
    sq = X * X
    if x2_shift:   # (a mutation of the host file: x^2 taken from the neighbouring column)
        sq = np.roll(sq, -1, axis=1)
    aug = np.concatenate([X, sq, np.ones((X.shape[0], 1), np.float32)], axis=1)
    assert aug.dtype == np.float32
    return aug


def _sums(resp, aug, lse, K, keep=None):
    """block [sx, sxx, nk] (K, 2 D + 1) and loglik_sum: the sums over the frames in float64"""
    r = np.asarray(resp, dtype=np.float64)[:, :K]
    a = np.asarray(aug, dtype=np.float64)
    l = np.asarray(lse, dtype=np.float64)
    if keep is not None:
        r, a, l = r[keep], a[keep], l[keep]
    return r.T @ a, float(l.sum())


def ref64(w, mu, cov, X):
    X64 = np.asarray(np.asarray(X, dtype=np.float32), dtype=np.float64)
    n, D = X64.shape
    nk, sx, sxx, ll = O.gmm_em_stats(w, mu, cov, X64)
    lp = O.gmm_log_prob(w, mu, cov, X64)
    m = lp.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(lp - m).sum(axis=1, keepdims=True)))[:, 0]
    resp = np.exp(lp - lse[:, None])
    aug = np.abs(np.concatenate([X64, X64 * X64, np.ones((n, 1))], axis=1))
    return dict(block=np.concatenate([sx, sxx, nk[:, None]], axis=1), ll=ll, lse=lse, resp=resp, s=resp.T @ aug, A=aug.sum(axis=0), n=n,
                nk=nk)


def emu32(w, mu, cov, X, pad_const=PAD_CONST, sep_halves=False, x2_shift=False, keep=None):
    """the yardstick (module docstring).  The keyword arguments are the host file's mutations: a padded mixture's constant, the two
    32-mixture halves of a chunk normalised separately, x^2 from the neighbouring column, `keep`: the frames that reach the sums."""
    K, D = np.shape(mu)
    W = em_image(w, mu, cov, pad_const).astype(np.float32)
    aug = _aug32(X, x2_shift)
    acc = np.zeros((aug.shape[0], W.shape[0]), dtype=np.float32)
    for j in range(2 * D + 1):
        acc = acc + aug[:, j:j + 1] * W[None, :, j]   # float32 product, float32 sum, one term at a time
    assert acc.dtype == np.float32

    def lse_of(a):
        mx = a.max(axis=1, keepdims=True)
        return mx[:, 0] + np.log(np.exp(a - mx).sum(axis=1, dtype=np.float32))

    lse = lse_of(acc)
    if sep_halves:
        resp = np.concatenate([np.exp(acc[:, h:h + 32] - lse_of(acc[:, h:h + 32])[:, None]) for h in range(0, W.shape[0], 32)], axis=1)
    else:
        resp = np.exp(acc - lse[:, None])
    assert lse.dtype == np.float32 and resp.dtype == np.float32
    block, ll = _sums(resp, _aug32(X), lse, K, keep)
    return dict(block=block, ll=ll, lse=lse)


def emu32_alt(w, mu, cov, X):
    """another legitimate float32 evaluation (module docstring)"""
    K, D = np.shape(mu)
    W = em_image(w, mu, cov).astype(np.float32).astype(np.float64)
    aug = _aug32(X)
    a64 = aug.astype(np.float64)
    acc = np.zeros((aug.shape[0], W.shape[0]), dtype=np.float32)
    js = list(range(2 * D, -1, -1))
    for i in range(0, len(js), 2):
        pair = a64[:, js[i]:js[i] + 1] * W[None, :, js[i]]           # products of float32 values: exact in float64
        if i + 1 < len(js):
            pair = pair + a64[:, js[i + 1]:js[i + 1] + 1] * W[None, :, js[i + 1]]
        acc = (acc.astype(np.float64) + pair).astype(np.float32)      # one rounding per pair
    mx = acc.max(axis=1, keepdims=True)
    e = np.exp2((acc - mx) * LOG2E_F32)
    tot = e.sum(axis=1, dtype=np.float32)
    resp = e / tot[:, None]
    lse = mx[:, 0] + np.log2(tot) * LN2_F32
    assert lse.dtype == np.float32 and resp.dtype == np.float32
    block, ll = _sums(resp, aug, lse, K)
    return dict(block=block, ll=ll, lse=lse)


def evaluate(w, mu, cov, X):
    """ref64 and emu32 of one model over X"""
    return dict(ref=ref64(w, mu, cov, X), emu=emu32(w, mu, cov, X), K=np.shape(mu)[0], D=np.shape(mu)[1])


def block_of(st, m=None):
    """[sx, sxx, nk] (K, 2 D + 1) and loglik_sum of an api result (model m of a batched one)"""
    if "block" in st:
        return np.asarray(st["block"], dtype=np.float64), float(st["ll"])
    nk, sx, sxx, ll = st["nk"], st["sx"], st["sxx"], st["loglik_sum"]
    if m is not None:
        nk, sx, sxx, ll = nk[m], sx[m], sxx[m], ll[m]
    return np.concatenate([sx, sxx, np.asarray(nk)[:, None]], axis=1).astype(np.float64), float(ll)


# ------------------------------------------------------------------------------------------------- the comparison
MAX_FACTOR, RMS_FACTOR = 8.0, 3.0
RMS_MIN_NK, RMS_MIN_MIX = 8.0, 4


def _norm_err(v, ref):
    """e(v): |v - ref64| / den per entry; an entry made of nothing (den = 0: an all-zero feature column) must be exact"""
    den = ref["s"] + 2.0 ** -100 * ref["A"][None, :]
    err = np.abs(np.asarray(v, dtype=np.float64) - ref["block"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v)))) if np.size(v) else 0.0


def limits(ev, L):
    """the four limits of the rule for one evaluation and L frames per accumulator (module docstring)"""
    ref, emu = ev["ref"], ev["emu"]
    ee = _norm_err(emu["block"], ref)
    rows = ref["nk"] >= RMS_MIN_NK
    d = np.asarray(emu["lse"], dtype=np.float64) - ref["lse"]
    n = ref["n"]
    mx = MAX_FACTOR * float(ee.max()) + 2.0 ** -20 + L * 2.0 ** -24
    return dict(max=mx, rms=RMS_FACTOR * _rms(ee[rows]) + 2.0 ** -22, rms_rows=rows, rms_applies=int(rows.sum()) >= RMS_MIN_MIX,
                ll=MAX_FACTOR * max(abs(float(d.sum())), np.sqrt(n) * _rms(d)) + 2.0 ** -22 * float((np.abs(ref["lse"]) + 1).sum()),
                mass=n * mx, emu_max=float(ee.max()), emu_rms=_rms(ee[rows]))


def measure(got, ev, L, what="", m=None):
    """the measured ratios of one result under the rule (error over its limit: max_ratio, rms_ratio — None when the rms rule is skipped —
    ll_ratio, mass_ratio, worst: the largest of them; max_vs_emu: the error over emu32's own; message: what compare raises with).
    got: an api result (model m of a batched one) or an emulation's dict; ev: evaluate(...); L: acc_frames(...)."""
    ref = ev["ref"]
    block, ll = block_of(got, m)
    assert block.shape == ref["block"].shape, (what, block.shape, ref["block"].shape)
    if not (np.isfinite(block).all() and np.isfinite(ll)):
        raise AssertionError("%s: %d entries are not finite" % (what, int((~np.isfinite(block)).sum()) + int(not np.isfinite(ll))))
    lim = limits(ev, L)
    e = _norm_err(block, ref)
    res = dict(max_ratio=float(e.max()) / lim["max"], max_err=float(e.max()),
               rms_ratio=(_rms(e[lim["rms_rows"]]) / lim["rms"]) if lim["rms_applies"] else None, rms_skipped=not lim["rms_applies"],
               ll_ratio=abs(ll - ref["ll"]) / lim["ll"], ll_err=abs(ll - ref["ll"]),
               mass_ratio=abs(float(block[:, -1].sum()) - ref["n"]) / lim["mass"],
               emu_max=lim["emu_max"], emu_rms=lim["emu_rms"], max_vs_emu=float(e.max()) / max(lim["emu_max"], 1e-300), limits=lim)
    res["worst"] = max(res["max_ratio"], res["rms_ratio"] or 0.0, res["ll_ratio"], res["mass_ratio"])
    k, j = np.unravel_index(int(np.argmax(e)), e.shape)
    res["message"] = ("%s: ratios to the limits: max %.3g (entry [%d, %d], e = %.3g, emu32 %.3g), rms %s, loglik %.3g (error %.3g), mass %.3g"
                      % (what, res["max_ratio"], k, j, res["max_err"], res["emu_max"],
                         "skipped" if res["rms_skipped"] else "%.3g" % res["rms_ratio"], res["ll_ratio"], res["ll_err"], res["mass_ratio"]))
    return res


def compare(got, ev, L, what="", m=None):
    """The one rule of the EM instance files: measure(...), and AssertionError when a ratio exceeds 1."""
    res = measure(got, ev, L, what, m)
    if res["worst"] > 1.0:
        raise AssertionError(res["message"])
    return res


def agree(got_a, L_a, got_b, L_b, ev, what="", m_a=None, m_b=None):
    """two routes' results for one evaluation agree within the sum of their two limits (max rule, loglik and mass)"""
    (ba, la), (bb, lb) = block_of(got_a, m_a), block_of(got_b, m_b)
    a, b = limits(ev, L_a), limits(ev, L_b)
    den = ev["ref"]["s"] + 2.0 ** -100 * ev["ref"]["A"][None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(den > 0, np.abs(ba - bb) / den, np.where(ba == bb, 0.0, np.inf))
    assert float(e.max()) <= a["max"] + b["max"], (what, float(e.max()), a["max"] + b["max"])
    assert abs(la - lb) <= a["ll"] + b["ll"], (what, abs(la - lb), a["ll"] + b["ll"])


def old_rule_accepts(got, ev):
    """the `1e-4 * max` rule of the older EM tests (tests/test_gpu_parity.py, tests/test_gmm_em_batch.py), for the host file's mutation"""
    block, ll = block_of(got)
    ref = ev["ref"]["block"]
    D = ev["D"]
    ok = abs(ll - ev["ref"]["ll"]) <= 1e-5 * abs(ev["ref"]["ll"])
    for sl in (slice(0, D), slice(D, 2 * D), slice(2 * D, 2 * D + 1)):
        ok = ok and np.allclose(block[:, sl], ref[:, sl], rtol=1e-4, atol=1e-4 * np.abs(ref[:, sl]).max())
    return bool(ok)


# ------------------------------------------------------------------------------------------------- case builders
LENS = (1, 63, 64, 65, 129, 209)   # frames per model: the 64-frame tile and the 16-frame wave split on their edges
SWEEP_D = (1, 2, 3, 4, 7, 13, 15, 16, 17, 26, 31, 32, 33, 39, 46, 47, 48, 49, 60, 63, 64)
SWEEP_K = (1, 5, 31, 32, 33, 63, 64, 65, 70, 128, 129)
# the unfused NCT = 1 and NCT = 2 instances, single and batched; (33, 26): the rotation gives every D in 16 .. 31 a K > 64, and the
# fused NCT = 2 instances would go unreached
SWEEP_FIXED = ((70, 7), (70, 15), (129, 16), (70, 31), (33, 26))
HARD_SHAPES = ((16, 39), (64, 13), (70, 13), (129, 26))
HARD_KINDS = ("uncentred10", "uncentred30", "uncentred100", "wide_cov", "skewed_w", "identical", "outliers")
LATE_D = 39
CAP_SHAPES = (("single", 64, 47), ("single", 5, 7), ("single", 70, 16), ("single", 5, 60), ("batch", 512, 39), ("batch", 70, 15))

_CACHE = {}


def sweep_shapes():
    return tuple((SWEEP_K[i % len(SWEEP_K)], D) for i, D in enumerate(SWEEP_D)) + SWEEP_FIXED


def _draw_models(rng, K, D, M, spread=0.3):
    base = rng.standard_normal((K, D))
    w = rng.dirichlet(5 * np.ones(K), M)
    cov = rng.uniform(0.5, 2.0, (M, K, D))
    mus = base[None] + spread * np.sqrt(cov) * rng.standard_normal((M, K, D))
    return w, mus, cov


def _draw_frames(rng, w, mu, cov, n):
    comp = rng.choice(len(w), size=n, p=w / w.sum())
    return (mu[comp] + np.sqrt(cov[comp]) * rng.standard_normal((n, mu.shape[1]))).astype(np.float32)


def _case(name, family, w, mus, cov, feats, **extra):
    c = dict(name=name, family=family, w=w, mus=mus, cov=cov, feats=[np.ascontiguousarray(f, dtype=np.float32) for f in feats],
             lens=[len(f) for f in feats], M=mus.shape[0], K=mus.shape[1], D=mus.shape[2], _ev={})
    c.update(extra)
    return c


def ev_of(c, m, pm=None):
    """the evaluations of model pm's parameters (default: m's own) over model m's frames, computed once per case"""
    pm = m if pm is None else pm
    if (pm, m) not in c["_ev"]:
        c["_ev"][(pm, m)] = evaluate(c["w"][pm], c["mus"][pm], c["cov"][pm], c["feats"][m])
    return c["_ev"][(pm, m)]


def alt_of(c, m):
    if ("alt", m) not in c["_ev"]:
        c["_ev"][("alt", m)] = emu32_alt(c["w"][m], c["mus"][m], c["cov"][m], c["feats"][m])
    return c["_ev"][("alt", m)]


def yardstick_ratios(c, m, entry="single", num_cu=NUM_CU_DEFAULT):
    """emu32_alt of model m under the rule: the ratios compare returns (it raises above 1)"""
    return compare(alt_of(c, m), ev_of(c, m), acc_frames(c["lens"][m], walk_cap(entry, c["K"], num_cu)), c["name"] + " emu32_alt")


def construction_ok(c):
    """The construction conditions every case is built to (the host file asserts them): emu32_alt, a different legitimate float32
    evaluation, stays at or below half of every limit on every model, an uncentred case's mixtures overlap (at least 5 % of its
    frames have a second-best float64 responsibility above 0.05), and lone_frames_are_typical."""
    try:
        for m in range(c["M"]):
            if yardstick_ratios(c, m)["worst"] > 0.5:
                return False
    except AssertionError:
        return False
    if c["family"].startswith("uncentred") and overlap_share(c) < 0.05:
        return False
    return lone_frames_are_typical(c)


def lone_frames_are_typical(c):
    """The loglik limit of a model of fewer than 8 frames rests on emu32's error on those few frames: 8 sqrt(n) rms d.  Where emu32
    happens to round them right (|d| a twentieth of an ulp of the exponent's terms: seen at the 1-frame model of an uncentred case) the
    limit says nothing about float32 evaluation, and a correct kernel one ulp off misses it.  Condition, on emu32 alone: the rms of d over
    such a model's frames is at least the rms of d over all frames of the case (same shape, same kind of parameters)."""
    d = [np.asarray(ev_of(c, m)["emu"]["lse"], dtype=np.float64) - ev_of(c, m)["ref"]["lse"] for m in range(c["M"])]
    pooled = _rms(np.concatenate(d))
    return all(_rms(dm) >= pooled for dm in d if len(dm) < 8)


def _search(key, base_seed, make):
    """The case of the first seed among base_seed, base_seed + 1, ... at which the construction conditions hold: the seed moves, never a
    limit.  What moves it: the loglik limit of the 1-frame model is 8 |d_0| + 2^-22 (|lse| + 1) with d_0 emu32's error on that ONE frame —
    where emu32 happens to round that frame right, a float32 kernel a few ulp of |lp| off has no room; and emu32_alt, which starts from
    the constant and adds every term at the full magnitude of the exponent, is at D >= 33 often more than 4 x emu32's largest error away;
    lone_frames_are_typical asks that emu32's error on the 1-frame model is no lucky draw."""
    if key not in _CACHE:
        for i in range(400):
            c = make(np.random.default_rng(base_seed + i))
            if construction_ok(c):
                c["seed"], c["seeds_skipped"] = base_seed + i, i
                _CACHE[key] = c
                break
        else:
            raise AssertionError("no seed in 400 gives case %r its construction conditions" % (key,))
    return _CACHE[key]


def sweep_case(K, D):
    """the width sweep: centred data, every model its own parameters, its frames drawn from it"""
    def make(rng):
        w, mus, cov = _draw_models(rng, K, D, len(LENS))
        feats = [_draw_frames(rng, w[m], mus[m], cov[m], n) for m, n in enumerate(LENS)]
        return _case("sweep_K%d_D%d" % (K, D), "sweep", w, mus, cov, feats)
    return _search(("sweep", K, D), 100000 + 1000 * sweep_shapes().index((K, D)), make)


def overlap_share(c):
    """share of a case's frames whose second-best float64 responsibility exceeds 0.05"""
    second = np.concatenate([np.sort(ev_of(c, m)["ref"]["resp"], axis=1)[:, -2] for m in range(c["M"])])
    return float((second > 0.05).mean())


def hard_case(kind, K, D):
    def make(rng):
        M = len(LENS)
        w, mus, cov = _draw_models(rng, K, D, M)
        extra = {}
        if kind.startswith("uncentred"):
            # ONE common offset, ratio sigma in every column, the mixture means spread 0.7 around it: the expansion's terms are ratio^2
            # larger than their sum while the mixtures still overlap (an offset scaled per mixture by sqrt(cov) separates them: resp 0 or 1)
            ratio = float(kind[len("uncentred"):])
            mus = ratio * rng.choice([-1.0, 1.0], D) + 0.7 * rng.standard_normal((M, K, D))
            extra["ratio"] = ratio
        elif kind == "wide_cov":
            cov = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), (M, K, D)))
        elif kind == "skewed_w":
            w = np.maximum(rng.dirichlet(0.02 * np.ones(K), M), 1e-300)
        elif kind == "identical":
            w = np.full((M, K), 1.0 / K)
            mus = np.repeat(mus[:, :1], K, axis=1)
            cov = np.repeat(cov[:, :1], K, axis=1)
        if kind == "outliers":
            reach = np.abs(mus).max() + 50.0 * np.sqrt(2.0)   # 50 sigma of the widest mixture (cov <= 2) beyond the farthest mean
            feats = [(reach * rng.choice([-1.0, 1.0], (n, D)) * rng.uniform(1.0, 1.05, (n, D))).astype(np.float32) for n in LENS]
        else:
            feats = [_draw_frames(rng, w[m], mus[m], cov[m], n) for m, n in enumerate(LENS)]
        return _case("%s_K%d_D%d" % (kind, K, D), kind, w, mus, cov, feats, **extra)
    return _search((kind, K, D), 200000 + 10000 * HARD_KINDS.index(kind) + 1000 * HARD_SHAPES.index((K, D)), make)


def late_dominant_case():
    """K = 70: the frames belong to mixture 69, in the padded second chunk (mixtures 64 .. 69 + 58 pads), and every other mixture is more
    than 300 nats below it"""
    K, D, M = 70, LATE_D, len(LENS)

    def make(rng):
        w, mus, cov = _draw_models(rng, K, D, M)
        mus[:, 69] += 15.0 * np.sqrt(cov[:, 69]) * rng.choice([-1.0, 1.0], D)
        feats = [(mus[m, 69] + 0.5 * np.sqrt(cov[m, 69]) * rng.standard_normal((n, D))).astype(np.float32) for m, n in enumerate(LENS)]
        return _case("late_dominant_K70_D%d" % D, "late_dominant", w, mus, cov, feats)
    return _search(("late",), 300000, make)


def late_gap(c):
    """smallest lead of mixture 69 over the best other mixture, in nats, over every frame of the case"""
    gaps = []
    for m in range(c["M"]):
        lp = O.gmm_log_prob(c["w"][m], c["mus"][m], c["cov"][m], c["feats"][m])
        gaps.append((lp[:, 69] - np.delete(lp, 69, axis=1).max(axis=1)).min())
    return float(min(gaps))


def cap_frames(entry, K, num_cu=NUM_CU_DEFAULT):
    """64 (cap + 3) + 17 frames: three walkers take a second tile, the last tile is partial"""
    return EM_TF * (walk_cap(entry, K, num_cu) + 3) + 17


def cap_case(entry, K, D, num_cu=NUM_CU_DEFAULT):
    """one model past the walker cap of its entry point (centred data)"""
    key = ("cap", entry, K, D, num_cu)
    if key not in _CACHE:
        rng = np.random.default_rng(777 + 10 * K + D)
        w, mus, cov = _draw_models(rng, K, D, 1)
        feats = [_draw_frames(rng, w[0], mus[0], cov[0], cap_frames(entry, K, num_cu))]
        _CACHE[key] = _case("cap_%s_K%d_D%d" % (entry, K, D), "cap", w, mus, cov, feats, entry=entry, num_cu=num_cu)
    return _CACHE[key]


def small_mixture_case():
    """the host file's mean-shift mutation: 8000 frames, K = 16, D = 13, one mixture with about two frames' worth of mass"""
    key = ("small",)
    if key not in _CACHE:
        K, D = 16, 13
        rng = np.random.default_rng(1613)
        w, mus, cov = _draw_models(rng, K, D, 1)
        w[0, 3] = 2.5e-4 * w[0].sum()
        w[0] /= w[0].sum()
        mus = mus * 2.0   # (apart enough that the small mixture keeps what is drawn from it)
        _CACHE[key] = _case("small_mixture_K16_D13", "small", w, mus, cov, [_draw_frames(rng, w[0], mus[0], cov[0], 8000)])
    return _CACHE[key]


def case_ids():
    """every case of the GPU file: (id, builder arguments)"""
    ids = [("sweep_K%d_D%d" % kd, ("sweep",) + kd) for kd in sweep_shapes()]
    ids += [("%s_K%d_D%d" % ((kind,) + kd), ("hard", kind) + kd) for kind in HARD_KINDS for kd in HARD_SHAPES]
    ids.append(("late_dominant_K70_D%d" % LATE_D, ("late",)))
    return ids


def calls_of(c):
    """the (entry, label, env names) calls tests/test_em_instances_gpu.py makes on a case: every route that exists for its shape; a
    walker-cap case runs the default route of its own entry point"""
    if c["family"] == "cap":
        return [(c["entry"], "default", ())]
    calls = [("single", label, env) for label, env in single_routes(c["K"], c["D"])]
    if c["D"] <= MAX_D_MFMA:
        calls += [("batch", "default", ()), ("shared", "default", ())]
    return calls


def all_specs(num_cu=NUM_CU_DEFAULT):
    """every case of the GPU file, the walker-cap cases included: (id, builder arguments)"""
    return case_ids() + [("cap_%s_K%d_D%d" % s, ("cap",) + s + (num_cu,)) for s in CAP_SHAPES]


def build(spec):
    if spec[0] == "sweep":
        return sweep_case(*spec[1:])
    if spec[0] == "hard":
        return hard_case(*spec[1:])
    if spec[0] == "late":
        return late_dominant_case()
    if spec[0] == "cap":
        return cap_case(*spec[1:])
    raise KeyError(spec)
