"""Cases, references and the one comparison rule of tests/test_cosine_instances_host.py and tests/test_cosine_instances_gpu.py: every
compiled instance of the cosine scorer (csrc/cosine.hip: cosine_reg_kernel<NQ>, cosine_bf16x3_kernel<NK, SPLIT>, the tiled cosine_kernel)
against float64, with margins on, below and above the error bands that decide which rows a split-precision sweep may settle by itself.

Evaluations of one case:
  ref64    oracle.ref_cpu.cosine_matrix on the float32 inputs: float64, the truth.
  emu32    a float32 numpy restatement of the fp32 kernel's formula: the centroid rows normalised in float32 as cos_pack_kernel does
           (float32 sum of squares, 1 / sqrt, one multiply per entry), the d products added one at a time in float32 in increasing k, one
           multiply by the float32 1 / sqrt(ss) of the embedding, 1 -, the clip to [0, 2].  It is the YARDSTICK: what float32 evaluation
           of this formula costs by reference arithmetic alone.  (tiled=True restates cosine_kernel, d > 256: raw centroids, two multiplies.)
  emu_hi   the hi-parts sweep (SPLIT = 1) and the bf16x3 sweep (SPLIT = 3) on the float32-normalised operands with round-to-nearest-even
  emu_x3   bf16: products of bf16 numbers are exact, they are summed in float64.  What is left of the difference to ref64 is what the
           SPLIT costs, and that is what cos_band1 / cos_band bound.
  got      the library.

The comparison of distances and minima at precision 0 (compare): over the finite entries of a case
  max   |got - ref64| <= 8 max|emu32 - ref64| + 2^-20 (|ref64| + 1)        per entry   (|dist| <= 2: at most 12 ulp of 2)
  rms   rms(got - ref64) <= 3 rms(emu32 - ref64) + 2^-22 (rms|ref64| + 1)
with the factors and floors of tests/gmm_cases.py and that file's reasoning: two float32 evaluations of one formula that differ in
summation order have RMS errors within a small factor of each other, their maxima over 1e4 .. 1e5 entries spread wider, and the MFMA
can only round less often than emu32 does.  The margins come from that reasoning, not from a run: a ratio above 1 is a finding.

The arg-min rule at EVERY precision (check_argmin), with tol the per-entry limit of the max rule: where the float64 margin of the two best
exceeds 2 tol the index is float64's; elsewhere the chosen index's float64 distance is within 2 tol of the minimum; and the chosen index is
the first of the centroids that are bit-identical to it.  The split-precision paths promise the fp32 path's arg-min on every row
(include/ssp.h), the fp32 path is within tol of float64, so one rule serves all of them — and fails when an error band is too small.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_cpu as O  # noqa: E402

MAX_FACTOR, RMS_FACTOR = 8.0, 3.0
U_BF16 = 2.0 ** -8   # unit roundoff of bf16 (8-bit significand, round to nearest)


# ---- the instance tables of csrc/cosine.hip, restated
def pick_nq(d):
    """cosine_reg_kernel<NQ>: k-depth / 8; -1: the tiled cosine_kernel"""
    return 8 if d <= 64 else 16 if d <= 128 else 24 if d <= 192 else 32 if d <= 256 else -1


def pick_nk(d):
    """cosine_bf16x3_kernel<NK, SPLIT>: k-steps of 16; 0: no split-precision instance"""
    return 4 if d <= 64 else 8 if d <= 128 else 12 if d <= 192 else 16 if d <= 256 else 0


def instance(d, precision):
    if pick_nq(d) < 0:
        return "tiled cosine_kernel BK=32"
    reg = "cosine_reg NQ=%d" % pick_nq(d)
    if precision == 0:
        return reg
    x3 = "bf16x3 NK=%d SPLIT=3" % pick_nk(d)
    return "%s > %s" % (x3, reg) if precision == 1 else "bf16x3 NK=%d SPLIT=1 > %s > %s" % (pick_nk(d), x3, reg)


# ---- the bands of include/ssp.h (csrc/cosine.hip cos_band, cos_band1), restated; OLD_*: the constants before the correction, which took
#      the unit roundoff of bf16 for 2^-9
def norm_slack(d):
    return (d + 8) * 2.0 ** -24


def band(d):
    return 3.01 * 2.0 ** -16 + 4.0 * d * 2.0 ** -23 * 1.02 + norm_slack(d)


def band1(d):
    return 2.01 * 2.0 ** -8 + 2.0 * d * 2.0 ** -23 * 1.01 + norm_slack(d)


def old_band(d):
    return 3.01 * 2.0 ** -18 + 4.0 * d * 2.0 ** -23 * 1.01 + norm_slack(d)


def old_band1(d):
    return 2.01 * 2.0 ** -9 + 2.0 * d * 2.0 ** -23 * 1.01 + norm_slack(d)


def order_slack(d):
    """what the matrix core's undocumented summation order may move a sweep's cosine by, against the float64 sum of the emulation"""
    return 4.0 * d * 2.0 ** -23


# ------------------------------------------------------------------------------------------------- references
def bf16_rne(v):
    """float32 -> the nearest bf16 (ties to even), returned as float32.  Finite input."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    b = v.view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def unit32(A):
    """rows of A normalised as the kernels do: float32 sum of squares in increasing k, 1 / sqrt in float32, one multiply per entry.
    Returns (A_hat float32, inv float32)"""
    A = np.asarray(A, dtype=np.float32)
    ss = np.zeros(A.shape[0], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(A.shape[1]):
            ss = ss + A[:, k] * A[:, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (np.float32(1.0) / np.sqrt(ss)).astype(np.float32)
        return (A * inv[:, None]).astype(np.float32), inv


def ref64(X, C):
    return O.cosine_matrix(np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32))


def emu32(X, C, tiled=False):
    """(N, S) float32 distances: the fp32 kernel's formula in float32 numpy, see the module docstring"""
    X, C = np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32)
    _, ix = unit32(X)
    chat, inc = unit32(C)
    A = C if tiled else chat
    acc = np.zeros((X.shape[0], C.shape[0]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(X.shape[1]):
            acc = acc + X[:, k:k + 1] * A[None, :, k]   # float32 product, float32 sum, one term at a time
        if tiled:
            acc = acc * inc[None, :]
        dv = np.float32(1.0) - acc * ix[:, None]
    assert dv.dtype == np.float32
    return np.where(np.isnan(dv), dv, np.clip(dv, np.float32(0.0), np.float32(2.0)))


def split_cosines(X, C):
    """(cos_hi, cos_x3), each (N, S) float64: the two sweeps' cosines by emulation, see the module docstring"""
    xh_, _ = unit32(X)
    ch_, _ = unit32(C)
    xh, ch = bf16_rne(xh_), bf16_rne(ch_)
    xl, cl = bf16_rne(xh_ - xh), bf16_rne(ch_ - ch)    # (v - hi is exact in float32)
    xh, xl, ch, cl = (a.astype(np.float64) for a in (xh, xl, ch, cl))
    hh = xh @ ch.T
    return hh, hh + xl @ ch.T + xh @ cl.T


def top2(cos):
    """(best, second, arg-max) of a (N, S) cosine matrix, first index on ties; second = -inf with one centroid"""
    am = cos.argmax(axis=1)
    rows = np.arange(len(cos))
    b1 = cos[rows, am]
    if cos.shape[1] == 1:
        return b1, np.full(len(cos), -np.inf), am
    rest = cos.copy()
    rest[rows, am] = -np.inf
    return b1, rest.max(axis=1), am


# ------------------------------------------------------------------------------------------------- the comparison
def entry_tolerance(ref, emu):
    """per-entry limit of the max rule (same shape as ref; NaN where ref is NaN)"""
    ref = np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    e = np.abs(np.asarray(emu, dtype=np.float64) - ref)[fin]
    return MAX_FACTOR * (e.max() if e.size else 0.0) + 2.0 ** -20 * (np.abs(ref) + 1)


def compare(got, ref, emu, what=""):
    """The one rule for distances and minima at precision 0.  Entries where ref is NaN are left out: the caller checks them.  Returns the
    measured ratios and raises AssertionError when one exceeds 1."""
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


def first_of_duplicates(C):
    """(S,) for every centroid the first index of a bit-identical row"""
    C = np.ascontiguousarray(C, dtype=np.float32)
    first = {}
    return np.array([first.setdefault(C[j].tobytes(), j) for j in range(len(C))], dtype=np.int64)


def argmin_split(ref, tol, C):
    """the rows of the exact check: (clear (N,) bool, ref arg-min with duplicates resolved to the first, margin).  A row whose two best
    are bit-identical centroids is clear when the next DIFFERENT centroid is: the answer there is the first of the duplicates."""
    ref = np.asarray(ref, dtype=np.float64)
    rows = np.arange(len(ref))
    fod = first_of_duplicates(C)
    am = ref.argmin(axis=1)                                   # numpy: the first index of equal values
    rest = np.where(fod[None, :] == fod[am][:, None], np.inf, ref)   # every copy of the best centroid out of the way
    second = rest.argmin(axis=1)
    margin = rest[rows, second] - ref[rows, am]
    t = np.maximum(tol[rows, am], tol[rows, second]) if np.ndim(tol) == 2 else tol
    return margin > 2 * t, fod[am], margin


def check_argmin(got, ref, tol, C, what=""):
    """The arg-min rule on the rows whose reference row is finite.  Returns the share of rows left out of the exact check."""
    got = np.asarray(got).astype(np.int64)
    ref = np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref).all(axis=1)
    assert fin.any(), what
    assert ((got >= 0) & (got < ref.shape[1])).all(), (what, "an index out of range")
    tol2 = np.broadcast_to(tol, ref.shape)
    clear, want, _ = argmin_split(ref[fin], tol2[fin], C)
    g = got[fin]
    bad = np.flatnonzero(clear & (g != want))
    if bad.size:
        raise AssertionError("%s: %d rows with a float64 margin above 2 tol have another arg-min (first: row %d, got %d, float64 %d)"
                             % (what, bad.size, np.flatnonzero(fin)[bad[0]], g[bad[0]], want[bad[0]]))
    rows = np.arange(len(g))
    r = ref[fin]
    gap = r[rows, g] - r.min(axis=1)
    lim = 2 * np.maximum(tol2[fin][rows, g], tol2[fin][rows, r.argmin(axis=1)])
    if (gap > lim).any():
        i = int(np.argmax(gap - lim))
        raise AssertionError("%s: row %d: the chosen centroid is %.3e above the float64 minimum (2 tol = %.3e)" % (what, np.flatnonzero(fin)[i], gap[i], lim[i]))
    fod = first_of_duplicates(C)
    if not np.array_equal(fod[g], g):
        raise AssertionError("%s: a duplicated centroid was not reported at its first index" % what)
    return float(1.0 - clear.mean())


def check_min(got_min, ref, allowed, what=""):
    """|min - ref64 min| <= allowed (scalar or (N,)) on the finite reference rows; returns the largest error / allowed"""
    ref = np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref).all(axis=1)
    g = np.asarray(got_min, dtype=np.float64)[fin]
    if not np.isfinite(g).all():
        raise AssertionError("%s: a minimum is not finite where the reference is" % what)
    ratio = np.abs(g - ref[fin].min(axis=1)) / np.broadcast_to(allowed, fin.shape)[fin]
    if ratio.max() > 1.0:
        raise AssertionError("%s: a minimum is %.2f x its allowance from float64's" % (what, ratio.max()))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------- cases
_CACHE = {}


def _finish(name, X, C, tiled=False, emulate=True, **extra):
    X, C = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(C, dtype=np.float32)
    c = dict(name=name, X=X, C=C, N=X.shape[0], S=C.shape[0], d=X.shape[1], ref=ref64(X, C), emu=emu32(X, C, tiled=tiled))
    c["tol"] = entry_tolerance(c["ref"], c["emu"])
    if emulate and pick_nk(c["d"]):
        c["cos_hi"], c["cos_x3"] = split_cosines(X, C)
    c.update(extra)
    return c


def left_out_share(c):
    fin = np.isfinite(c["ref"]).all(axis=1)
    if c["S"] == 1:
        return 0.0
    clear, _, _ = argmin_split(c["ref"][fin], c["tol"][fin], c["C"])
    return float(1.0 - clear.mean())


SWEEP_D = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
SWEEP_S = (1, 2, 31, 32, 33, 64, 65, 97)
SWEEP_N = 389            # three 128-row workgroups + 5 rows
SMALL_N = ((17, 1), (64, 127), (129, 128), (256, 129))   # one width each at N around the workgroup
LEFT_OUT_CAP = 0.01


def sweep_S(d):
    return SWEEP_S[SWEEP_D.index(d) % len(SWEEP_S)]


def _random_case(name, N, S, d, seed0, tiled=False):
    """centroids of norms over two decades, every embedding a noisy copy of one of them; the seed is the first of seed0, seed0 + 1, ... at
    which at most LEFT_OUT_CAP of the rows are left out of the exact arg-min check — the seed moves, never the limit"""
    for seed in range(seed0, seed0 + 200):
        rng = np.random.default_rng(seed)
        C = rng.standard_normal((S, d)) * 10.0 ** rng.uniform(-1, 1, (S, 1))
        lab = rng.integers(0, S, N)
        X = C[lab] / np.linalg.norm(C[lab], axis=1, keepdims=True) * np.sqrt(d) + 0.7 * rng.standard_normal((N, d))
        c = _finish(name, X, C, tiled=tiled, seed=seed, label=lab)
        if left_out_share(c) <= LEFT_OUT_CAP:
            return c
    raise AssertionError("no seed in 200 keeps case %s under the cap" % name)


def sweep_case(d):
    key = ("sweep", d)
    if key not in _CACHE:
        _CACHE[key] = _random_case("sweep_d%d" % d, SWEEP_N, sweep_S(d), d, 1000 * d)
    return _CACHE[key]


def head_of(c, N):
    """the first N rows of a case as a case of its own (the references are per row; tol stays the whole case's)"""
    h = dict(c)
    h.update(name="%s_N%d" % (c["name"], N), N=N)
    for k in ("X", "ref", "emu", "tol", "cos_hi", "cos_x3", "label"):
        if k in c:
            h[k] = c[k][:N]
    return h


TILED = tuple((d, S, N) for d, S, N in ((257, 1, 1), (257, 128, 300), (288, 127, 129), (320, 129, 300), (511, 128, 129), (511, 1, 300),
                                        (288, 129, 1), (320, 127, 1)))


def tiled_case(d, S, N):
    key = ("tiled", d, S, N)
    if key not in _CACHE:
        _CACHE[key] = _random_case("tiled_d%d_S%d_N%d" % (d, S, N), N, S, d, 7 * d + S + N, tiled=True)
    return _CACHE[key]


# ---- the margin ladder
LADDER_D = (16, 64, 128, 192, 256)
RUNGS = (0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 8.0)
ROWS_PER_RUNG = 64
LADDER_AT = (1, 30, 31, 32, 33, 38, 5, 17)   # where the four pairs sit among S = 40 centroids: both sides of the 32-row tile edge
LADDER_S = 40


def ladder_case(d):
    """Four pairs of orthogonal centroids among 40; row i has cosine 0.5 with one of a pair and 0.5 - m_i with the other, its remaining
    length orthogonal to all eight, m_i = band(d) x RUNGS then band1(d) x RUNGS, 64 rows a rung, the rows shuffled.  The 32 other centroids
    point away from every pair (cosine <= 0.3 with every row).  Which of the pair wins alternates."""
    key = ("ladder", d)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(500 + d)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    E = Q[:, :8].T                                  # the pairs' directions
    rest = Q[:, 8:]                                 # d - 8 directions orthogonal to them
    target = np.concatenate([np.repeat(b * np.asarray(RUNGS), ROWS_PER_RUNG) for b in (band(d), band1(d))])
    which = np.concatenate([np.repeat(w, len(RUNGS) * ROWS_PER_RUNG) for w in (0, 1)])   # 0: a rung of band, 1: of band1
    N = len(target)
    pair = np.arange(N) % 4
    flip = (np.arange(N) // 4) % 2
    n = rng.standard_normal((N, d - 8)) @ rest.T
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    a, b = np.full(N, 0.5), 0.5 - target
    X = np.sqrt(1.0 - a * a - b * b)[:, None] * n
    win, lose = 2 * pair + flip, 2 * pair + 1 - flip
    X += a[:, None] * E[win] + b[:, None] * E[lose]
    C = np.empty((LADDER_S, d))
    others = [j for j in range(LADDER_S) if j not in LADDER_AT]
    for i, j in enumerate(others):
        v = -E[i % 8] + 0.2 * rng.standard_normal(d) / np.sqrt(d)
        C[j] = v
    C[list(LADDER_AT)] = E
    C *= 10.0 ** rng.uniform(-1, 1, (LADDER_S, 1))
    X *= 10.0 ** rng.uniform(-1, 1, (N, 1))
    perm = rng.permutation(N)
    at = np.asarray(LADDER_AT)
    c = _finish("ladder_d%d" % d, X[perm], C, target=target[perm], which=which[perm], win=at[win][perm], lose=at[lose][perm])
    _CACHE[key] = c
    return c


def listed(cos, band2, slack):
    """rows a sweep with the cosines `cos` hands on: (certainly, possibly) — its margin below twice the band minus / plus the slack"""
    b1, b2, _ = top2(cos)
    m = b1 - b2
    return m < band2 - slack, m < band2 + slack


# ---- device-side list lengths
LIST_L = (0, 1, 31, 32, 33, 127, 128, 129)
LIST_N, LIST_S, LIST_D = 1000, 40, 64


def list_case(L):
    """N = 1000 rows of which exactly L (at the first L places of one fixed shuffle) sit beside a near-duplicate pair of centroids
    (6 and 37: 1e-6 apart); every other row belongs to a centroid without a twin.  The centroids and the other rows are the same for
    every L."""
    key = ("list", L)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(6400)
    C = rng.standard_normal((LIST_S, LIST_D))
    C[37] = C[6] * (1.0 + 1e-6 * rng.standard_normal(LIST_D))
    singles = np.array([j for j in range(LIST_S) if j not in (6, 37)])
    lab = singles[rng.integers(0, len(singles), LIST_N)]
    Z = rng.standard_normal((LIST_N, LIST_D))
    places = rng.permutation(LIST_N)
    lab = lab.copy()
    lab[places[:L]] = 6
    X = C[lab] + 0.3 * Z
    close = np.zeros(LIST_N, bool)
    close[places[:L]] = True
    c = _finish("list_L%d" % L, X, C, close=close)
    _CACHE[key] = c
    return c


# ---- duplicates across tiles
def duplicate_case(d, S=70):
    key = ("dup", d, S)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(3500 + d)
    C = rng.standard_normal((S, d)).astype(np.float32)
    C[35] = C[3]
    C[S - 1] = C[3]
    lab = rng.integers(0, S, 200)
    lab[::2] = (3, 35, S - 1, 3)[d % 4]
    X = C[lab] + 0.4 * rng.standard_normal((200, d))
    c = _finish("duplicates_d%d" % d, X, C, label=lab)
    _CACHE[key] = c
    return c


# ---- row norms
def norms_case(d):
    """rows scaled by 2^e, e uniform in [-40, 40], a zero row, a NaN row and an inf entry among them"""
    key = ("norms", d)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(4000 + d)
    S, N = 33, 300
    C = rng.standard_normal((S, d))
    lab = rng.integers(0, S, N)
    X = (C[lab] + 0.5 * rng.standard_normal((N, d))).astype(np.float32)
    e = rng.integers(-40, 41, N)
    e[:2] = (-40, 40)
    X = np.ldexp(X, e[:, None]).astype(np.float32)    # exact: a power of two
    X[7] = 0.0
    X[11, d // 3] = np.nan
    X[13, d // 2] = np.inf
    c = _finish("norms_d%d" % d, X, C, exponent=e, nan_rows=np.array([7, 11, 13]))
    _CACHE[key] = c
    return c


# ---- the auto path: d = 256, S = 1251, the smallest N the cost gate lets through to a pilot
AUTO_N = (47104, 47141)          # 368 workgroups; 368 workgroups + 37 rows
AUTO_S, AUTO_D = 1251, 256
AUTO_KINDS = {"separated": 2, "pairs": 1, "duplicates": 0}     # what the data forces the pilot to choose


def auto_case(kind):
    """The largest case: the float64 reference is taken 4096 rows at a time and only its per-row summary is kept (arg-min with duplicates
    resolved to the first, minimum, margin to the next DIFFERENT centroid); tol comes from emu32 on the first 256 rows, which can only
    make it smaller than the whole case's.
      separated   random centroids: every margin is far outside the bf16 sweep's band — the cascade
      pairs       625 centroids and a copy of each 5e-2 (relative, per entry) away: the two best cosines of a row are a pair, about 3e-3
                  apart — inside the bf16 sweep's band (1.6e-2), mostly outside the bf16x3 sweep's (3.7e-4): the bf16x3 sweep alone
      duplicates  625 centroids twice: every row an exact tie — fp32"""
    key = ("auto", kind)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(4700)
    N, S, d = AUTO_N[1], AUTO_S, AUTO_D
    C = rng.standard_normal((S, d)).astype(np.float32)
    lab = rng.integers(0, S, N)
    if kind == "pairs":
        C[625:1250] = C[:625] * (1.0 + 5e-2 * rng.standard_normal((625, d)).astype(np.float32))
        lab = lab % 625
    elif kind == "duplicates":
        C[625:1250] = C[:625]
        lab = lab % 625
    X = (C[lab] + 0.5 * rng.standard_normal((N, d)).astype(np.float32)).astype(np.float32)
    fod = first_of_duplicates(C)
    am, mn, margin, second = (np.empty(N, t) for t in (np.int64, np.float64, np.float64, np.float64))
    for r0 in range(0, N, 4096):
        ref = ref64(X[r0:r0 + 4096], C)
        rows = np.arange(len(ref))
        a = ref.argmin(axis=1)
        rest = np.where(fod[None, :] == fod[a][:, None], np.inf, ref)
        am[r0:r0 + 4096], mn[r0:r0 + 4096] = fod[a], ref[rows, a]
        second[r0:r0 + 4096] = rest.min(axis=1)
    margin = second - mn
    head_ref = ref64(X[:256], C)
    emax = float(np.abs(emu32(X[:256], C).astype(np.float64) - head_ref).max())
    tol = MAX_FACTOR * emax + 2.0 ** -20 * (second + 1)            # per row: the limit of the larger of its two best distances
    c = dict(name="auto_" + kind, X=X, C=C, N=N, S=S, d=d, ref_am=am, ref_min=mn, margin=margin, tol=tol, fod=fod, label=lab)
    _CACHE[key] = c
    return c


def check_argmin_summary(got, c, N, what=""):
    """the arg-min rule from the per-row summary of auto_case; returns the share of rows left out of the exact check"""
    got = np.asarray(got).astype(np.int64)[:N]
    assert ((got >= 0) & (got < c["S"])).all(), what
    am, tol, margin = c["ref_am"][:N], c["tol"][:N], c["margin"][:N]
    clear = margin > 2 * tol
    bad = np.flatnonzero(clear & (got != am))
    if bad.size:
        raise AssertionError("%s: %d rows with a float64 margin above 2 tol have another arg-min (first: row %d, got %d, float64 %d)"
                             % (what, bad.size, bad[0], got[bad[0]], am[bad[0]]))
    X64, G64 = c["X"][:N].astype(np.float64), c["C"][got].astype(np.float64)
    dist = 1.0 - (X64 * G64).sum(axis=1) / np.sqrt((X64 * X64).sum(axis=1) * (G64 * G64).sum(axis=1))
    if (dist - c["ref_min"][:N] > 2 * tol).any():
        raise AssertionError("%s: a chosen centroid is more than 2 tol above the float64 minimum" % what)
    if not np.array_equal(c["fod"][got], got):
        raise AssertionError("%s: a duplicated centroid was not reported at its first index" % what)
    return float(1.0 - clear.mean())


# ---- the host-fed sliced path: 1-MiB slices of d = 70 rows are 3744 rows, not a whole number of 128-row workgroups
def sliced_case():
    key = ("sliced",)
    if key not in _CACHE:
        _CACHE[key] = _random_case("host_sliced_d70", 8000, 40, 70, 7000)
    return _CACHE[key]


# ---- the worst triples of the host file's search with the constants before the correction (old_band1): float64 prefers centroid 0 by
#      more than 2 tol, the hi-parts sweep prefers centroid 1 by more than twice the old band.  (x, c0, c1) as found, float32.
OLD_BAND_TRIPLES = (
    ((-0.3237152099609375, -0.28664496541023254, -0.6035740971565247, 0.6702331304550171),
     (-0.32969117164611816, 0.043865058571100235, -1.1068459749221802, -0.29659202694892883),
     (-0.5277231335639954, -0.3684578537940979, 0.40262168645858765, 0.6576547622680664)),
)


def triple_case(i):
    x, c0, c1 = (np.asarray(v, dtype=np.float32) for v in OLD_BAND_TRIPLES[i])
    return _finish("old_band_triple_%d" % i, x[None, :], np.stack([c0, c1]))


# ------------------------------------------------------------------------------------------------- the band claims
def scan_family(d, n=4097):
    """x = c with all but one component equal, the common value scanned over [0.5, 1] / sqrt(d - 1) so that the normalised components
    cross bf16 midpoints; the last component completes the unit length.  d = 2: one scanned component.  Returns (X, C) with row i of X
    meant for row i of C."""
    t = np.linspace(0.5, 1.0, n) / np.sqrt(max(d - 1, 1))
    X = np.repeat(t[:, None], d, axis=1)
    X[:, -1] = np.sqrt(np.maximum(1.0 - (d - 1) * t * t, 0.0))
    X = X.astype(np.float32)
    return X, X.copy()


def random_pairs(d, n, seed):
    """seeded random unit vectors, each with a near-parallel partner (cosine about 0.99)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    C = X + 0.15 / np.sqrt(d) * rng.standard_normal((n, d)) * np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32), C.astype(np.float32)


def pair_all(X, C):
    """row i of X against row i of C: (ref64 cosine, emu32 distance, cos_hi, cos_x3), each (n,)"""
    X, C = np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32)
    xh_, ix = unit32(X)
    ch_, _ = unit32(C)
    acc = np.zeros(len(X), np.float32)
    for k in range(X.shape[1]):
        acc = acc + X[:, k] * ch_[:, k]
    dv = np.float32(1.0) - acc * ix
    emu = np.clip(dv, np.float32(0.0), np.float32(2.0))
    xh, ch = bf16_rne(xh_), bf16_rne(ch_)
    xl, cl = bf16_rne(xh_ - xh), bf16_rne(ch_ - ch)
    xh, xl, ch, cl = (a.astype(np.float64) for a in (xh, xl, ch, cl))
    hh = (xh * ch).sum(axis=1)
    x3 = hh + (xl * ch).sum(axis=1) + (xh * cl).sum(axis=1)
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    ref = (X64 * C64).sum(axis=1) / np.sqrt((X64 * X64).sum(axis=1) * (C64 * C64).sum(axis=1))
    return ref, emu, hh, x3


def pair_errors(X, C):
    """(|cos_hi - ref64|, |cos_x3 - ref64|) per row i for the pair (X[i], C[i])"""
    ref, _, hh, x3 = pair_all(X, C)
    return np.abs(hh - ref), np.abs(x3 - ref)


def band_errors(d):
    """the largest emulated error of either sweep over the scan family and 20 000 seeded random pairs"""
    key = ("band_errors", d)
    if key not in _CACHE:
        e = [pair_errors(*scan_family(d)), pair_errors(*random_pairs(d, 20000, 9000 + d))]
        _CACHE[key] = (max(float(v[0].max()) for v in e), max(float(v[1].max()) for v in e))
    return _CACHE[key]


def search_wrong_decision(d, split, band_of, steps=3000, climbers=64, seed=0):
    """A seeded, bounded hill climb over triples (x, c0, c1) for a WRONG DECISION of a sweep: float64 prefers c0 by more than 2 tol while
    the emulated sweep (split 1: hi parts, 3: bf16x3) prefers c1 by at least twice band_of(d) — a row the sweep would settle by itself,
    the wrong way.  `climbers` independent walks, each step moves one vector of each walk and keeps the move when it raises
        score = (sweep's cosine of c1 - of c0) - 2 band      while float64's margin for c0 stays above 2 tol.
    Returns (best score, the triple that has it as float32 arrays, its float64 margin): found when the score is >= 0."""
    rng = np.random.default_rng(seed + 100 * d + split)

    def evaluate(T):
        x, c0, c1 = T[:, 0], T[:, 1], T[:, 2]
        r0, e0, h0, t0 = pair_all(x, c0)
        r1, e1, h1, t1 = pair_all(x, c1)
        d0, d1 = np.clip(1.0 - r0, 0.0, 2.0), np.clip(1.0 - r1, 0.0, 2.0)
        emax = np.maximum(np.abs(e0 - d0), np.abs(e1 - d1))          # (a case of one row and two centroids)
        tol = MAX_FACTOR * emax + 2.0 ** -20 * (np.maximum(d0, d1) + 1)
        m64 = r0 - r1
        s = (h1 - h0) if split == 1 else (t1 - t0)
        return s - 2 * band_of(d), m64 > 2 * tol, m64

    # start: c1 made of c0's mirror image about x plus a little, so that the two cosines are nearly equal and c0 is just ahead
    x = rng.standard_normal((climbers, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    c0 = x + 1.2 * rng.standard_normal((climbers, d)) / np.sqrt(d)
    w = rng.standard_normal((climbers, d))
    w -= (w * x).sum(axis=1, keepdims=True) * x
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    cos0 = (x * c0).sum(axis=1) / np.linalg.norm(c0, axis=1)
    cos1 = cos0 - band_of(d)                        # float64 margin: about one band for c0
    c1 = cos1[:, None] * x + np.sqrt(1 - cos1 ** 2)[:, None] * w
    T = np.stack([x, c0, c1], axis=1).astype(np.float32)
    score, ok, m64 = evaluate(T)
    score = np.where(ok, score, -np.inf)
    for step in range(steps):
        which = rng.integers(0, 3, climbers)
        scale = 10.0 ** rng.uniform(-4, -1, (climbers, 1))
        move = rng.standard_normal((climbers, d)) * scale * (rng.random((climbers, d)) < 0.5)
        P = T.copy()
        rows = np.arange(climbers)
        P[rows, which] = (P[rows, which] * (1.0 + move)).astype(np.float32)
        s2, ok2, m2 = evaluate(P)
        take = ok2 & (s2 > score)
        T[take], score[take], m64[take] = P[take], s2[take], m2[take]
    i = int(np.argmax(score))
    return float(score[i]), tuple(T[i, j].copy() for j in range(3)), float(m64[i])
