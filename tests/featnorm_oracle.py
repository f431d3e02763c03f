"""float64 restatement of include/ssp.h's sliding-window normalisation, feature warping and frame selection (ssp_featnorm_sliding,
ssp_select_frames, ssp_featnorm_table), with the error bands the tests hold the device to (an ordinary module like
tests/snorm_oracle.py).  The toolkits' counterparts (Kaldi apply-cmvn-sliding, sidekit cep_sliding_norm / stg, feature warping) are
recalled, parity unpinned: this file is the yardstick.

Window of frame t of an utterance of T frames: lo = t - W // 2, hi = lo + W; lo < 0: hi -= lo, lo = 0; hi > T: lo -= hi - T, hi = T,
lo = max(lo, 0).  NaN entries are left out of the statistics and ranks and come out as NaN; n = non-NaN entries of the column in the
window.

Bands.  Modes 0 / 1, with u = 2^-24, a = mean |x| over the window's n entries, s = the oracle's deviation (1 in mode 0):
    |got - want| <= (n + 8) u (a / s + |want|)
— the a-priori bound of summing n float32 terms in any order, carried through the two-pass deviation (its second-order term fits in the
slack while a / s <= 100).  Mode 2: |got - want| <= 2^-23 |want|, and exactly 0 where k = n: neighbouring table entries are at least
1.2e-3 apart at window 1024, so a value inside the band proves that the count was exact.  Non-finite outputs must be of the oracle's
kind at the oracle's places and nowhere else.
"""
import numpy as np
from scipy.special import ndtri

U = 2.0 ** -24
STD_FLOOR = 10.0 * 2.0 ** -23


def window_bounds(T, W):
    """-> (lo, hi) int64[T]: the window [lo, hi) of every frame"""
    t = np.arange(T, dtype=np.int64)
    lo = t - W // 2
    hi = lo + W
    neg = lo < 0
    hi = np.where(neg, hi - lo, hi)
    lo = np.where(neg, 0, lo)
    over = hi > T
    lo = np.where(over, np.maximum(lo - (hi - T), 0), lo)
    hi = np.where(over, T, hi)
    return lo, hi


def sliding(x, W, mode):
    """one utterance x (T, D) float32 -> (want, band) float64 (T, D); band is inf where want is not finite"""
    x = np.asarray(x, dtype=np.float32)
    T, D = x.shape
    want = np.full((T, D), np.nan)
    band = np.full((T, D), np.inf)
    if T == 0:
        return want, band
    lo, hi = window_bounds(T, W)
    cnt = int(hi[0] - lo[0])
    assert ((hi - lo) == cnt).all() and cnt == min(W, T)
    idx = lo[:, None] + np.arange(cnt, dtype=np.int64)[None, :]
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        for d in range(D):
            col = xd[:, d]
            win = col[idx]                       # (T, cnt)
            ok = ~np.isnan(win)
            n = ok.sum(axis=1).astype(np.float64)
            if mode == 2:
                lt = (win < col[:, None]).sum(axis=1)
                eq = (win == col[:, None]).sum(axis=1)
                k = 2 * lt + eq
                w = np.where(np.isnan(col), np.nan, ndtri(k / np.maximum(2.0 * n, 1.0)))
                w = np.where(~np.isnan(col) & (k == n), 0.0, w)
                want[:, d] = w
                band[:, d] = np.where(np.isfinite(w), 2.0 ** -23 * np.abs(w), np.inf)
                continue
            z = np.where(ok, win, 0.0)
            mean = z.sum(axis=1) / n              # inf - inf, or no entry at all: NaN, as numpy has it
            dev = np.where(ok, win - mean[:, None], 0.0)
            sd = np.sqrt((dev * dev).sum(axis=1) / n)
            if mode == 0:
                s = np.ones(T)
            else:
                s = np.where(sd < STD_FLOOR, 1.0, sd)
            w = (col - mean) / s
            a = np.abs(z).sum(axis=1) / n
            want[:, d] = w
            band[:, d] = np.where(np.isfinite(w), (n + 8.0) * U * (a / s + np.abs(w)), np.inf)
    return want, band


def sliding_batch(x, offsets, W, mode):
    """the rows of x laid out by offsets (int64[n + 1], any start) -> (want, band) for rows offsets[0] .. offsets[-1]"""
    offsets = np.asarray(offsets, dtype=np.int64)
    parts = [sliding(x[offsets[u]:offsets[u + 1]], W, mode) for u in range(offsets.size - 1)]
    D = x.shape[1]
    want = np.concatenate([p[0] for p in parts] or [np.zeros((0, D))], axis=0)
    band = np.concatenate([p[1] for p in parts] or [np.zeros((0, D))], axis=0)
    return want, band


def sliding_brute(x, W, mode):
    """the definition frame by frame and column by column, with numpy's own nan-statistics (slow: the oracle's own check)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    T, D = x.shape
    out = np.full((T, D), np.nan)
    with np.errstate(all="ignore"):
        for t in range(T):
            lo = t - W // 2
            hi = lo + W
            if lo < 0:
                hi -= lo
                lo = 0
            if hi > T:
                lo -= hi - T
                hi = T
                lo = max(lo, 0)
            for d in range(D):
                w = x[lo:hi, d]
                w = w[~np.isnan(w)]
                v = x[t, d]
                if np.isnan(v):
                    continue
                if mode == 2:
                    k = 2 * int((w < v).sum()) + int((w == v).sum())
                    out[t, d] = 0.0 if k == w.size else ndtri(k / (2.0 * w.size))
                    continue
                m = w.sum() / w.size
                if mode == 0:
                    out[t, d] = v - m
                else:
                    sd = np.sqrt((np.abs(w - m) ** 2).sum() / w.size)
                    out[t, d] = (v - m) / (1.0 if sd < STD_FLOOR else sd)
    return out


def kind(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))


def check(got, want, band, what):
    """the device's rows against the oracle: the same kind of non-finite value at the same places, the finite ones inside the band.
    Prints the largest share of the band used; returns it."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    kg, kw = kind(got), kind(want)
    bad = np.argwhere(kg != kw)
    assert bad.size == 0, "%s: %d entries are not of the oracle's kind, the first at %s: %r against %r" % (
        what, bad.shape[0], tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    fin = kw == 0
    if not fin.any():
        print("[measured] %s: no finite entry" % what)
        return 0.0
    err = np.abs(got[fin] - want[fin])
    bnd = band[fin]
    share = float((err / np.where(bnd > 0, bnd, 1.0))[bnd > 0].max()) if (bnd > 0).any() else 0.0
    print("[measured] %s: max |err| %.3e, largest share of the band %.3f" % (what, float(err.max()), share))
    over = np.flatnonzero(err > bnd)
    assert over.size == 0, "%s: %d of %d finite entries leave the band, the worst by a factor %.3g (err %.3e, band %.3e)" % (
        what, over.size, err.size, float((err[over] / np.maximum(bnd[over], 1e-300)).max()), float(err[over].max()), float(bnd[over].min()))
    return share


def table(W):
    """float64 phi^-1(k / 2n), k = 1 .. 2n - 1, row n at offset (n - 1)^2, the centre exactly 0"""
    out = np.empty(W * W)
    for n in range(1, W + 1):
        k = np.arange(1, 2 * n, dtype=np.float64)
        row = ndtri(k / (2.0 * n))
        row[n - 1] = 0.0
        out[(n - 1) ** 2: n * n] = row
    return out


def select(x, offsets, mask):
    """-> (kept rows as uint32 bits, counts int64[n]): numpy boolean indexing on the rows of the segment table"""
    offsets = np.asarray(offsets, dtype=np.int64)
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    m = np.asarray(mask).reshape(-1) != 0
    a, b = int(offsets[0]), int(offsets[-1])
    kept = bits[a:b][m[a:b]]
    counts = np.array([int(m[offsets[u]:offsets[u + 1]].sum()) for u in range(offsets.size - 1)], dtype=np.int64)
    return kept, counts


def frames_in_segments(segments, n_frames, win=400, hop=160):
    out = np.zeros(n_frames, dtype=np.uint8)
    for t in range(n_frames):
        c = t * hop + win // 2
        out[t] = 1 if any(a <= c < b for a, b in segments) else 0
    return out
