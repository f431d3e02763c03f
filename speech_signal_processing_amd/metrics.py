"""Verification metrics from a score matrix: miss / false-alarm counts over a threshold grid on the device (api.det_counts,
ssp_det_counts), then the DET curve, the equal error rate and the minimum detection cost on the host in float64.  An extension and
UNPINNED: the reference has no error-rate code; tests/snorm_oracle.py restates these by brute force.

A trial (t, s) is a target trial when row t belongs to enrolled speaker s.  At threshold theta_j a trial is accepted when its score is
>= theta_j:  p_miss_j = #{target scores < theta_j} / n_tar,   p_fa_j = #{non-target scores >= theta_j} / n_non.  NaN scores are counted
apart and excluded from both totals.

    from speech_signal_processing_amd import metrics
    counts = metrics.det_counts(scores, target)          # scores (N, S), target (N,) in [0, S) or -1
    rate, threshold = metrics.eer(counts)
    cost = metrics.min_dcf(counts, p_target=0.01)

diarization_error(ref, hyp) is the frame-level diarization error of two label sequences (host only; diarize.py produces such labels).
"""
from __future__ import annotations

import numpy as np

from . import api


def det_counts(scores, target, thresholds=None, n_thresholds=1024, ctx=None) -> dict:
    """api.det_counts with a default grid: with no thresholds a first call without any gives the range of the scores, and the grid is
    numpy.linspace(lo, hi, n_thresholds) rounded to float32.  -> {"tar_hist", "non_hist" (M + 1,), "nan_count" (2,), "range" (4,),
    "thresholds" (M,)} on the host."""
    ctx = ctx or api.default_context()
    if thresholds is None:
        if int(n_thresholds) != n_thresholds or not 1 <= n_thresholds <= api.DET_MAX_THRESHOLDS:
            raise ValueError("n_thresholds must be an integer in [1, %d]" % api.DET_MAX_THRESHOLDS)
        r = api.det_counts(ctx, scores, target)["range"].astype(np.float64)
        lo, hi = min(r[0], r[2]), max(r[1], r[3])
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("no finite score range to place a grid on (no score that is not NaN, or infinite scores): pass thresholds")
        thresholds = np.linspace(lo, hi, int(n_thresholds)).astype(np.float32)
    return api.det_counts(ctx, scores, target, thresholds)


def error_rates(counts):
    """-> (thresholds (M,), p_miss (M,), p_fa (M,)) in float64: p_miss_j = sum_{b <= j} tar_hist[b] / n_tar,
    p_fa_j = sum_{b > j} non_hist[b] / n_non (NaN trials are in neither total; counts["nan_count"] reports them).  A side without trials
    gives NaN rates."""
    tar = np.asarray(counts["tar_hist"], dtype=np.int64)
    non = np.asarray(counts["non_hist"], dtype=np.int64)
    n_tar, n_non = int(tar.sum()), int(non.sum())
    miss = np.cumsum(tar)[:-1].astype(np.float64)
    fa = (n_non - np.cumsum(non)[:-1]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(counts["thresholds"], dtype=np.float64), miss / np.float64(n_tar), fa / np.float64(n_non)


def eer(counts):
    """-> (equal error rate, threshold): at the first grid point j where p_miss - p_fa becomes >= 0, interpolated linearly between j - 1
    and j (j = 0: that point itself).  NaN when the difference never gets there (a grid that ends below the crossing, a side without
    trials)."""
    th, miss, fa = error_rates(counts)
    d = miss - fa
    hit = np.flatnonzero(d >= 0)
    if hit.size == 0:
        return float("nan"), float("nan")
    j = int(hit[0])
    if j == 0:
        return float(0.5 * (miss[0] + fa[0])), float(th[0])
    w = -d[j - 1] / (d[j] - d[j - 1])   # d[j - 1] < 0 <= d[j]
    return float(miss[j - 1] + w * (miss[j] - miss[j - 1])), float(th[j - 1] + w * (th[j] - th[j - 1]))


def min_dcf(counts, p_target=0.01, c_miss=1.0, c_fa=1.0):
    """the minimum over the grid of c_miss p_target p_miss + c_fa (1 - p_target) p_fa, divided by min(c_miss p_target,
    c_fa (1 - p_target)) (the cost of the better of the two trivial systems)"""
    if not 0.0 < p_target < 1.0 or c_miss <= 0 or c_fa <= 0:
        raise ValueError("p_target must lie in (0, 1) and the costs must be positive")
    _, miss, fa = error_rates(counts)
    if miss.size == 0:
        return float("nan")
    cost = c_miss * p_target * miss + c_fa * (1.0 - p_target) * fa
    return float(np.min(cost) / min(c_miss * p_target, c_fa * (1.0 - p_target)))


def diarization_error(ref, hyp) -> dict:
    """Frame-level diarization error, no collar, on the host: ref and hyp are integer label arrays of one entry per frame, -1 for
    silence.  The hypothesis speakers are mapped one-to-one onto the reference speakers so that the frames on which both agree are as
    many as possible (scipy.optimize.linear_sum_assignment).  -> {"miss", "false_alarm", "confusion", "der"}: reference speech
    frames the hypothesis calls silence, hypothesis speech frames the reference calls silence, frames both call speech but of
    different (mapped) speakers, and their sum, each divided by the number of reference speech frames (NaN when there is none)."""
    ref = np.asarray(ref).reshape(-1).astype(np.int64)
    hyp = np.asarray(hyp).reshape(-1).astype(np.int64)
    if ref.shape != hyp.shape:
        raise ValueError("ref and hyp must have one label per frame each")
    if (ref < -1).any() or (hyp < -1).any():
        raise ValueError("labels must be >= 0, or -1 for silence")
    rs, hs = ref >= 0, hyp >= 0
    miss, fa, both = int((rs & ~hs).sum()), int((~rs & hs).sum()), rs & hs
    matched = 0
    if both.any():
        from scipy.optimize import linear_sum_assignment   # (host-only helper: imported where it is needed, as VAD.py does)
        ru, ri = np.unique(ref[both], return_inverse=True)
        hu, hi = np.unique(hyp[both], return_inverse=True)
        agree = np.zeros((ru.size, hu.size), dtype=np.int64)
        np.add.at(agree, (ri, hi), 1)
        rows, cols = linear_sum_assignment(agree, maximize=True)
        matched = int(agree[rows, cols].sum())
    conf = int(both.sum()) - matched
    n_ref = int(rs.sum())
    den = np.float64(n_ref) if n_ref else np.float64("nan")
    return {"miss": float(miss / den), "false_alarm": float(fa / den), "confusion": float(conf / den), "der": float((miss + fa + conf) / den)}
