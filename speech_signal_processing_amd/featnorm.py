"""Sliding-window normalisation, feature warping and speech-frame selection of feature matrices on the GPU: the step between the feature
extractors and the models that the long-recording back ends (diarize.Diarizer, ivector.TotalVariability, plda.Plda) are fed through.

* ``cmvn_sliding``        mean (and variance) normalisation over a window centred on each frame — Kaldi's apply-cmvn-sliding
                          (center=true), sidekit's cep_sliding_norm
* ``feature_warp``        rank warping to a standard normal over the same window — Pelecanos and Sridharan, sidekit's stg
* ``select_frames``       the rows a mask keeps, packed — Kaldi's select-voiced-frames
* ``frames_in_segments``  host helper: VAD.speech_segments' sample ranges as a mask over feature frames

The toolkits' counterparts are recalled, parity unpinned: none of them is at hand and the reference has no such step (it scales once
per utterance, GMM_UBM.py:93).  include/ssp.h (ssp_featnorm_sliding, ssp_select_frames) has the definitions, tests/featnorm_oracle.py
restates them in float64.  Every function takes one (T, D) array or a list of them; a list goes to the device as one ragged batch and
runs in one launch.  Arrays come back in the input's float dtype (float64 for anything that is not a float array).
"""
from __future__ import annotations

import numpy as np

from . import api


def _batch(feats):
    """-> (is_single, list of 2-D arrays, result dtype)"""
    single = not isinstance(feats, (list, tuple))
    arrs = [np.asarray(f) for f in ([feats] if single else feats)]
    for f in arrs:
        if f.ndim != 2:
            raise ValueError("every feature array must be (frames, dim)")
    if arrs and len({f.shape[1] for f in arrs}) != 1:
        raise ValueError("the arrays of one batch must have the same number of columns")
    dt = arrs[0].dtype if arrs and arrs[0].dtype.kind == "f" else np.dtype(np.float64)
    return single, arrs, dt


def _flat(arrs):
    if len(arrs) == 1:
        return np.ascontiguousarray(arrs[0], dtype=np.float32)
    return np.concatenate([np.asarray(f, dtype=np.float32) for f in arrs], axis=0)


def _sliding(feats, window, mode):
    single, arrs, dt = _batch(feats)
    ctx = api.default_context()
    if not arrs:
        return []
    seg = api.Segments.from_lengths(ctx, [f.shape[0] for f in arrs])
    out = api.featnorm_sliding(ctx, _flat(arrs), seg, window=int(window), mode=mode).astype(dt, copy=False)
    o = seg.offsets
    res = [out[o[i]:o[i + 1]] for i in range(len(arrs))]
    return res[0] if single else res


def cmvn_sliding(feats, window=300, norm_vars=True):
    """Every column minus its mean over the ``window`` frames centred on the frame (slid back inside the utterance at its ends) and,
    ``norm_vars``, divided by its deviation over them (a deviation below 10 * 2^-23 counts as 1).  NaN entries are left out and stay NaN."""
    return _sliding(feats, window, 1 if norm_vars else 0)


def feature_warp(feats, window=300):
    """Every entry replaced by the standard normal quantile of its mid-rank among the ``window`` frames around it:
    phi^-1((2 #{smaller} + #{equal}) / 2n).  NaN entries are left out and stay NaN."""
    return _sliding(feats, window, 2)


def select_frames(feats, masks):
    """The rows of each (T, D) array whose mask entry is non-zero (one array and one mask, or two lists of equal length)."""
    single, arrs, dt = _batch(feats)
    ms = [np.asarray(m).reshape(-1) for m in ([masks] if single else masks)]
    if len(ms) != len(arrs) or any(m.shape[0] != f.shape[0] for m, f in zip(ms, arrs)):
        raise ValueError("one mask entry per feature row")
    ctx = api.default_context()
    if not arrs:
        return []
    seg = api.Segments.from_lengths(ctx, [f.shape[0] for f in arrs])
    mask = np.concatenate([m != 0 for m in ms]).astype(np.uint8)
    kept, kseg, _ = api.select_frames(ctx, _flat(arrs), seg, mask)
    kept = kept.astype(dt, copy=False)
    o = kseg.offsets
    res = [kept[o[i]:o[i + 1]] for i in range(len(arrs))]
    return res[0] if single else res


def frames_in_segments(segments, n_frames, win=400, hop=160):
    """uint8 mask over ``n_frames`` feature frames (window ``win``, step ``hop`` samples): frame t is kept when its centre sample
    ``t * hop + win // 2`` lies in one of the ``(start, end)`` sample ranges (end exclusive) that VAD.speech_segments returns.  Host only."""
    centre = np.arange(int(n_frames), dtype=np.int64) * int(hop) + int(win) // 2
    mask = np.zeros(int(n_frames), dtype=np.uint8)
    for a, b in segments:
        mask[(centre >= int(a)) & (centre < int(b))] = 1
    return mask
