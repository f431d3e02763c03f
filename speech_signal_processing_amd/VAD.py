"""GPU-backed mirror of the reference's ``VAD.py``: framing without a window (VAD.py:28-50), zero-crossing rate (:53-64), frame energy
(:67-76), spectral entropy (:79-105), ``feature`` (:108-119), the two-threshold detector ``VAD_detection`` (:136-182) and the entropy
detector ``VAD_frequency`` (:185-186) — same names, same shapes, float64 out.  The per-frame Python loops of the reference run as one
feature kernel (ssp_vad_features) and one detector kernel (ssp_vad_detect); the calls that take the framed ``(256, n_frames)`` matrix
hand its columns over as one utterance with step 256.  ``enframe`` and ``wavdata`` only read and copy samples and stay on the host.

The batched surface — ``feature_batch``, ``detect_batch``, ``speech_segments``, ``remove_silence`` — takes a list of raw signals (int16
PCM as ``utils.tools.read`` returns it, or float arrays) and runs one launch per batch.

Two deliberate differences from the reference: ``feature`` does not print, and ``VAD_detection``'s backward walk stops at frame 0
where Python's index -1 would go on with the last frame (the same result whenever the last frame is quiet).

The threshold search — ``label`` (VAD.py:223-228), ``optimize`` (:189-220) and, beyond the reference, ``label_frames``, ``f1_counts``,
``sweep`` and ``optimize_batch`` — evaluates the reference's OBJECTIVE, ``cv(zcr_gate, ampl, amph)`` = F1 of ``VAD_detection`` against
the frame labels, for thousands of threshold triples in one launch (ssp_vad_sweep: every triple runs the detector's own state machine,
only the integer counts tp / fp / fn leave the device).  At any given triple that objective is the reference's, and that is what the
tests pin.  The SEARCH STRATEGY IS NOT the reference's: the reference asks ``bayes_opt`` for 35 sequential evaluations of a
Gaussian-process surrogate search; here a dense grid over the same box (16 x 16 x 16 by default) is evaluated at once and re-gridded
around its winner.  The triple returned is therefore not the one the reference would return (its search is randomised anyway); its F1 is
that of the best grid point.  Only the plots and ``main`` are not mirrored.  There is no CPU fallback: without a device the computing
calls raise ``SspError``."""
from __future__ import annotations

import math

import numpy as np

from . import api
from .utils.tools import wave_read

frameSize = 256
overlap = 128
_MIN_LEN = 16   # VAD.py:138


def enframe(wavData):
    """VAD.py:28-50 — ``(frameSize, ceil(n / step))`` float64, one frame per column, zero padded behind the end; no window."""
    wavData = np.asarray(wavData).reshape(-1)
    wlen = wavData.shape[0]
    step = frameSize - overlap
    frameNum = math.ceil(wlen / step)
    frameData = np.zeros((frameSize, frameNum))
    idx = np.arange(frameSize)[:, None] + step * np.arange(frameNum)[None, :]
    inside = idx < wlen
    frameData[inside] = wavData[idx[inside]]
    return frameData


def wavdata(wavfile):
    """VAD.py:123-132 — the file's int16 samples divided by their peak (taken on widened values: |-32768| = 32768), framed."""
    f = wave_read(wavfile)
    nframes = f.getparams()[3]
    waveData = np.frombuffer(f.readframes(nframes), dtype=np.int16).astype(np.float64)
    f.close()
    waveData = waveData / np.max(np.abs(waveData))
    return enframe(waveData)


def _frame_features(frameData, gate=True):
    """the three planes of the columns of a (256, n) frame matrix, float64 (n, 1) each"""
    frameData = np.asarray(frameData)
    if frameData.ndim != 2:
        raise ValueError("frameData must be (frameSize, frameNum)")
    ctx = api.default_context()
    n = frameData.shape[1]
    flat = np.ascontiguousarray(frameData.T, dtype=np.float32).reshape(-1)
    seg = api.Segments.from_lengths(ctx, [flat.shape[0]])
    zcr, power, ent, _ = api.vad_features(ctx, flat, seg, frame_size=frameData.shape[0], step=frameData.shape[0], normalize=False, gate_zcr=gate)
    return tuple(np.asarray(v, dtype=np.float64).reshape(n, 1) for v in (zcr, power, ent))


def ZCR(frameData):
    """VAD.py:53-64 — sign changes between neighbouring samples of every frame (a zero sample makes none)."""
    return _frame_features(frameData, gate=False)[0]


def energy(frameData):
    """VAD.py:67-76 — sum of squares per frame."""
    return _frame_features(frameData)[1]


def spectrum_entropy(frameData):
    """VAD.py:79-105 — entropy of the energy shares of 10 blocks of 12 bins among bins 0..127 of the frame's 256-point spectrum."""
    return _frame_features(frameData)[2]


def feature(waveData):
    """VAD.py:108-119 — ``(zcr * (power > 0.1), power, spectral entropy)`` of a framed signal, one kernel launch (and no print)."""
    return _frame_features(waveData)


def VAD_detection(zcr, power, zcr_gate=35, ampl=0.3, amph=12):
    """VAD.py:136-182 — the two-threshold state machine; ``(n_frames, 1)`` float64 of 0 / 1."""
    ctx = api.default_context()
    z = np.ascontiguousarray(np.asarray(zcr, dtype=np.float32).reshape(-1))
    p = np.ascontiguousarray(np.asarray(power, dtype=np.float32).reshape(-1))
    if z.shape != p.shape:
        raise ValueError("zcr and power must have one value per frame each")
    seg = api.Segments.from_lengths(ctx, [z.shape[0]])
    mask, _ = api.vad_detect(ctx, z, p, seg, 0, zcr_gate, ampl, amph, _MIN_LEN)
    return np.asarray(mask, dtype=np.float64).reshape(-1, 1)


def VAD_frequency(spectrum):
    """VAD.py:185-186 — ``np.where(spectrum > 0.4, 0, 1)``."""
    ctx = api.default_context()
    s = np.asarray(spectrum)
    e = np.ascontiguousarray(s.astype(np.float32).reshape(-1))
    seg = api.Segments.from_lengths(ctx, [e.shape[0]])
    mask, _ = api.vad_detect(ctx, None, e, seg, 1, ampl=0.4)
    return np.asarray(mask, dtype=np.int64).reshape(s.shape)


# ---- batched surface -------------------------------------------------------------------------------------------------------------
def feature_batch(signals, normalize=True):
    """``feature(enframe(x / max|x|))`` for every signal of a list (int16 PCM or float arrays) in one launch: a list of
    ``(zcr, power, entropy)``, float64 ``(n_frames, 1)`` each.  ``normalize=False`` takes the samples as they are."""
    ctx = api.default_context()
    flat, lens = api.flatten_signals(signals)
    seg = api.Segments.from_lengths(ctx, lens)
    zcr, power, ent, fseg = api.vad_features(ctx, flat, seg, normalize=normalize)
    o = fseg.offsets
    return [tuple(np.asarray(v[o[i]:o[i + 1]], dtype=np.float64).reshape(-1, 1) for v in (zcr, power, ent)) for i in range(len(lens))]


def detect_batch(signals, zcr_gate=35, ampl=0.3, amph=12, method='time', normalize=True):
    """Per-frame speech masks (uint8, 1 = speech) of a list of signals: ``method='time'`` is ``VAD_detection`` on each signal's features,
    ``'frequency'`` is ``VAD_frequency``.  The samples go to the device once; the features stay there between the two kernels."""
    if method not in ('time', 'frequency'):
        raise ValueError("method must be 'time' or 'frequency'")
    import torch
    ctx = api.default_context()
    flat, lens = api.flatten_signals(signals)
    seg = api.Segments.from_lengths(ctx, lens)
    dev = torch.from_numpy(flat).to("cuda:%d" % ctx.device)
    zcr, power, ent, fseg = api.vad_features(ctx, dev, seg, normalize=normalize)
    if method == 'time':
        mask, _ = api.vad_detect(ctx, zcr, power, fseg, 0, zcr_gate, ampl, amph, _MIN_LEN)
    else:
        mask, _ = api.vad_detect(ctx, None, ent, fseg, 1, ampl=0.4)
    mask = mask.cpu().numpy()
    o = fseg.offsets
    return [mask[o[i]:o[i + 1]] for i in range(len(lens))]


def speech_segments(mask, n_samples):
    """``(start_sample, end_sample)`` ranges (end exclusive) of the samples that a frame marked 1 covers — frame t covers
    ``[t * step, t * step + frameSize)`` — clipped to the utterance; ranges that touch or overlap are one range."""
    m = np.asarray(mask).reshape(-1) != 0
    step = frameSize - overlap
    out = []
    for t in np.flatnonzero(m):
        a, b = int(t) * step, min(int(t) * step + frameSize, int(n_samples))
        if a >= b:
            continue
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def remove_silence(signals, **thresholds):
    """Every signal of a list with only the samples of its ``speech_segments`` (mask on the device, slicing in numpy).  ``thresholds``:
    ``detect_batch``'s keyword arguments."""
    sig = [np.asarray(s).reshape(-1) for s in signals]
    masks = detect_batch(sig, **thresholds)
    out = []
    for x, m in zip(sig, masks):
        parts = [x[a:b] for a, b in speech_segments(m, x.shape[0])]
        out.append(np.concatenate(parts) if parts else x[:0])
    return out


# ---- threshold search ------------------------------------------------------------------------------------------------------------
BOUNDS = {'zcr_gate': (20, 40), 'ampl': (0.3, 4), 'amph': (5, 15)}   # VAD.py:197-201
_AXES = ('zcr_gate', 'ampl', 'amph')


def label_frames(sample_labels):
    """Frame labels from per-sample labels (VAD.py:226-228): 1 where a frame covers a sample labelled > 0 in sum, else 0; int ``(n_frames,)``."""
    return np.where(enframe(sample_labels).sum(axis=0) > 0, 1, 0)


def label(mat_file):
    """VAD.py:223-228 — the ``y_label`` array of a .mat file through ``label_frames`` (host only, as ``enframe``)."""
    from scipy.io import loadmat
    return label_frames(loadmat(mat_file)['y_label'])


def f1_counts(tp, fp, fn):
    """``2 tp / (2 tp + fp + fn)`` in float64, 0.0 where the denominator is 0 — what ``sklearn.metrics.f1_score`` returns (VAD.py:210)."""
    tp, fp, fn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn))
    den = 2.0 * tp + fp + fn
    out = np.zeros(den.shape, dtype=np.float64)
    np.divide(2.0 * tp, den, out=out, where=den > 0)
    return out if out.ndim else float(out)


def sweep(zcr, power, y, zcr_gate, ampl, amph):
    """The reference's objective ``cv`` (VAD.py:204-210) of one utterance at every threshold triple (scalars or arrays that broadcast
    against each other) in one launch: ``(f1 float64 (n_par,), counts int32 (n_par, 3) = tp, fp, fn)``.  ``zcr`` / ``power``: the
    ``(n, 1)`` planes of ``feature``; ``y``: the frame labels."""
    ctx = api.default_context()
    z = np.ascontiguousarray(np.asarray(zcr, dtype=np.float32).reshape(-1))
    p = np.ascontiguousarray(np.asarray(power, dtype=np.float32).reshape(-1))
    lab = np.asarray(y).reshape(-1)
    if not (z.shape == p.shape == lab.shape):
        raise ValueError("zcr, power and y must hold one value per frame each")
    seg = api.Segments.from_lengths(ctx, [z.shape[0]])
    counts = np.asarray(api.vad_sweep(ctx, z, p, lab, seg, zcr_gate, ampl, amph, 0, _MIN_LEN))[:, 0, :]
    return f1_counts(counts[:, 0], counts[:, 1], counts[:, 2]), counts


def _axis(lo, hi, n):
    """n float32 grid values from lo to hi, both included (n = 1: the middle), as float64"""
    v = np.linspace(lo, hi, n) if n > 1 else np.array([(lo + hi) / 2.0])
    return v.astype(np.float32).astype(np.float64)


def _grid_search(count_fn, grid, refine, bounds):
    """Dense grid search of the pooled F1.  count_fn(zcr_gate, ampl, amph) takes three float32 arrays of n_par values and returns the
    counts ``(n_par, n_utt, 3)``; one call per round.  Round 0 grids ``bounds``; each of the ``refine`` rounds grids the box spanned by
    the grid neighbours of the winner so far (the box's own edge where the winner sits on it).  The best F1 wins, ties go to the lowest
    flat index in (zcr_gate, ampl, amph) C order and to the earlier round.  -> the dict that ``optimize.last`` holds."""
    grid = tuple(int(n) for n in grid)
    if len(grid) != 3 or min(grid) < 1 or refine < 0:
        raise ValueError("grid must be three positive counts (zcr_gate, ampl, amph) and refine >= 0")
    box = dict(BOUNDS)
    box.update(bounds or {})
    for k in _AXES:
        if not float(box[k][0]) <= float(box[k][1]):
            raise ValueError("bounds[%r] must be (low, high)" % k)
    best, evaluations = None, 0
    for _ in range(1 + int(refine)):
        axes = [_axis(float(box[k][0]), float(box[k][1]), n) for k, n in zip(_AXES, grid)]
        mesh = [m.reshape(-1) for m in np.meshgrid(*axes, indexing='ij')]
        counts = np.asarray(count_fn(*(m.astype(np.float32) for m in mesh)), dtype=np.int64)
        if counts.shape[0] != mesh[0].shape[0] or counts.shape[-1] != 3:
            raise ValueError("the count function returned %r for %d triples" % (counts.shape, mesh[0].shape[0]))
        pooled = counts.reshape(counts.shape[0], -1, 3).sum(axis=1)
        f1 = f1_counts(pooled[:, 0], pooled[:, 1], pooled[:, 2])
        evaluations += f1.shape[0]
        flat = int(np.argmax(f1))   # (the first of equal maxima)
        idx = np.unravel_index(flat, grid)
        if best is None or f1[flat] > best['target']:
            best = {'target': float(f1[flat]), 'params': {k: float(a[i]) for k, a, i in zip(_AXES, axes, idx)}, 'counts': pooled[flat].copy()}
            box = {k: (float(a[max(i - 1, 0)]), float(a[min(i + 1, len(a) - 1)])) for k, a, i in zip(_AXES, axes, idx)}
        else:   # nothing better inside the box: halve it around the winner so far
            box = {k: ((box[k][0] + best['params'][k]) / 2.0, (box[k][1] + best['params'][k]) / 2.0) for k in _AXES}
    best['evaluations'] = evaluations
    return best


def optimize(X, y, grid=(16, 16, 16), refine=2, bounds=None):
    """VAD.py:189-220 — thresholds ``{'zcr_gate', 'ampl', 'amph'}`` that maximise the F1 of ``VAD_detection`` on the framed signal ``X``
    (``(256, n)``) against the frame labels ``y``, like ``BO.max['params']``.  The objective is the reference's; the search is a dense
    grid over the reference's box (``bounds`` overrides it per key) evaluated in ONE ssp_vad_sweep call, then ``refine`` rounds that
    re-grid the box between the winner's grid neighbours, one call each — not the reference's 35-point Gaussian-process search.  Ties go
    to the lowest flat index in (zcr_gate, ampl, amph) order.  Prints nothing; ``optimize.last`` keeps ``{'target', 'params',
    'evaluations', 'counts'}`` of the call."""
    zcr, power, _ = feature(X)
    lab = np.asarray(y).reshape(-1)
    if lab.shape[0] != zcr.shape[0]:
        raise ValueError("y must hold one label per frame of X")
    ctx = api.default_context()
    z = np.ascontiguousarray(zcr.reshape(-1), dtype=np.float32)
    p = np.ascontiguousarray(power.reshape(-1), dtype=np.float32)
    seg = api.Segments.from_lengths(ctx, [z.shape[0]])
    optimize.last = _grid_search(lambda g, lo, hi: api.vad_sweep(ctx, z, p, lab, seg, g, lo, hi, 0, _MIN_LEN), grid, refine, bounds)
    return dict(optimize.last['params'])


optimize.last = None


def optimize_batch(signals, sample_labels, grid=(16, 16, 16), refine=2, bounds=None, normalize=True):
    """``optimize`` for a labelled corpus: ``signals`` a list of raw signals (int16 PCM or float arrays), ``sample_labels`` their
    per-sample labels.  The features of all signals come from one device pass and stay there; the counts are summed over the
    utterances before F1 is taken (the pooled F1).  ``optimize_batch.last`` as ``optimize.last``."""
    import torch
    if len(signals) != len(sample_labels):
        raise ValueError("one label array per signal")
    ctx = api.default_context()
    flat, lens = api.flatten_signals(signals)
    labs = [label_frames(np.asarray(v).reshape(-1)).astype(np.uint8) for v in sample_labels]
    for n, v in zip(lens, sample_labels):
        if np.asarray(v).reshape(-1).shape[0] != n:
            raise ValueError("a label array differs in length from its signal")
    seg = api.Segments.from_lengths(ctx, lens)
    dev = "cuda:%d" % ctx.device
    zcr, power, _, fseg = api.vad_features(ctx, torch.from_numpy(flat).to(dev), seg, normalize=normalize)
    lab = torch.from_numpy(np.concatenate(labs) if labs else np.zeros(0, np.uint8)).to(dev)
    optimize_batch.last = _grid_search(lambda g, lo, hi: api.vad_sweep(ctx, zcr, power, lab, fseg, g, lo, hi, 0, _MIN_LEN).cpu().numpy(),
                                       grid, refine, bounds)
    return dict(optimize_batch.last['params'])


optimize_batch.last = None
