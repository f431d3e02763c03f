"""GPU-backed mirror of the reference's ``VAD.py``: framing without a window (VAD.py:28-50), zero-crossing rate (:53-64), frame energy
(:67-76), spectral entropy (:79-105), ``feature`` (:108-119), the two-threshold detector ``VAD_detection`` (:136-182) and the entropy
detector ``VAD_frequency`` (:185-186) — same names, same shapes, float64 out.  The per-frame Python loops of the reference run as one
feature kernel (ssp_vad_features) and one detector kernel (ssp_vad_detect); the calls that take the framed ``(256, n_frames)`` matrix
hand its columns over as one utterance with step 256.  ``enframe`` and ``wavdata`` only read and copy samples and stay on the host.

The batched surface — ``feature_batch``, ``detect_batch``, ``speech_segments``, ``remove_silence`` — takes a list of raw signals (int16
PCM as ``utils.tools.read`` returns it, or float arrays) and runs one launch per batch.

Two deliberate differences from the reference: ``feature`` does not print, and ``VAD_detection``'s backward walk stops at frame 0
where Python's index -1 would go on with the last frame (the same result whenever the last frame is quiet).  ``optimize``, ``label``,
the plots and ``main`` are not mirrored.  There is no CPU fallback: without a device the computing calls raise ``SspError``."""
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
