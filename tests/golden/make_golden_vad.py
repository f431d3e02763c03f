#!/usr/bin/env python
"""Generate tests/golden/vad.npz from the REFERENCE's VAD.py (run in the build container only, like make_golden.py).

Imports the reference with empty stubs for the packages its plotting / tuning code wants (seaborn, bayes_opt, pyaudio, simpleaudio)
and calls its own enframe / feature / VAD_detection / VAD_frequency on seeded int16 signals.  Stored per case c: the int16 input
``x_c``, the shape of enframe's output ``shape_c``, ``zcr_c`` / ``power_c`` / ``entropy_c`` (float64 (n, 1)), ``det0_c`` / ``det1_c``
(VAD_detection with the default and with an off-default threshold set, ``thresholds``) and ``freq_c`` (VAD_frequency).  Arrays only.

The generator ASSERTS what makes an exact comparison of decisions fair and fails rather than write a fixture that violates it:
(a) no frame's power within a relative 1e-4 of 0.1 or of a threshold set's ampl / amph, no entropy within 1e-4 of 0.4;
(b) the last frame of every case is quiet under both threshold sets (there the reference's wrap-around to index -1 equals a stop at 0);
(c) no sample equals -32768 (numpy's int16 abs wraps there).

    python tests/golden/make_golden_vad.py
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, _stub  # noqa: E402
import vad_oracle as VO  # noqa: E402  (signal recipe only: every stored result comes from the reference)

THRESHOLDS = np.array([[35.0, 0.3, 12.0], [27.3, 1.7, 8.4]])   # zcr_gate, ampl, amph; the second set lies inside optimize's ranges
BAND = 1e-4


def import_vad():
    if not hasattr(np, "int"):
        np.int = int
    _stub("pyaudio", PyAudio=object, paInt16=8)
    _stub("simpleaudio")
    _stub("seaborn")
    _stub("bayes_opt", BayesianOptimization=None)
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    import VAD  # noqa
    return VAD


def noise(rng, n):
    return 131.0 * rng.standard_normal(n)   # about 0.4 % of full scale


def to_i16(x):
    return np.clip(np.round(x), -32767, 32767).astype(np.int16)


def cases():
    out = {}
    # a: 3 s at 16 kHz, three bursts
    rng = np.random.default_rng(101)
    x = noise(rng, 48000)
    for at, m in ((5000, 7000), (20000, 9000), (36000, 6000)):
        x[at:at + m] += VO.burst(rng, m)
    out["a"] = to_i16(x)
    # b: a length that is no multiple of 128, speech from sample 0
    rng = np.random.default_rng(102)
    x = noise(rng, 30077)
    x[0:8000] += VO.burst(rng, 8000)
    x[15000:21000] += VO.burst(rng, 6000)
    out["b"] = to_i16(x)
    # c: a 50 ms burst, then a 400 ms one: the short run is not reset and the long one extends it across the gap
    rng = np.random.default_rng(103)
    x = noise(rng, 48000)
    x[10000:10800] += VO.burst(rng, 800, amp=26000)
    x[13000:19400] += VO.burst(rng, 6400, amp=24000)
    out["c"] = to_i16(x)
    # d: 300 samples (3 frames), a click at the start
    rng = np.random.default_rng(104)
    x = noise(rng, 300)
    x[0:60] += VO.burst(rng, 60, f0=700, amp=26000)
    out["d"] = to_i16(x)
    # e: several close bursts
    rng = np.random.default_rng(105)
    x = noise(rng, 48000)
    for k in range(6):
        at = 4000 + k * 5600
        x[at:at + 4200] += VO.burst(rng, 4200)
    out["e"] = to_i16(x)
    # f: an exact multiple of 128
    rng = np.random.default_rng(106)
    x = noise(rng, 128 * 200)
    x[3000:12000] += VO.burst(rng, 9000)
    out["f"] = to_i16(x)
    # g: digital silence: 0 / 0, NaN power and entropy
    out["g"] = np.zeros(1000, dtype=np.int16)
    return out


def main():
    VAD = import_vad()
    store = {"thresholds": THRESHOLDS, "cases": np.array(sorted(cases()))}
    worst_p, worst_e = np.inf, np.inf
    for name, x in cases().items():
        assert x.dtype == np.int16 and not (x == -32768).any(), name                       # (c)
        with warnings.catch_warnings(), np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("ignore")
            frames = VAD.enframe(x / (max(abs(x))))                                           # wavdata's normalisation, VAD.py:131-132
            zcr, power, ent = VAD.feature(frames)
            det = [VAD.VAD_detection(zcr, power, zcr_gate=g, ampl=lo, amph=hi) for g, lo, hi in THRESHOLDS]
            freq = VAD.VAD_frequency(ent)
        finite = np.isfinite(power[:, 0])
        for g, lo, hi in THRESHOLDS:
            for thr in (0.1, lo, hi):                                                       # (a)
                d = np.abs(power[finite, 0] - thr) / thr
                worst_p = min(worst_p, d.min()) if d.size else worst_p
                assert not (d <= BAND).any(), (name, thr, d.min())
            if finite.any():                                                                # (b)
                assert not (power[-1, 0] > lo or zcr[-1, 0] > g), (name, "last frame is not quiet")
        d = np.abs(ent[finite, 0] - 0.4) / 0.4
        worst_e = min(worst_e, d.min()) if d.size else worst_e
        assert not (d <= BAND).any(), (name, "entropy", d.min())
        store["x_" + name] = x
        store["shape_" + name] = np.array(frames.shape)
        store["zcr_" + name], store["power_" + name], store["entropy_" + name] = zcr, power, ent
        store["det0_" + name], store["det1_" + name], store["freq_" + name] = det[0], det[1], freq
        print("%s: %6d samples %4d frames, speech frames %3d / %3d (frequency %3d), power %.4g .. %.4g" % (
            name, x.shape[0], frames.shape[1], int(det[0].sum()), int(det[1].sum()), int(freq.sum()),
            np.nanmin(power) if finite.any() else np.nan, np.nanmax(power) if finite.any() else np.nan))
    print("smallest relative distance to a threshold: power %.3g, entropy %.3g" % (worst_p, worst_e))
    np.savez_compressed(os.path.join(HERE, "vad.npz"), **store)
    print("wrote", os.path.join(HERE, "vad.npz"), os.path.getsize(os.path.join(HERE, "vad.npz")), "bytes")


if __name__ == "__main__":
    main()
