#!/usr/bin/env python
"""Generate tests/golden/vad_sweep.npz from the REFERENCE's VAD.py (run in the build container only, like make_golden_vad.py): the
objective of its threshold search — F1 of VAD_detection against frame labels — on a grid of threshold triples, as integer counts.

Imports the reference with make_golden_vad.py's stubs and calls its own enframe / feature / VAD_detection / label, and
sklearn.metrics.f1_score as its ``cv`` does (VAD.py:204-210).  Stored per case c: the int16 signal ``x_c``, the per-sample labels ``y_c``,
the frame labels ``ylab_c`` (the reference's ``label()`` on a temporary .mat written with scipy.io.savemat), ``zcr_c`` / ``power_c`` /
``entropy_c`` (float64 (n, 1)), ``counts_c`` int32 (125, 3) = (tp, fp, fn) of VAD_detection at every triple of the grid (flat C order of
gate x ampl x amph, the triples themselves in ``gates`` / ``ampls`` / ``amphs``), ``f1_c`` = f1_score of each, and for the entropy
thresholds ``ethr``: ``ecounts_c`` / ``ef1_c`` of ``np.where(entropy > thr, 0, 1)`` (0.4 is the reference's own VAD_frequency).  Arrays only.

Cases: three GRADED signals h, i, j (seeds 201-203) — 3 s of make_golden_vad.py's noise floor, five tone bursts of 500-1300 Hz with linear
1500-sample ramps at peak amplitudes 30000 / 9000 / 7000 / 5500 / 11000 (frame powers that straddle the amph grid) and a 3000-sample
900 Hz stretch at amplitude 1500 (gated zero-crossing counts inside 20...40, power near the low ampl values) over the end of one burst's
ramp, labelled as non-speech — and make_golden_vad.py's cases c (a short run left open), d (3 frames) and g (digital silence, all-zero labels).

The generator ASSERTS what makes integer equality fair and what makes the grid worth sweeping, and refuses to write otherwise:
(a) no finite power within a relative 1e-4 of 0.1 or of any grid ampl / amph, no entropy within 1e-4 of an entropy threshold;
(b) every zcr value is an integer and every gate an x.5;
(c) the last frame is quiet under every (gate, ampl) (there the reference's wrap-around to index -1 equals a stop at 0);
(d) no sample equals -32768;
(e) every graded case has at least 20 distinct (tp, fp, fn) outcomes over the 125 triples, and along each of the three axes at least
    10 triples whose outcome changes when only that axis moves.

    python tests/golden/make_golden_vad_sweep.py
"""
import contextlib
import io
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_vad as MV  # noqa: E402  (the stubs, the noise floor and cases c / d / g)

GATES = (20.5, 25.5, 30.5, 35.5, 39.5)
AMPLS = (0.3, 0.9, 1.7, 2.6, 4.0)
AMPHS = (5.0, 7.5, 8.4, 12.0, 15.0)
ETHR = (0.2, 0.3, 0.4, 0.5, 0.7)
BAND = 1e-4
PEAKS = (30000, 9000, 7000, 5500, 11000)
GRADED = (("h", 201), ("i", 202), ("j", 203))


def graded(seed):
    """-> (int16 signal of 48000 samples, uint8 per-sample labels: 1 inside the five bursts)"""
    rng = np.random.default_rng(seed)
    n = 48000
    x = MV.noise(rng, n)
    y = np.zeros(n, dtype=np.uint8)
    ends = []
    for k in rng.permutation(5):
        at = 1500 + 8000 * int(k) + int(rng.integers(0, 500))
        m = int(rng.integers(5000, 6500))
        ends.append(at + m)
        f = rng.uniform(500, 1300)
        env = np.minimum(1.0, np.minimum(np.arange(m) + 1, m - np.arange(m)) / 1500.0)
        x[at:at + m] += PEAKS[k] * env * np.sin(2 * np.pi * f * np.arange(m) / 16000.0 + rng.uniform(0, 6.28))
        y[at:at + m] = 1
    at = ends[int(rng.integers(0, 5))] - 500   # behind a burst, over the end of its ramp: the forward walk meets it
    x[at:at + 3000] += 1500 * np.sin(2 * np.pi * 900 * np.arange(3000) / 16000.0)
    return MV.to_i16(x), y


def cases():
    out = {}
    for name, seed in GRADED:
        out[name] = graded(seed)
    old = MV.cases()
    y = np.zeros(old["c"].shape[0], dtype=np.uint8)
    y[10000:10800] = 1
    y[13000:19400] = 1
    out["c"] = (old["c"], y)
    y = np.zeros(old["d"].shape[0], dtype=np.uint8)
    y[0:60] = 1
    out["d"] = (old["d"], y)
    out["g"] = (old["g"], np.zeros(old["g"].shape[0], dtype=np.uint8))
    return out


def counts_of(res, ylab):
    m, y = np.asarray(res).reshape(-1) != 0, np.asarray(ylab).reshape(-1) != 0
    return [int((m & y).sum()), int((m & ~y).sum()), int((~m & y).sum())]


def main():
    VAD = MV.import_vad()
    from scipy.io import savemat
    from sklearn import metrics
    gates, ampls, amphs = (m.reshape(-1) for m in np.meshgrid(GATES, AMPLS, AMPHS, indexing="ij"))
    assert all(g * 2 == int(g * 2) and g != int(g) for g in GATES)                                      # (b)
    all_cases = cases()
    store = {"cases": np.array(list(all_cases)), "graded": np.array([n for n, _ in GRADED]), "gates": gates, "ampls": ampls, "amphs": amphs,
             "ethr": np.array(ETHR)}
    worst_p, worst_e = np.inf, np.inf
    for name, (x, y) in all_cases.items():
        assert x.dtype == np.int16 and not (x == -32768).any() and y.shape == x.shape, name               # (d)
        with warnings.catch_warnings(), np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("ignore")
            with tempfile.TemporaryDirectory() as tmp:
                savemat(os.path.join(tmp, "y.mat"), {"y_label": y.reshape(-1, 1)})
                ylab = VAD.label(os.path.join(tmp, "y.mat"))
            frames = VAD.enframe(x / (max(abs(x))))                                                       # wavdata's normalisation, VAD.py:131-132
            zcr, power, ent = VAD.feature(frames)
            assert ylab.shape == (frames.shape[1],), (name, ylab.shape)
            counts, f1 = [], []
            for g, lo, hi in zip(gates, ampls, amphs):
                res = VAD.VAD_detection(zcr, power, zcr_gate=g, ampl=lo, amph=hi)
                counts.append(counts_of(res, ylab))
                f1.append(metrics.f1_score(ylab.reshape(1, -1)[0], res.reshape(1, -1)[0]))               # cv, VAD.py:204-210
            ecounts, ef1 = [], []
            for thr in ETHR:
                res = np.where(ent > thr, 0, 1)
                ecounts.append(counts_of(res, ylab))
                ef1.append(metrics.f1_score(ylab, res.reshape(-1)))
        counts, ecounts = np.array(counts, dtype=np.int32), np.array(ecounts, dtype=np.int32)
        finite = np.isfinite(power[:, 0])
        assert np.array_equal(zcr, np.round(zcr)), name                                                   # (b)
        for thr in (0.1,) + AMPLS + AMPHS:                                                               # (a)
            d = np.abs(power[finite, 0] - thr) / thr
            worst_p = min(worst_p, d.min()) if d.size else worst_p
            assert not (d <= BAND).any(), (name, thr, d.min())
        for thr in ETHR:
            d = np.abs(ent[finite, 0] - thr) / thr
            worst_e = min(worst_e, d.min()) if d.size else worst_e
            assert not (d <= BAND).any(), (name, "entropy", thr, d.min())
        if finite.any():                                                                                  # (c)
            assert not (power[-1, 0] > min(AMPLS) or zcr[-1, 0] > min(GATES)), (name, "last frame is not quiet")
        distinct = len({tuple(c) for c in counts.tolist()})
        cube = counts.reshape(5, 5, 5, 3)
        axis_effect = [int((cube != np.roll(cube, 1, axis=a)).any(axis=3).sum()) for a in range(3)]     # differs from its cyclic neighbour along the axis
        if name in dict(GRADED):                                                                          # (e)
            assert distinct >= 20, (name, distinct)
            assert min(axis_effect) >= 10, (name, axis_effect)
        store["x_" + name], store["y_" + name], store["ylab_" + name] = x, y, ylab.astype(np.uint8)
        store["zcr_" + name], store["power_" + name], store["entropy_" + name] = zcr, power, ent
        store["counts_" + name], store["f1_" + name] = counts, np.array(f1, dtype=np.float64)
        store["ecounts_" + name], store["ef1_" + name] = ecounts, np.array(ef1, dtype=np.float64)
        print("%s: %6d samples %4d frames, %3d speech frames, %2d distinct outcomes, axis effects %s, best F1 %.4f" % (
            name, x.shape[0], frames.shape[1], int(ylab.sum()), distinct, axis_effect, max(f1)))
    print("smallest relative distance to a threshold: power %.3g, entropy %.3g" % (worst_p, worst_e))
    path = os.path.join(HERE, "vad_sweep.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
