"""Float64 restatement of the voice activity detection the library implements (numpy only), for the randomised GPU checks.

Written from the description of the reference's VAD.py, not copied from it; tests/test_vad_host.py pins it to the reference's own
outputs in tests/golden/vad.npz (features to 1e-11, decisions exactly).  The product never imports this file.

Framing: frames of 256 samples every 128, ceil(n / 128) of them, zero padded behind the end, no window.  Features per frame: energy =
sum of squares; zero crossings = neighbouring pairs of opposite sign, kept where energy > 0.1; spectral entropy of the energy shares of
10 blocks of 12 bins among bins 0..127 of the 256-point spectrum.  Detector: the two-threshold state machine with its quirks (a run that
is too short stays open, a run open at the end is never flushed, the merge branch is dead); the backward walk stops at frame 0.
"""
import numpy as np

FRAME = 256
STEP = 128
MIN_LEN = 16
BAND = 1e-4   # relative distance to a threshold inside which fp32 and fp64 may decide differently


def num_frames(n, step=STEP):
    return -(-int(n) // step)


def normalise(x):
    """samples divided by the utterance's peak, int16 widened first (|-32768| = 32768); digital silence gives 0 / 0 = NaN"""
    x = np.asarray(x).reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / (np.max(np.abs(x)) if x.size else 1.0)


def enframe(x, step=STEP):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = num_frames(x.shape[0], step)
    idx = np.arange(FRAME)[:, None] + step * np.arange(n)[None, :]
    out = np.zeros((FRAME, n))
    inside = idx < x.shape[0]
    out[inside] = x[idx[inside]]
    return out


def features(frames):
    """(gated zcr, power, entropy) of the columns of a (256, n) matrix, float64 (n,) each"""
    frames = np.asarray(frames, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        power = (frames * frames).sum(axis=0)
        sg = np.sign(frames)
        cross = ((sg[:-1] * sg[1:]) < 0).sum(axis=0).astype(np.float64)
        zcr = cross * (power > 0.1)
        X = np.fft.fft(frames, axis=0)[:FRAME // 2]
        P = X.real ** 2 + X.imag ** 2
        eol = P.sum(axis=0)
        blocks = P[:120].reshape(10, 12, -1).sum(axis=1)
        s = blocks / (eol + 1e-8)
        ent = -(s * np.log2(s + 1e-8)).sum(axis=0)
    return zcr, power, ent


def signal_features(x, normalize=True):
    return features(enframe(normalise(x) if normalize else np.asarray(x, dtype=np.float64)))


def detect(zcr, power, zcr_gate=35, ampl=0.3, amph=12, min_len=MIN_LEN):
    zcr = np.asarray(zcr, dtype=np.float64).reshape(-1)
    power = np.asarray(power, dtype=np.float64).reshape(-1)
    n = power.shape[0]
    with np.errstate(invalid="ignore"):
        loud = power > amph
        active = (power > ampl) | (zcr > zcr_gate)
    res = np.zeros(n, dtype=np.uint8)
    is_open, start, end = False, 0, 0
    for i in range(n):
        if loud[i]:
            if not is_open:
                start = i
            end = i
            is_open = True
        elif end - start + 1 > min_len:
            while start >= 0 and active[start]:   # (stops at frame 0: the documented deviation from Python's wrap-around)
                start -= 1
            start += 1
            while end < n and active[end]:
                end += 1
            end -= 1
            res[start:end + 1] = 1
            is_open, start, end = False, 0, 0
    return res


def detect_frequency(entropy, threshold=0.4):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(entropy) > threshold, 0, 1).astype(np.uint8)


def near_threshold(zcr, power, entropy, ampl=0.3, amph=12):
    """frames whose power lies within BAND (relative) of 0.1, ampl or amph | whose entropy lies within BAND of 0.4"""
    with np.errstate(invalid="ignore"):
        p = np.zeros(power.shape, dtype=bool)
        for thr in (0.1, ampl, amph):
            p |= np.abs(power - thr) <= BAND * thr
        e = np.abs(entropy - 0.4) <= BAND * 0.4
    return p, e


def speech_segments(mask, n_samples):
    keep = np.zeros(int(n_samples), dtype=bool)
    for t in np.flatnonzero(np.asarray(mask).reshape(-1)):
        keep[t * STEP:t * STEP + FRAME] = True
    edges = np.flatnonzero(np.diff(np.concatenate(([0], keep.astype(np.int8), [0]))))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])], keep


def burst(rng, n, f0=None, amp=None):
    """a voiced-like burst of n samples: a few harmonics under a raised-cosine envelope"""
    f0 = rng.uniform(90, 260) if f0 is None else f0
    amp = rng.uniform(9000, 26000) if amp is None else amp
    t = np.arange(n) / 16000.0
    x = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6.28)) / h for h in range(1, 5))
    ramp = min(n // 2, int(rng.integers(120, 900)))
    env = np.ones(n)
    if ramp > 0:
        w = 0.5 - 0.5 * np.cos(np.pi * (np.arange(ramp) + 0.5) / ramp)
        env[:ramp] = w
        env[n - ramp:] = np.minimum(env[n - ramp:], w[::-1])
    return amp * env * x / 2.1


def random_signal(rng, n, start_in_speech=False, end_in_speech=False):
    """int16 test signal of n samples: background noise at about 0.4 % of full scale and a few bursts"""
    x = 131.0 * rng.standard_normal(n)
    if n >= 600:
        for k in range(int(rng.integers(1, 5))):
            m = int(rng.integers(300, max(301, min(n, 9000))))
            at = int(rng.integers(0, n - m + 1))
            if k == 0 and start_in_speech:
                at = 0
            if k == 1 and end_in_speech:
                at = n - m
            x[at:at + m] += burst(rng, m)
    return np.clip(np.round(x), -32767, 32767).astype(np.int16)


RANDOM_LENGTHS = (0, 1, 127, 128, 129, 255, 256, 257, 300)
# (seed, utterances, kind) of the randomised GPU checks.  About one frame in 10 000 of these signals lies within BAND of a threshold (three power
# thresholds and the entropy's 0.4, on frames spread over decades), so an utterance of F frames is set aside with probability ~ F / 10 000:
# utterances of 5 to 47 frames keep the expected share near 0.25 %, a quarter of the cap of 1 %; test_vad_host.py checks these very batches.
RANDOM_BATCHES = ((11, 400, "int16"), (12, 400, "float32"), (13, 400, "unnormalised"))


def random_batch(seed, n_utt):
    """ragged batch: the short lengths above, then random lengths; every third long utterance starts or ends in speech"""
    rng = np.random.default_rng(seed)
    out = []
    for u in range(n_utt):
        n = RANDOM_LENGTHS[u] if u < len(RANDOM_LENGTHS) else int(rng.integers(600, 6000))
        out.append(random_signal(rng, n, start_in_speech=(u % 3 == 0), end_in_speech=(u % 3 == 1)))
    return out


def batch_of(seed, n_utt, kind):
    """-> (signals, normalize).  int16: PCM as utils.tools.read returns it; float32: the same integers; unnormalised: float32 in about
    [-2, 2], taken as they are (noise frames stay under the 0.1 gate, bursts pass amph)"""
    sigs = random_batch(seed, n_utt)
    if kind == "float32":
        return [s.astype(np.float32) for s in sigs], True
    if kind == "unnormalised":
        return [(s.astype(np.float32) / np.float32(32768.0)) * np.float32(2.0) for s in sigs], False
    return sigs, True
