"""Restatement of the x-vector forward pass (include/ssp.h, "x-vector extractor forward") in numpy: frame layer, statistics pooling,
network, pool windows.  float64 by default; ``dtype=np.float32`` evaluates the same formulas with float32 operands and products (the
pooling keeps its float64 accumulators, as the definition says) for the CPU precondition of the GPU network tests.  An ordinary module
like tests/lstm_oracle.py; tests/test_xvector_host.py corroborates it against torch.nn.functional.conv1d in float64."""
import numpy as np

SNYDER = ((5, 1), (3, 2), (3, 3), (1, 1), (1, 1))
# True: every output row is ONE matrix-vector product of the same shape whatever the sequence holds, so that a row's bits cannot depend
# on its neighbours (a BLAS picks its summation order by the shape of the whole product); slow, for the exact window-equality test
ROWWISE = False


def span(layer):
    W = np.asarray(layer["W"])
    return (W.shape[1] - 1) * int(layer.get("dilation", 1)) if W.ndim == 3 else 0


def receptive_field(frame_layers):
    return 1 + sum(span(L) for L in frame_layers)


def layer(x, L, dtype=np.float64, pre=False):
    """one frame layer on ONE sequence x (T, d_in) -> (max(0, T - span), units); W (units, taps, d_in) or (units, d_in) (taps = 1).
    pre: return z (before the activation, scale and offset) as well"""
    W = np.asarray(L["W"], dtype=dtype)
    if W.ndim == 2:
        W = W[:, None, :]
    dil = int(L.get("dilation", 1))
    x = np.asarray(x, dtype=dtype)
    units, taps, _ = W.shape
    To = max(0, x.shape[0] - (taps - 1) * dil)
    z = np.zeros((To, units), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if ROWWISE:
            Wm = np.ascontiguousarray(W.reshape(units, -1))
            for t in range(To):
                z[t] = Wm @ np.concatenate([x[t + j * dil] for j in range(taps)])
        else:
            for j in range(taps):   # taps ascending
                z = z + x[j * dil:j * dil + To] @ W[:, j, :].T
        if L.get("b") is not None:
            z = z + np.asarray(L["b"], dtype=dtype)
        a = np.where(z <= 0, dtype(0), z) if L.get("relu", False) else z     # (a NaN stays a NaN: NaN <= 0 is false)
        y = a
        if L.get("scale") is not None:
            y = y * np.asarray(L["scale"], dtype=dtype)
        if L.get("offset") is not None:
            y = y + np.asarray(L["offset"], dtype=dtype)
    return (y, z) if pre else y


def layer_bound(x, L):
    """the per-element error bound of ssp_tdnn_forward against layer(x, L) in float64: 1.01 (K + 1) 2^-23 (sum |x| |w| + |b|) before scale /
    offset; with them multiplied by |scale|, plus 2^-23 |y|"""
    W = np.asarray(L["W"], dtype=np.float64)
    if W.ndim == 2:
        W = W[:, None, :]
    A = {"W": np.abs(W), "dilation": L.get("dilation", 1), "b": None if L.get("b") is None else np.abs(np.asarray(L["b"], dtype=np.float64))}
    mag = layer(np.abs(np.asarray(x, dtype=np.float64)), A)
    K = W.shape[1] * W.shape[2]
    bound = 1.01 * (K + 1) * 2.0 ** -23 * mag
    if L.get("scale") is not None or L.get("offset") is not None:
        if L.get("scale") is not None:
            bound = bound * np.abs(np.asarray(L["scale"], dtype=np.float64))
        bound = bound + 2.0 ** -23 * np.abs(layer(x, L))
    return bound


def pool(x, var_floor=1e-10):
    """x (n, C) -> (2 C,) float32: means then deviations, centred population variance, float64 accumulators with t ascending, rounded to
    float32 once; n = 0: NaN"""
    x = np.asarray(x)
    n, C = x.shape
    if n == 0:
        return np.full(2 * C, np.nan, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(C, dtype=np.float64)
        for t in range(n):
            s += x[t].astype(np.float64)
        mean = s / n
        q = np.zeros(C, dtype=np.float64)
        for t in range(n):
            e = x[t].astype(np.float64) - mean
            q += e * e
        var = q / n
        var = np.where(var < var_floor, var_floor, var)   # (a NaN stays a NaN)
        return np.concatenate([mean, np.sqrt(var)]).astype(np.float32)


def frames(x, frame_layers, dtype=np.float64):
    """the last frame layer's rows of ONE sequence"""
    h = np.asarray(x, dtype=dtype)
    for L in frame_layers:
        h = layer(h, L, dtype)
    return h


def head(p, segment_layers, dtype=np.float64):
    h = np.asarray(p, dtype=dtype)[None, :]
    for L in segment_layers:
        h = layer(h, L, dtype)
    return h[0]


def embed(x, frame_layers, segment_layers, var_floor=1e-10, dtype=np.float64):
    """ONE sequence -> its embedding (float64 or float32 values; the pooled vector passes through float32, as the definition rounds it)"""
    return head(pool(frames(x, frame_layers, dtype), var_floor), segment_layers, dtype)


def network(feats, counts, frame_layers, segment_layers, var_floor=1e-10, windows=None, dtype=np.float64):
    """feats (frames, d_in) laid out by counts -> (n_seq or n_win, embed).  A window (sequence, first, end) pools the last frame layer's
    rows [first, end - R + 1) of its sequence, every sequence's frame layers computed ONCE"""
    off = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])
    R = receptive_field(frame_layers)
    H = [frames(feats[off[i]:off[i + 1]], frame_layers, dtype) for i in range(len(counts))]
    if windows is None:
        windows = [(i, 0, int(off[i + 1] - off[i])) for i in range(len(counts))]
    out = []
    for q, a, b in windows:
        rows = H[q][a:max(a, b - R + 1)]
        out.append(head(pool(rows, var_floor), segment_layers, dtype))
    return np.stack(out) if out else np.zeros((0, 0))


def random_layers(rng, d_in, spec, segment=(), affine=True):
    """spec: (units, taps, dilation, relu) per frame layer, segment: (units, relu) per segment layer; Glorot-uniform kernels, biases in
    [-0.1, 0.1], affine: scale in [0.5, 2] (sign flipped on every third unit) and offset in [-0.1, 0.1]"""
    def one(shape, fan, relu, dil=None):
        lim = np.sqrt(6.0 / fan)
        L = {"W": rng.uniform(-lim, lim, shape).astype(np.float32), "b": rng.uniform(-0.1, 0.1, shape[0]).astype(np.float32), "relu": bool(relu)}
        if dil is not None:
            L["dilation"] = dil
        if affine:
            sc = rng.uniform(0.5, 2.0, shape[0])
            sc[::3] *= -1
            L["scale"] = sc.astype(np.float32)
            L["offset"] = rng.uniform(-0.1, 0.1, shape[0]).astype(np.float32)
        return L
    fl, d = [], d_in
    for units, taps, dil, relu in spec:
        fl.append(one((units, taps, d), taps * d + units, relu, dil))
        d = units
    sl, d = [], 2 * d
    for units, relu in segment:
        sl.append(one((units, d), d + units, relu))
        d = units
    return fl, sl


def diar_signals():
    """two 8 kHz recordings of two synthetic voices for the Extractor-in-Diarizer.run tests: voice A a steady harmonic tone at 150 Hz, voice
    B at 410 Hz with a 20 Hz amplitude modulation of depth 0.7 (a difference that survives mean normalisation), noise inside the speech,
    near-silence between"""
    rng = np.random.RandomState(4)

    def voice(f0, n, am):
        t = np.arange(n)
        s = sum(6000.0 / k * np.sin(2 * np.pi * k * f0 * t / 8000.0) for k in (1, 2, 3, 5))
        return s * (1.0 + 0.7 * np.sin(2 * np.pi * am * t / 8000.0)) + rng.randn(n) * 100

    def quiet(n):
        return rng.randn(n) * 2.0
    a = np.concatenate([quiet(2560), voice(150, 9600, 0), quiet(3840), voice(410, 8960, 20), quiet(2560)])
    b = np.concatenate([quiet(1280), voice(410, 8320, 20), quiet(3840), voice(150, 9600, 0), quiet(1280)])
    return [a.astype(np.int16), b.astype(np.int16)]


def extractor_routes(sigs, net, window, win=3072, hop=1536, min_len=2560):
    """Both routes of xvector.Extractor inside diarize.Diarizer.run restated on the host in float64 — the VAD, MFCC (25-band sidekit preset
    at 8 kHz, frames of 256 every 128), sliding mean normalisation (window None: none), network and AHC restatements of this directory:
    "windows" extracts and normalises every recording once and pools frame windows, "chunks" extracts every window as a signal of its
    own.  -> {route: (L2-normalised embeddings, labels at two speakers per recording)}, windows per recording"""
    import diarize_oracle as DO
    import featnorm_oracle as FO
    import vad_oracle as VO
    from oracle import ref_cpu as O
    from speech_signal_processing_amd import diarize
    cfg, w, fb, dct = O.sidekit_tables(fs=8000, nwin=0.032, shift=0.016, nlogfilt=24, nceps=13, maxfreq=4000)

    def feats(x):
        f = O.mfcc_pipeline(np.asarray(x, dtype=np.float64), cfg, w, fb, dct).astype(np.float32)
        return FO.sliding(f, window, 0)[0].astype(np.float32) if window else f
    wins = []
    for x in sigs:
        zcr, power = VO.signal_features(np.asarray(x, dtype=np.float64))[:2]
        m = VO.detect(zcr, power)
        m = m[0] if isinstance(m, tuple) else m
        wins.append(diarize.windows(VO.speech_segments(m, len(x))[0], win, hop, min_len))
    counts = [w_.shape[0] for w_ in wins]
    out = {}
    for route in ("windows", "chunks"):
        embs = []
        for x, wn in zip(sigs, wins):
            f = feats(x) if route == "windows" else None
            for a, b in wn:
                rows = f[-(-a // 128):max(-(-a // 128), (b - 256) // 128 + 1)] if route == "windows" else feats(x[a:b])
                embs.append(embed(rows, net.frame_layers, net.segment_layers, net.var_floor))
        E = np.stack(embs)
        E = E / np.linalg.norm(E, axis=1, keepdims=True)
        S = DO.pairwise(E.astype(np.float32), DO.offsets(counts)).astype(np.float32)
        out[route] = (E, DO.ahc_batch(S, counts, "average", 0.0, n_speakers=[2] * len(counts))["labels"])
    return out, counts
