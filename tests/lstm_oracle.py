"""Restatement in numpy of the Keras LSTM cell the reference's recurrent d-vector network runs (d_vector.py:271-294: LSTM(128),
return_sequences False, use_bias True, no mask, zero initial state), for the tests of the GPU kernel.  Test code only: the package never
imports it.

    z_t = x_t W + h_{t-1} U + b        W (D, 4H)  U (H, 4H)  b (4H,)   gate blocks i | f | c | o
    i = s(z_i)  f = s(z_f)  g = tanh(z_c)  o = s(z_o)
    c_t = f c_{t-1} + i g              h_t = o tanh(c_t)               output h_T

s is 'hard_sigmoid' = clip(0.2 z + 0.5, 0, 1) or the logistic 'sigmoid'.  The arithmetic runs in ``dtype`` (float64 is the oracle; float32
is the yardstick of how far single precision alone drifts on given weights)."""
import numpy as np

ACTIVATIONS = ("hard_sigmoid", "sigmoid")


def _gate(z, act):
    if act == "hard_sigmoid":
        return np.clip(z.dtype.type(0.2) * z + z.dtype.type(0.5), 0, 1)
    if act == "sigmoid":
        return 1 / (1 + np.exp(-z))
    raise ValueError(act)


def forward(W, U, b, X, act, lengths=None, dtype=np.float64):
    """X (N, T, D) (rows beyond a sequence's length are never read into its state) -> h at every sequence's own last step, (N, H).
    A sequence of length 0 gives zeros."""
    W, U, X = (np.asarray(v, dtype=dtype) for v in (W, U, X))
    N, T, _ = X.shape
    H = U.shape[0]
    b = np.zeros(4 * H, dtype) if b is None else np.asarray(b, dtype=dtype)
    lengths = np.full(N, T) if lengths is None else np.asarray(lengths)
    h, c = np.zeros((N, H), dtype), np.zeros((N, H), dtype)
    for t in range(T):
        z = X[:, t] @ W + h @ U + b
        i, f, o = _gate(z[:, :H], act), _gate(z[:, H:2 * H], act), _gate(z[:, 3 * H:], act)
        cn = f * c + i * np.tanh(z[:, 2 * H:3 * H])
        hn = o * np.tanh(cn)
        on = (t < lengths)[:, None]
        c, h = np.where(on, cn, c), np.where(on, hn, h)
    return h


def forward_ragged(W, U, b, feats, offsets, act, dtype=np.float64):
    """feats (frames, D) laid out by offsets (n + 1) -> (n, H)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.diff(offsets)
    n, T = lengths.shape[0], int(lengths.max()) if lengths.size else 0
    X = np.zeros((n, T, feats.shape[1]), dtype)
    for s in range(n):
        X[s, :lengths[s]] = feats[offsets[s]:offsets[s + 1]]
    return forward(W, U, b, X, act, lengths, dtype)


def keras_init(rng, D, H, scale=1.0):
    """Keras' own initialisation of an LSTM layer, times ``scale``: Glorot-uniform kernel, an orthogonal block per gate for the recurrent
    kernel, zero bias with the forget block at one (unit_forget_bias)."""
    lim = np.sqrt(6.0 / (D + 4 * H))
    W = rng.uniform(-lim, lim, (D, 4 * H))
    U = np.concatenate([np.linalg.qr(rng.standard_normal((H, H)))[0] for _ in range(4)], axis=1)
    b = np.zeros(4 * H)
    b[H:2 * H] = 1.0
    return (scale * W).astype(np.float32), (scale * U).astype(np.float32), b.astype(np.float32)


def unpack_image(img, d_in, units):
    """The documented layout of ssp_lstm_pack_weights' image (include/ssp.h) read back into (W, U, b) of the padded shape:
    image[(((j G + g) 4 + q) 64 + lane) 4 + r], then bias [4][16 HT].  Returns (W (16 dT, 4, 16 HT), U (16 HT, 4, 16 HT), b (4, 16 HT))."""
    HT = 1 if units <= 16 else 2 if units <= 32 else 4 if units <= 64 else 8
    dT = (d_in + 15) // 16
    G = dT + HT
    img = np.asarray(img)
    assert img.shape == (HT * G * 1024 + 64 * HT,), img.shape
    body = img[:HT * G * 1024].reshape(HT, G, 4, 64, 4)
    M = np.zeros((16 * G, 4, 16 * HT), np.float32)   # [input row of [x | h]][gate][unit]
    for lane in range(64):
        for r in range(4):
            k = 4 * (lane >> 4) + r
            # body[j, g, q, lane, r] = M[16 g + k, q, 16 j + (lane & 15)]
            M[k::16, :, (lane & 15)::16] = body[:, :, :, lane, r].transpose(1, 2, 0)
    return M[:16 * dT], M[16 * dT:], img[HT * G * 1024:].reshape(4, 16 * HT)
