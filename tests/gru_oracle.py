"""Restatement in numpy of the conv + GRU d-vector network the reference trains (d_vector.py:213-269 inference_gru), for the tests of the
GPU kernels.  Test code only: the package never imports it.  Keras' arithmetic at inference:

    conv2d_same   Conv2D, one input channel, channels last, linear, TensorFlow's `same`: out = ceil(in / s),
                  pad = max((out - 1) s + k - in, 0), pad // 2 in front, the rest behind; a cross-correlation; then
                  TimeDistributed(Flatten): (To, Do F), index f_out F + c
    gru           W (d_in, 3H), U (H, 3H), gate blocks z | r | h, zero initial state, return_sequences; s = hard_sigmoid or sigmoid
                  reset_after False, b (3H,):     z = s(x W_z + b_z + h U_z)   r = s(x W_r + b_r + h U_r)   hh = tanh(x W_h + b_h + (r h) U_h)
                  reset_after True,  b (2, 3H):   z = s(x W_z + b_iz + h U_z + b_rz)   r likewise   hh = tanh(x W_h + b_ih + r (h U_h + b_rh))
                  h_t = z h_{t-1} + (1 - z) hh
    mean over time (t ascending), Dense, y / sqrt(max(sum y^2, 1e-12))

The arithmetic runs in ``dtype`` (float64 is the oracle; float32 is the yardstick of how far single precision alone drifts)."""
import numpy as np

ACTIVATIONS = ("hard_sigmoid", "sigmoid")
VARIANTS = [(a, r) for a in ACTIVATIONS for r in (False, True)]


def _gate(z, act):
    if act == "hard_sigmoid":
        return np.clip(z.dtype.type(0.2) * z + z.dtype.type(0.5), 0, 1)
    if act == "sigmoid":
        return 1 / (1 + np.exp(-z))
    raise ValueError(act)


def same_padding(n, k, s):
    """(out, before, after) of TensorFlow's `same` rule"""
    out = -(-n // s)
    pad = max((out - 1) * s + k - n, 0)
    return out, pad // 2, pad - pad // 2


def conv2d_same(X, K, b, strides, dtype=np.float64):
    """X (N, T, D), K (kh, kw, 1, F), b (F,) or None -> (N, To, Do * F)"""
    X, K = np.asarray(X, dtype=dtype), np.asarray(K, dtype=dtype)
    kh, kw, _, F = K.shape
    N, T, D = X.shape
    To, pt, pb = same_padding(T, kh, strides[0])
    Do, pl, pr = same_padding(D, kw, strides[1])
    Xp = np.pad(X, ((0, 0), (pt, pb), (pl, pr)))
    Y = np.zeros((N, To, Do, F), dtype)
    for i in range(kh):
        for j in range(kw):
            win = Xp[:, i:i + (To - 1) * strides[0] + 1:strides[0], j:j + (Do - 1) * strides[1] + 1:strides[1]]
            Y += win[..., None] * K[i, j, 0]
    if b is not None:
        Y += np.asarray(b, dtype=dtype)
    return Y.reshape(N, To, Do * F)


def gru(W, U, b, X, act, reset_after, dtype=np.float64):
    """X (N, T, d_in) -> the output sequence (N, T, H)"""
    W, U, X = (np.asarray(v, dtype=dtype) for v in (W, U, X))
    N, T, _ = X.shape
    H = U.shape[0]
    if b is None:
        bi, br = np.zeros(3 * H, dtype), np.zeros(3 * H, dtype)
    elif reset_after:
        b = np.asarray(b, dtype=dtype)
        assert b.shape == (2, 3 * H)
        bi, br = b[0], b[1]
    else:
        bi, br = np.asarray(b, dtype=dtype).reshape(3 * H), np.zeros(3 * H, dtype)
    h = np.zeros((N, H), dtype)
    out = np.zeros((N, T, H), dtype)
    one = dtype(1)
    for t in range(T):
        xp = X[:, t] @ W + bi
        if reset_after:
            hu = h @ U + br
            z = _gate(xp[:, :H] + hu[:, :H], act)
            r = _gate(xp[:, H:2 * H] + hu[:, H:2 * H], act)
            hh = np.tanh(xp[:, 2 * H:] + r * hu[:, 2 * H:])
        else:
            z = _gate(xp[:, :H] + h @ U[:, :H], act)
            r = _gate(xp[:, H:2 * H] + h @ U[:, H:2 * H], act)
            hh = np.tanh(xp[:, 2 * H:] + (r * h) @ U[:, 2 * H:])
        h = z * h + (one - z) * hh
        out[:, t] = h
    return out


def time_mean(seq):
    s = np.zeros((seq.shape[0], seq.shape[2]), seq.dtype)
    for t in range(seq.shape[1]):
        s += seq[:, t]
    return s / seq.dtype.type(seq.shape[1])


def l2_normalize(y, eps=1e-12):
    y = np.asarray(y)
    return y / np.sqrt(np.maximum((y * y).sum(axis=-1, keepdims=True), y.dtype.type(eps)))


def network(conv, grus, dense, X, act, reset_after, dtype=np.float64):
    """-> (embedding (N, E), mean over time of the last GRU (N, H))"""
    K, bc, strides = conv
    h = conv2d_same(X, K, bc, strides, dtype)
    for W, U, b in grus:
        h = gru(W, U, b, h, act, reset_after, dtype)
    m = time_mean(h)
    Wd, bd = dense
    y = m @ np.asarray(Wd, dtype=dtype)
    if bd is not None:
        y = y + np.asarray(bd, dtype=dtype)
    return l2_normalize(y), m


def glorot(rng, shape, fan_in, fan_out, scale=1.0):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return (scale * rng.uniform(-lim, lim, shape)).astype(np.float32)


def gru_init(rng, d_in, H, reset_after, scale=1.0, bias=True):
    """Keras' initialisation of a GRU layer times ``scale`` (Glorot-uniform kernel, an orthogonal block per gate) with a small random
    bias in place of Keras' zeros, so that the bias paths are exercised"""
    W = glorot(rng, (d_in, 3 * H), d_in, 3 * H, scale)
    U = (scale * np.concatenate([np.linalg.qr(rng.standard_normal((H, H)))[0] for _ in range(3)], axis=1)).astype(np.float32)
    b = None
    if bias:
        b = (0.1 * rng.standard_normal((2, 3 * H) if reset_after else (3 * H,))).astype(np.float32)
    return W, U, b


def network_init(rng, T, D, F, H, E, n_gru, reset_after, kernel=(5, 5), strides=(2, 2), scale=1.0):
    kh, kw = kernel
    K = glorot(rng, (kh, kw, 1, F), kh * kw, kh * kw * F, scale)
    bc = (0.1 * rng.standard_normal(F)).astype(np.float32)
    Do = -(-D // strides[1])
    grus, d_in = [], Do * F
    for _ in range(n_gru):
        grus.append(gru_init(rng, d_in, H, reset_after, scale))
        d_in = H
    Wd = glorot(rng, (H, E), H, E, scale)
    bd = (0.1 * rng.standard_normal(E)).astype(np.float32)
    return (K, bc, strides), grus, (Wd, bd)
