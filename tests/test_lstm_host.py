"""CPU-side tests of the LSTM d-vector network: the float64 restatement (tests/lstm_oracle.py) against torch.nn.LSTM on the CPU and
against a hand-computed case, the packed weight image against its documented layout, and that nothing computes without a device.
(Unpinned against Keras: the reference tree holds no LSTM weights or outputs and Keras is not a dependency; torch's cell is the
corroboration for the sigmoid mode, the hand computation for hard_sigmoid.)"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_oracle as LO  # noqa: E402


def test_oracle_sigmoid_matches_torch_lstm_float64():
    """W.T -> weight_ih, U.T -> weight_hh (torch's gate order i | f | g | o is Keras' i | f | c | o), bias on one side: <= 1e-13"""
    import torch
    rng = np.random.default_rng(3)
    worst = 0.0
    for D, H, T, N in ((13, 128, 98, 37), (26, 64, 31, 9), (5, 16, 7, 4)):
        W, U, b = LO.keras_init(rng, D, H, 1.5)
        b = (b + 0.1 * rng.standard_normal(4 * H)).astype(np.float32)
        X = 3 * rng.standard_normal((N, T, D))
        net = torch.nn.LSTM(D, H, batch_first=True).double()
        with torch.no_grad():
            net.weight_ih_l0.copy_(torch.from_numpy(W.T.astype(np.float64)))
            net.weight_hh_l0.copy_(torch.from_numpy(U.T.astype(np.float64)))
            net.bias_ih_l0.copy_(torch.from_numpy(b.astype(np.float64)))
            net.bias_hh_l0.zero_()
            out, (hT, _) = net(torch.from_numpy(X))
        got = LO.forward(W, U, b, X, "sigmoid")
        worst = max(worst, float(np.abs(got - hT[0].numpy()).max()))
        # ragged: a sequence cut at length L equals torch's output row at step L - 1
        lengths = rng.integers(1, T + 1, N)
        rag = LO.forward(W, U, b, X, "sigmoid", lengths)
        worst = max(worst, float(np.abs(rag - out.numpy()[np.arange(N), lengths - 1]).max()))
    print("oracle vs torch.nn.LSTM float64: %.3e" % worst)
    assert worst <= 1e-13


def test_oracle_hard_sigmoid_three_steps_by_hand():
    """D = 1, H = 1, weights chosen so that the gates sit in the linear part, below 0 and above 1 of clip(0.2 z + 0.5, 0, 1)"""
    W = np.array([[1.0, 2.0, 0.5, -1.0]])
    U = np.array([[0.5, -4.0, 1.0, 10.0]])
    b = np.array([0.0, 1.0, 0.0, 0.5])
    x = [1.0, -2.0, 3.0]
    h = c = 0.0
    hs = lambda z: min(max(0.2 * z + 0.5, 0.0), 1.0)  # noqa: E731
    seen = set()
    for xt in x:
        z = [xt * W[0, q] + h * U[0, q] + b[q] for q in range(4)]
        for q in (0, 1, 3):
            seen.add("lo" if 0.2 * z[q] + 0.5 < 0 else "hi" if 0.2 * z[q] + 0.5 > 1 else "mid")
        c = hs(z[1]) * c + hs(z[0]) * np.tanh(z[2])
        h = hs(z[3]) * np.tanh(c)
    assert "mid" in seen and ("lo" in seen or "hi" in seen)
    got = LO.forward(W, U, b, np.array(x).reshape(1, 3, 1), "hard_sigmoid")
    assert abs(got[0, 0] - h) <= 1e-15
    # step 1 written out: z = (1, 3, 0.5, -0.5): i = 0.7, f = 1 (clipped from 1.1), o = 0.4; c = 0.7 tanh(0.5); h = 0.4 tanh(c)
    one = LO.forward(W, U, b, np.array([[[1.0]]]), "hard_sigmoid")
    assert abs(one[0, 0] - 0.4 * np.tanh(0.7 * np.tanh(0.5))) <= 1e-15
    assert abs(LO.forward(W, U, b, np.array([[[1.0]]]), "sigmoid")[0, 0] - one[0, 0]) > 1e-3      # the two modes differ
    assert np.array_equal(LO.forward(W, U, b, np.zeros((2, 0, 1)), "sigmoid"), np.zeros((2, 1)))   # no steps: zero state


def test_oracle_ragged_layout_and_zero_length():
    rng = np.random.default_rng(5)
    W, U, b = LO.keras_init(rng, 13, 16)
    lengths = np.array([3, 0, 7, 1])
    off = np.concatenate(([0], np.cumsum(lengths)))
    feats = rng.standard_normal((off[-1], 13))
    got = LO.forward_ragged(W, U, b, feats, off, "hard_sigmoid")
    for s, n in enumerate(lengths):
        alone = LO.forward(W, U, b, feats[off[s]:off[s + 1]][None], "hard_sigmoid")[0] if n else np.zeros(16)
        assert np.abs(got[s] - alone).max() <= 1e-14, s   # (the host's matrix product may round a batch and a single row differently)
    assert not got[1].any() and got[0].any()


@pytest.mark.parametrize("d_in,units", [(13, 128), (26, 64), (39, 16), (64, 48), (1, 112), (17, 32)])
def test_packed_weight_image_round_trips(d_in, units):
    """ssp_lstm_pack_weights (host only: no context, no device) against the layout include/ssp.h documents; padding is zero"""
    from speech_signal_processing_amd import api
    rng = np.random.default_rng(d_in * 1000 + units)
    W = rng.standard_normal((d_in, 4 * units)).astype(np.float32)
    U = rng.standard_normal((units, 4 * units)).astype(np.float32)   # (asymmetric: a transposed image cannot pass)
    b = rng.standard_normal(4 * units).astype(np.float32)
    Wp, Up, bp = LO.unpack_image(api.lstm_pack_weights(W, U, b), d_in, units)
    assert np.array_equal(Wp[:d_in, :, :units], W.reshape(d_in, 4, units))
    assert np.array_equal(Up[:units, :, :units], U.reshape(units, 4, units))
    assert np.array_equal(bp[:, :units], b.reshape(4, units))
    assert not Wp[d_in:].any() and not Wp[:, :, units:].any() and not Up[units:].any() and not Up[:, :, units:].any() and not bp[:, units:].any()
    nob = LO.unpack_image(api.lstm_pack_weights(W, U, None), d_in, units)[2]
    assert not nob.any()


def test_bad_arguments_are_refused_before_any_gpu_work():
    """null handles, a bad activation enum and shapes the kernel does not cover are answered without a device"""
    from speech_signal_processing_amd import _lib, api
    lib = _lib.load()
    W = np.zeros((13, 512), np.float32)
    U = np.zeros((128, 512), np.float32)
    out = ctypes.c_void_p()
    wp, up = W.ctypes.data, U.ctypes.data
    assert lib.ssp_lstm_create(None, 13, 128, wp, up, None, 0, None) == _lib.SSP_ERR_INVALID               # null out
    assert lib.ssp_lstm_create(None, 13, 128, None, up, None, 0, ctypes.byref(out)) == _lib.SSP_ERR_INVALID   # null kernel
    assert lib.ssp_lstm_create(None, 13, 128, wp, None, None, 0, ctypes.byref(out)) == _lib.SSP_ERR_INVALID
    for enum in (-1, 2, 7):
        assert lib.ssp_lstm_create(None, 13, 128, wp, up, None, enum, ctypes.byref(out)) == _lib.SSP_ERR_INVALID
        assert b"recurrent_activation" in lib.ssp_last_error()
    for d_in, units in ((0, 128), (13, 0), (-3, 16)):
        assert lib.ssp_lstm_create(None, d_in, units, wp, up, None, 1, ctypes.byref(out)) == _lib.SSP_ERR_INVALID
    for d_in, units in ((13, 100), (13, 144), (13, 256), (65, 128), (13, 8)):
        assert lib.ssp_lstm_create(None, d_in, units, wp, up, None, 1, ctypes.byref(out)) == _lib.SSP_ERR_UNSUPPORTED, (d_in, units)
        n = ctypes.c_int64()
        assert lib.ssp_lstm_pack_weights(d_in, units, None, None, None, None, ctypes.byref(n)) == _lib.SSP_ERR_UNSUPPORTED
    assert lib.ssp_lstm_create(None, 13, 128, wp, up, None, 1, ctypes.byref(out)) == _lib.SSP_ERR_INVALID   # a good shape, but no ctx
    assert not out.value
    assert lib.ssp_lstm_forward(None, None, None, None, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_lstm_destroy(None) == _lib.SSP_OK
    n = ctypes.c_int64()
    assert lib.ssp_lstm_pack_weights(13, 128, None, None, None, None, ctypes.byref(n)) == _lib.SSP_OK and n.value == 8 * 9 * 1024 + 512
    assert lib.ssp_lstm_pack_weights(13, 128, None, None, None, None, None) == _lib.SSP_ERR_INVALID
    img = np.zeros(n.value, np.float32)
    assert lib.ssp_lstm_pack_weights(13, 128, None, up, None, img.ctypes.data, None) == _lib.SSP_ERR_INVALID
    with pytest.raises(NotImplementedError):
        api.lstm_pack_weights(np.zeros((13, 400), np.float32), np.zeros((100, 400), np.float32))
    with pytest.raises(ValueError):
        api.lstm_pack_weights(np.zeros((13, 512), np.float32), np.zeros((128, 500), np.float32))


def test_python_surface_names_the_activation_and_fails_loudly_without_gpu():
    """recurrent_activation is a required keyword of LstmNet (no silent default); without a device building a net raises"""
    import torch
    from speech_signal_processing_amd import _lib, d_vector
    W, U, b = LO.keras_init(np.random.default_rng(0), 13, 16)
    with pytest.raises(TypeError):
        d_vector.LstmNet(W, U, b)
    with pytest.raises(TypeError):
        d_vector.LstmNet(W, U, b, "sigmoid")
    if torch.cuda.is_available():
        return
    with pytest.raises((_lib.SspError, RuntimeError)):   # (torch's stream lookup or the library's context: neither computes on the CPU)
        d_vector.LstmNet(W, U, b, recurrent_activation="sigmoid")


def test_product_never_imports_the_test_oracle():
    pkg = os.path.join(ROOT, "speech_signal_processing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(tests|oracle|lstm_oracle)\b", text, flags=re.M), os.path.join(dirpath, f)
                assert "lstm_oracle" not in text, os.path.join(dirpath, f)
