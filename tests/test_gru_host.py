"""CPU-side tests of the conv + GRU d-vector network: the float64 restatement (tests/gru_oracle.py) against torch.nn.GRU and
torch.nn.functional.conv2d on the CPU and against hand-computed steps, the header and the bindings, and that nothing computes without a
device.  (Unpinned against Keras: the reference tree holds no GRU weights or outputs and Keras is not a dependency; torch's cell is the
corroboration for sigmoid with reset_after, the hand computation for hard_sigmoid without.)"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_oracle as GO  # noqa: E402


def test_oracle_sigmoid_reset_after_matches_torch_gru_float64():
    """torch's gate order is r | z | n and its cell is the reset_after form with both bias rows: reorder the blocks, <= 1e-12"""
    import torch
    rng = np.random.default_rng(11)
    worst = 0.0
    for D, H, T, N in ((448, 64, 49, 5), (13, 48, 21, 9), (7, 16, 1, 3)):
        W, U, b = GO.gru_init(rng, D, H, True, 1.5)

        def tz(M):  # columns z | r | h -> rows r | z | n
            M = np.asarray(M, np.float64)
            return np.concatenate([M[..., H:2 * H], M[..., :H], M[..., 2 * H:]], axis=-1)
        X = 3 * rng.standard_normal((N, T, D))
        net = torch.nn.GRU(D, H, batch_first=True).double()
        with torch.no_grad():
            net.weight_ih_l0.copy_(torch.from_numpy(tz(W).T.copy()))
            net.weight_hh_l0.copy_(torch.from_numpy(tz(U).T.copy()))
            net.bias_ih_l0.copy_(torch.from_numpy(tz(b[0])))
            net.bias_hh_l0.copy_(torch.from_numpy(tz(b[1])))
            out, _ = net(torch.from_numpy(X))
        got = GO.gru(W, U, b, X, "sigmoid", True)
        worst = max(worst, float(np.abs(got - out.numpy()).max()))
    print("oracle vs torch.nn.GRU float64: %.3e" % worst)
    assert worst <= 1e-12


def test_oracle_hard_sigmoid_no_reset_after_three_steps_by_hand():
    """d_in = 1, H = 2: the candidate multiplies (r . h) by U_h (not r by (h U_h)), gates in the linear part and clipped"""
    W = np.array([[1.0, -3.0, 2.0, 0.5, 0.7, -1.0]])                      # z0 z1 | r0 r1 | h0 h1
    U = np.array([[0.5, 1.0, -2.0, 4.0, 1.0, -0.5], [2.0, -1.0, 3.0, 0.25, 0.3, 2.0]])
    b = np.array([0.1, 0.0, -0.2, 0.3, 0.0, 0.05])
    xs = [1.0, -2.0, 3.0]
    hs = lambda v: min(max(0.2 * v + 0.5, 0.0), 1.0)  # noqa: E731
    h = [0.0, 0.0]
    seen = set()
    want = []
    for x in xs:
        z = [hs(x * W[0, u] + b[u] + h[0] * U[0, u] + h[1] * U[1, u]) for u in range(2)]
        pre_r = [x * W[0, 2 + u] + b[2 + u] + h[0] * U[0, 2 + u] + h[1] * U[1, 2 + u] for u in range(2)]
        for v in pre_r:
            seen.add("lo" if 0.2 * v + 0.5 < 0 else "hi" if 0.2 * v + 0.5 > 1 else "mid")
        r = [hs(v) for v in pre_r]
        rh = [r[0] * h[0], r[1] * h[1]]
        hh = [np.tanh(x * W[0, 4 + u] + b[4 + u] + rh[0] * U[0, 4 + u] + rh[1] * U[1, 4 + u]) for u in range(2)]
        h = [z[u] * h[u] + (1 - z[u]) * hh[u] for u in range(2)]
        want.append(list(h))
    assert "mid" in seen and ("lo" in seen or "hi" in seen), seen
    got = GO.gru(W, U, b, np.array(xs).reshape(1, 3, 1), "hard_sigmoid", False)
    assert np.abs(got[0] - np.array(want)).max() <= 1e-15
    # step 1 written out: z = hs(1.1), hs(-3) = 0.72, 0;  hh = tanh(0.7), tanh(-0.95);  h = (1 - z) hh
    assert abs(got[0, 0, 0] - 0.28 * np.tanh(0.7)) <= 1e-15 and abs(got[0, 0, 1] - np.tanh(-0.95)) <= 1e-15
    # the two placements of r differ once h is non-zero, and so do the two activations
    b2 = np.stack([b, np.zeros(6)])
    assert np.abs(GO.gru(W, U, b2, np.array(xs).reshape(1, 3, 1), "hard_sigmoid", True)[0, 1:] - got[0, 1:]).max() > 1e-3
    assert np.abs(GO.gru(W, U, b, np.array(xs).reshape(1, 3, 1), "sigmoid", False) - got).max() > 1e-3


@pytest.mark.parametrize("T,D", [(98, 13), (97, 14), (1, 1), (5, 3)])
@pytest.mark.parametrize("k", [5, 3, 1])
@pytest.mark.parametrize("strides", [(2, 2), (1, 1), (2, 1)])
def test_oracle_convolution_matches_torch_conv2d_float64(T, D, k, strides):
    import torch
    rng = np.random.default_rng(T * 100 + D * 10 + k)
    F = 6
    X = rng.standard_normal((3, T, D))
    K = rng.standard_normal((k, k, 1, F))
    b = rng.standard_normal(F)
    To, pt, pb = GO.same_padding(T, k, strides[0])
    Do, pl, pr = GO.same_padding(D, k, strides[1])
    xp = torch.nn.functional.pad(torch.from_numpy(X)[:, None], (pl, pr, pt, pb))
    ref = torch.nn.functional.conv2d(xp, torch.from_numpy(K).permute(3, 2, 0, 1).contiguous(), torch.from_numpy(b), stride=strides)
    ref = ref.permute(0, 2, 3, 1).reshape(3, To, Do * F).numpy()      # (N, F, To, Do) -> (N, To, Do F)
    got = GO.conv2d_same(X, K, b, strides)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12


def test_same_padding_of_the_reference_shape():
    assert GO.same_padding(98, 5, 2) == (49, 1, 2) and GO.same_padding(13, 5, 2) == (7, 2, 2)


def test_oracle_l2_normalisation():
    rng = np.random.default_rng(2)
    y = rng.standard_normal((5, 512))
    y[3] = 0.0
    y[4] = 1e-9 * y[4] / np.linalg.norm(y[4])      # sum of squares 1e-18 < eps: divided by sqrt(eps) = 1e-6
    n = GO.l2_normalize(y)
    assert np.abs(np.linalg.norm(n[:3], axis=1) - 1).max() <= 1e-14
    assert np.abs(n[0] - y[0] / np.linalg.norm(y[0])).max() <= 1e-15
    assert not n[3].any() and np.isfinite(n).all()
    assert abs(np.linalg.norm(n[4]) - 1e-3) <= 1e-12


def test_header_declares_and_bindings_bind_the_new_entries():
    from speech_signal_processing_amd import _lib
    text = open(os.path.join(ROOT, "include", "ssp.h")).read()
    lib = _lib.load()
    for name in ("ssp_gru_create", "ssp_gru_destroy", "ssp_gru_forward", "ssp_conv2d_same_forward", "ssp_l2_normalize"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct ssp_gru ssp_gru;" in text
    assert re.search(r"#define SSP_ABI_VERSION 4\b", text) and lib.ssp_abi_version() == 4      # no version step
    assert "d_vector.py:213-269" in text


def test_bad_arguments_are_refused_before_any_gpu_work():
    from speech_signal_processing_amd import _lib
    lib = _lib.load()
    W = np.zeros((7, 3 * 1024), np.float32)
    U = np.zeros((1024, 3 * 1024), np.float32)
    out = ctypes.c_void_p()
    o = ctypes.byref(out)
    wp, up = W.ctypes.data, U.ctypes.data
    for units in (1040, 24):
        assert lib.ssp_gru_create(None, 7, units, wp, up, None, 1, 1, o) == _lib.SSP_ERR_UNSUPPORTED, units
    assert lib.ssp_gru_create(None, 4097, 16, wp, up, None, 1, 1, o) == _lib.SSP_ERR_UNSUPPORTED
    assert lib.ssp_gru_create(None, 0, 16, wp, up, None, 1, 1, o) == _lib.SSP_ERR_INVALID            # d_in 0
    assert lib.ssp_gru_create(None, 7, 16, wp, up, None, 1, 2, o) == _lib.SSP_ERR_INVALID            # reset_after 2
    assert b"reset_after" in lib.ssp_last_error()
    assert lib.ssp_gru_create(None, 7, 16, wp, up, None, 2, 0, o) == _lib.SSP_ERR_INVALID            # activation 2
    assert b"recurrent_activation" in lib.ssp_last_error()
    assert lib.ssp_gru_create(None, 7, 16, None, up, None, 1, 1, o) == _lib.SSP_ERR_INVALID          # a null array
    assert lib.ssp_gru_create(None, 7, 16, wp, None, None, 1, 1, o) == _lib.SSP_ERR_INVALID
    assert lib.ssp_gru_create(None, 7, 16, wp, up, None, 1, 1, None) == _lib.SSP_ERR_INVALID         # null out
    assert lib.ssp_gru_create(None, 7, 1024, wp, up, None, 1, 1, o) == _lib.SSP_ERR_INVALID          # a good shape, but no ctx
    assert not out.value
    assert lib.ssp_gru_forward(None, None, 1, 1, None, None, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_gru_destroy(None) == _lib.SSP_OK
    x = np.zeros((1, 5, 3), np.float32)
    k = np.zeros((8, 8, 1, 4), np.float32)
    y = np.zeros((1, 5, 3 * 4), np.float32)
    xp, kp, yp = x.ctypes.data, k.ctypes.data, y.ctypes.data
    assert lib.ssp_conv2d_same_forward(None, xp, 1, 5, 3, kp, None, 8, 5, 4, 1, 1, yp, 0, None) == _lib.SSP_ERR_UNSUPPORTED   # kh = 8
    assert lib.ssp_conv2d_same_forward(None, xp, 1, 5, 3, kp, None, 5, 5, 257, 1, 1, yp, 0, None) == _lib.SSP_ERR_UNSUPPORTED
    assert lib.ssp_conv2d_same_forward(None, xp, 1, 5, 3, kp, None, 5, 5, 4, 3, 1, yp, 0, None) == _lib.SSP_ERR_UNSUPPORTED
    assert lib.ssp_conv2d_same_forward(None, xp, 1, 5, 3, kp, None, 5, 5, 4, 0, 1, yp, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_conv2d_same_forward(None, xp, 1, 5, 3, None, None, 5, 5, 4, 1, 1, yp, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_conv2d_same_forward(None, None, 1, 5, 3, kp, None, 5, 5, 4, 1, 1, yp, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_conv2d_same_forward(None, xp, 1, 5, 3, kp, None, 5, 5, 4, 1, 1, yp, 0, None) == _lib.SSP_ERR_INVALID      # no ctx
    assert lib.ssp_l2_normalize(None, None, 1, 4, 1e-12, yp, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_l2_normalize(None, xp, 1, 0, 1e-12, yp, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_l2_normalize(None, xp, 1, 4, 1e-12, yp, 0, None) == _lib.SSP_ERR_INVALID                                  # no ctx


def test_python_surface_names_both_switches_and_fails_loudly_without_gpu():
    import torch
    from speech_signal_processing_amd import _lib, api, d_vector
    rng = np.random.default_rng(0)
    conv, grus, dense = GO.network_init(rng, 10, 6, 4, 16, 8, 1, False)
    with pytest.raises(TypeError):
        d_vector.ConvGruNet(conv, grus, dense)
    with pytest.raises(TypeError):
        d_vector.ConvGruNet(conv, grus, dense, recurrent_activation="sigmoid")
    with pytest.raises(TypeError):
        d_vector.ConvGruNet(conv, grus, dense, reset_after=False)
    with pytest.raises(TypeError):
        d_vector.ConvGruNet(conv, grus, dense, "sigmoid", False)
    with pytest.raises(ValueError):
        d_vector.ConvGruNet(conv, grus, dense, recurrent_activation="relu", reset_after=False)
    with pytest.raises(ValueError):
        d_vector.ConvGruNet(conv, grus, dense, recurrent_activation="sigmoid", reset_after=None)
    with pytest.raises(TypeError):
        api.GruForward(None, *grus[0])
    with pytest.raises(ValueError):
        api.GruForward(None, *grus[0], "tanh", False)
    with pytest.raises(ValueError):
        api.GruForward(None, *grus[0], "sigmoid", 2)
    if torch.cuda.is_available():
        return
    with pytest.raises((_lib.SspError, RuntimeError, AssertionError)):   # (torch's stream lookup or the library's context: neither computes on the CPU)
        d_vector.ConvGruNet(conv, grus, dense, recurrent_activation="sigmoid", reset_after=False)


def test_product_never_imports_the_test_oracle():
    pkg = os.path.join(ROOT, "speech_signal_processing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert "gru_oracle" not in text, os.path.join(dirpath, f)
