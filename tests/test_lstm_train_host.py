"""CPU tests around the recurrent d-vector network's training: the float64 restatement (tests/lstm_train_oracle.py) against torch.autograd
and against central differences, the Keras initialisation, and what the header, the bindings and the build declare.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_train_oracle as LO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ssp_lstm_trainer_create", "ssp_lstm_trainer_destroy", "ssp_lstm_trainer_epoch", "ssp_lstm_trainer_evaluate", "ssp_lstm_trainer_read",
       "ssp_lstm_trainer_steps"]


def _case(seed, d_in=5, units=6, T=7, B=9, C=4, bias=True):
    rng = np.random.default_rng(seed)
    W, U, b, Wd, bd = LO.keras_init(rng, d_in, units, C)
    b = (b + 0.1 * rng.standard_normal(b.shape)).astype(np.float32)
    bd = (0.1 * rng.standard_normal(bd.shape)).astype(np.float32)
    X = (3.0 * rng.standard_normal((B, T, d_in))).astype(np.float32)
    y = rng.integers(0, C, B)
    return (W, U, b if bias else None, Wd, bd if bias else None), X, y


def _torch_grads(params, X, y, activation):
    import torch
    W, U, b, Wd, bd = [None if p is None else torch.tensor(np.asarray(p, np.float64), requires_grad=True) for p in params]
    x = torch.tensor(np.asarray(X, np.float64))
    B, T, _ = x.shape
    H = U.shape[0]
    s = torch.sigmoid if activation == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T):
        z = x[:, t] @ W + h @ U
        if b is not None:
            z = z + b
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
    logits = h @ Wd
    if bd is not None:
        logits = logits + bd
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(np.asarray(y, np.int64)), reduction="mean")
    loss.backward()
    return {k: None if p is None else p.grad.numpy() for k, p in zip(LO.NAMES, (W, U, b, Wd, bd))}, float(loss.detach()) * B


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("activation", ["hard_sigmoid", "sigmoid"])
def test_oracle_gradients_equal_torch_autograd(activation, bias):
    params, X, y = _case(3, bias=bias)
    net = LO.Net(*params, activation)
    h, stash = net.forward(X)
    loss, _, g = net.loss(net.logits(h), y)
    got = net.backward(h, stash, g)
    ref, ref_loss = _torch_grads(params, X, y, activation)
    assert abs(loss - ref_loss) <= 1e-10 * abs(ref_loss)
    for k in LO.NAMES:
        assert (got[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            assert np.abs(got[k] - ref[k]).max() <= 1e-10 * np.abs(ref[k]).max(), k


@pytest.mark.parametrize("activation", ["hard_sigmoid", "sigmoid"])
def test_oracle_gradients_equal_central_differences(activation):
    """random entries of all five tensors; hard_sigmoid only on inputs whose clip margin exceeds the step"""
    eps = 1e-6
    for seed in range(20):
        params, X, y = _case(40 + seed)
        net = LO.Net(*params, activation)
        h, stash = net.forward(X)
        if activation == "sigmoid" or net.min_clip > 1e-3:   # (1e-3: far more than eps times any input or state)
            break
    else:
        raise AssertionError("no seed with a clip margin")
    _, _, g = net.loss(net.logits(h), y)
    grads = net.backward(h, stash, g)
    B = len(y)

    def mean_loss(p):
        n = LO.Net(*p, activation)
        hh, _ = n.forward(X)
        return n.loss(n.logits(hh), y)[0] / B
    rng = np.random.default_rng(9)
    for ti, k in enumerate(LO.NAMES):
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in params[ti].shape)
            hi = [np.array(p, np.float64) for p in params]
            lo = [np.array(p, np.float64) for p in params]
            hi[ti][idx] += eps
            lo[ti][idx] -= eps
            num = (mean_loss(hi) - mean_loss(lo)) / (2 * eps)
            assert abs(num - grads[k][idx]) <= 1e-6 * max(1.0, np.abs(grads[k]).max()) + 1e-8, (k, idx, num, grads[k][idx])


def test_oracle_records_margins():
    params, X, y = _case(5)
    net = LO.Net(*params, "hard_sigmoid")
    net.step(X, y, 1e-4)
    assert np.isfinite(net.min_clip) and np.isfinite(net.min_margin) and net.t == 1
    net = LO.Net(*params, "sigmoid")
    net.step(X, y, 1e-4)
    assert net.min_clip == np.inf and np.isfinite(net.min_margin)


def test_float32_oracle_stays_close_to_float64():
    params, X, y = _case(6, d_in=13, units=16, T=9, B=19, C=5)
    a, b = LO.Net(*params, "sigmoid", np.float64), LO.Net(*params, "sigmoid", np.float32)
    a.step(X, y, 1e-4)
    b.step(X, y, 1e-4)
    for k in LO.NAMES:
        assert b.g[k].dtype == np.float32
        assert np.abs(b.g[k] - a.g[k]).max() <= 1e-5 * np.abs(a.g[k]).max(), k


def test_keras_initialiser():
    W, U, b, Wd, bd = LO.keras_init(np.random.default_rng(0), 13, 128, 40)
    assert W.shape == (13, 512) and U.shape == (128, 512) and b.shape == (512,) and Wd.shape == (128, 40) and bd.shape == (40,)
    assert np.abs(U.astype(np.float64) @ U.T.astype(np.float64) - np.eye(128)).max() <= 1e-6
    assert np.array_equal(b[128:256], np.ones(128, np.float32)) and not b[:128].any() and not b[256:].any() and not bd.any()
    assert np.abs(W).max() <= np.sqrt(6.0 / (13 + 512)) and np.abs(W).max() > 0.9 * np.sqrt(6.0 / (13 + 512))
    assert np.abs(Wd).max() <= np.sqrt(6.0 / (128 + 40)) and np.abs(Wd).max() > 0.9 * np.sqrt(6.0 / (128 + 40))
    # the same seed gives the same draws, and the package's initialisation is this one
    again = LO.keras_init(np.random.default_rng(0), 13, 128, 40)
    assert all(np.array_equal(x, r) for x, r in zip((W, U, b, Wd, bd), again))


def test_header_bindings_and_build_declare_the_trainer():
    from speech_signal_processing_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "ssp.h")).read()
    assert re.search(r"#define SSP_ABI_VERSION 4\b", hdr) and L.ABI_VERSION == 4
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.ssp_abi_version.restype = ctypes.c_int
    assert lib.ssp_abi_version() == 4
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    for cite in ("d_vector.py:271-294", ":274", ":278", ":281-284", ":289-290"):
        assert cite in hdr, cite
    src = open(os.path.join(ROOT, "speech_signal_processing_amd", "csrc", "lstm_train.hip")).read()
    assert "d_vector.py:271-294" in src
    from speech_signal_processing_amd import build
    assert "lstm_train.hip" in build.SOURCES
    assert re.findall(r"atomic\w*\s*\(", src) == []   # no atomic call at all, a float one least of all


def test_refusals_need_no_device():
    """every limit of ssp_lstm_trainer_create is answered before the context is touched: a null context reaches none of them"""
    from speech_signal_processing_amd import _lib as L
    lib = L.load()
    W, U, Wd = np.zeros((13, 64), np.float32), np.zeros((16, 64), np.float32), np.zeros((16, 3), np.float32)
    h = ctypes.c_void_p()

    def create(d_in=13, units=16, n_class=3, T=5, act=0, w=W, u=U, wd=Wd, mb=8):
        return lib.ssp_lstm_trainer_create(None, d_in, units, n_class, T, act, None if w is None else w.ctypes.data,
                                           None if u is None else u.ctypes.data, None, None if wd is None else wd.ctypes.data, None, mb, ctypes.byref(h))
    for kw in (dict(units=24), dict(units=144), dict(d_in=65), dict(T=0), dict(T=1025), dict(n_class=1), dict(n_class=4097), dict(mb=0), dict(mb=1025)):
        assert create(**kw) == L.SSP_ERR_UNSUPPORTED and not h.value, kw
    for kw in (dict(w=None), dict(u=None), dict(wd=None), dict(act=2), dict(act=-1)):
        assert create(**kw) == L.SSP_ERR_INVALID and not h.value, kw
    assert create() == L.SSP_ERR_INVALID      # everything in range: only the null context is left to object to
