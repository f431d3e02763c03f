"""Host tests of the conv + GRU trainer's restatement (tests/gru_train_oracle.py): its gradients of every tensor against torch.autograd in
float64 on a network composed from torch ops (torch.nn.GRU is the reset_after cell and is not used; hard_sigmoid is a clamp), central
differences, the eps branch of the l2_normalize backward, the properties of the initialisation, and that the header, the bindings and the
build declare the new entry points.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_oracle as GO  # noqa: E402
import gru_train_oracle as TO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(seed, T=7, D=5, F=4, H=16, n_gru=2, E=8, C=5, B=6, kernel=(5, 5), strides=(2, 2), bias=True, scale_dense=1.0):
    rng = np.random.default_rng(seed)
    p = TO.keras_init(rng, T, D, F, H, n_gru, E, C, kernel, strides)
    p["dense_W"] = (p["dense_W"] * scale_dense).astype(np.float32)
    for k in list(p):
        if k.endswith("_b"):
            p[k] = (0.1 * rng.standard_normal(p[k].shape)).astype(np.float32) if bias else None
    X = (2.0 * rng.standard_normal((B, T, D))).astype(np.float32)
    y = rng.integers(0, C, B)
    return p, X, y


def _torch_grads(p, X, y, strides, act):
    """mean cross-entropy + 0.01 sum K^2 of the network composed from torch ops, float64 -> {name: gradient}"""
    import torch
    import torch.nn.functional as Fn
    tp = {k: None if v is None else torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    x = torch.tensor(np.asarray(X, np.float64))
    K = tp["conv_K"]
    kh, kw, _, F = K.shape
    B, T, D = x.shape
    To, pt, pb = GO.same_padding(T, kh, strides[0])
    Do, pl, pr = GO.same_padding(D, kw, strides[1])
    h = Fn.conv2d(Fn.pad(x[:, None], (pl, pr, pt, pb)), K.permute(3, 2, 0, 1), tp["conv_b"], stride=strides)
    h = h.permute(0, 2, 3, 1).reshape(B, To, Do * F)

    def s(a):
        return torch.sigmoid(a) if act == "sigmoid" else torch.clamp(0.2 * a + 0.5, 0.0, 1.0)
    n_gru = len([k for k in p if k.endswith("_U")])
    for i in range(n_gru):
        W, U, b = tp["gru%d_W" % i], tp["gru%d_U" % i], tp["gru%d_b" % i]
        H = U.shape[0]
        P = h @ W if b is None else h @ W + b
        st = torch.zeros(B, H, dtype=torch.float64)
        outs = []
        for t in range(To):
            z = s(P[:, t, :H] + st @ U[:, :H])
            r = s(P[:, t, H:2 * H] + st @ U[:, H:2 * H])
            hh = torch.tanh(P[:, t, 2 * H:] + (r * st) @ U[:, 2 * H:])
            st = z * st + (1 - z) * hh
            outs.append(st)
        h = torch.stack(outs, dim=1)
    e = h.mean(dim=1) @ tp["dense_W"]
    if tp["dense_b"] is not None:
        e = e + tp["dense_b"]
    yv = e / torch.sqrt(torch.clamp((e * e).sum(dim=1, keepdim=True), min=TO.L2_EPS))
    logits = yv @ tp["head_W"]
    if tp["head_b"] is not None:
        logits = logits + tp["head_b"]
    loss = Fn.cross_entropy(logits, torch.tensor(np.asarray(y, np.int64))) + TO.LAMBDA * (K * K).sum()
    loss.backward()
    return {k: None if v is None else v.grad.numpy() for k, v in tp.items()}, float(loss.detach())


def _oracle_grads(p, X, y, strides, act):
    net = TO.Net(p, strides, act)
    logits, st = net.forward(X)
    loss, _, g = net.loss(logits, y)
    return net.backward(st, g), loss / len(y), st


@pytest.mark.parametrize("n_gru", [1, 2])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("act", GO.ACTIVATIONS)
def test_gradients_against_autograd(act, bias, n_gru):
    p, X, y = _make(3 + n_gru, n_gru=n_gru, bias=bias)
    ref, loss_t = _torch_grads(p, X, y, (2, 2), act)
    got, loss_o, _ = _oracle_grads(p, X, y, (2, 2), act)
    assert abs(loss_o - loss_t) <= 1e-12 * max(1.0, abs(loss_t))
    for k, r in ref.items():
        if r is None:
            assert got[k] is None
            continue
        assert np.abs(r).max() > 0, k
        gap = np.abs(got[k] - r).max() / np.abs(r).max()
        assert gap <= 1e-9, (k, gap)


def test_gradients_against_autograd_stride_1_and_3x3():
    p, X, y = _make(9, T=6, D=5, kernel=(3, 3), strides=(1, 1), n_gru=1)
    ref, _ = _torch_grads(p, X, y, (1, 1), "sigmoid")
    got, _, _ = _oracle_grads(p, X, y, (1, 1), "sigmoid")
    for k, r in ref.items():
        assert np.abs(got[k] - r).max() <= 1e-9 * np.abs(r).max(), k


def test_central_differences_on_sigmoid_gates():
    p, X, y = _make(11)
    got, _, _ = _oracle_grads(p, X, y, (2, 2), "sigmoid")
    rng = np.random.default_rng(0)

    def loss_of(q):
        net = TO.Net(q, (2, 2), "sigmoid")
        return net.loss(net.forward(X)[0], y)[0] / len(y)
    for k in p:
        flat = np.asarray(p[k], np.float64).reshape(-1)
        scale = np.abs(got[k]).max()
        for j in rng.choice(flat.size, size=min(3, flat.size), replace=False):
            vals = []
            for sgn in (1.0, -1.0):
                q = {n: np.asarray(v, np.float64).copy() for n, v in p.items()}
                q[k].reshape(-1)[j] += sgn * 1e-5
                vals.append(loss_of(q))
            num = (vals[0] - vals[1]) / 2e-5
            assert abs(num - got[k].reshape(-1)[j]) <= 1e-6 * max(scale, 1e-3), (k, j, num, got[k].reshape(-1)[j])


def test_l2_normalize_backward_below_eps():
    """embeddings whose squared norm lies below 1e-12 are divided by sqrt(eps): the gradient passes straight through, dx = dy / n"""
    p, X, y = _make(13, bias=False, scale_dense=1e-8)
    got, _, st = _oracle_grads(p, X, y, (2, 2), "sigmoid")
    assert st["ss"].max() < TO.L2_EPS
    assert np.all(st["n"] == np.sqrt(TO.L2_EPS))
    ref, _ = _torch_grads(p, X, y, (2, 2), "sigmoid")
    for k, r in ref.items():
        if r is not None:
            assert np.abs(got[k] - r).max() <= 1e-9 * np.abs(r).max(), k
    # and the branch itself: dense_W's gradient is mean^T (dy / n)
    net = TO.Net(p, (2, 2), "sigmoid")
    logits, st = net.forward(X)
    _, _, g = net.loss(logits, y)
    dy = g @ net.p["head_W"].T
    assert np.allclose(got["dense_W"], st["mean"].T @ (dy / np.sqrt(TO.L2_EPS)), rtol=1e-12, atol=0)


def test_initialisation_properties():
    T, D, F, H, E, C = 12, 13, 4, 32, 16, 4
    p = TO.keras_init(np.random.default_rng(5), T, D, F, H, 2, E, C)
    assert p["conv_K"].shape == (5, 5, 1, F) and np.abs(p["conv_K"]).max() <= np.sqrt(6.0 / (25 + 25 * F))
    d0 = 7 * F
    for i, d_in in enumerate((d0, H)):
        W, U, b = p["gru%d_W" % i], p["gru%d_U" % i], p["gru%d_b" % i]
        assert W.shape == (d_in, 3 * H) and U.shape == (H, 3 * H) and not b.any()
        assert np.abs(W).max() <= np.sqrt(6.0 / (d_in + 3 * H)) and np.abs(W).max() > 0.5 * np.sqrt(6.0 / (d_in + 3 * H))
        assert np.abs(U.astype(np.float64) @ U.astype(np.float64).T - np.eye(H)).max() < 1e-5     # orthonormal rows
    assert np.abs(p["dense_W"]).max() <= np.sqrt(6.0 / (H + E)) and np.abs(p["head_W"]).max() <= np.sqrt(6.0 / (E + C))
    assert all(p[k].dtype == np.float32 for k in p) and not p["conv_b"].any() and not p["dense_b"].any() and not p["head_b"].any()
    # the same seed draws the same tensors; the draws come in the documented order (the conv kernel first)
    q = TO.keras_init(np.random.default_rng(5), T, D, F, H, 2, E, C)
    assert all(np.array_equal(p[k], q[k]) for k in p)
    lim = np.sqrt(6.0 / (25 + 25 * F))
    assert np.array_equal(p["conv_K"], np.random.default_rng(5).uniform(-lim, lim, (5, 5, 1, F)).astype(np.float32))


ENTRY_POINTS = ("ssp_gru_trainer_create", "ssp_gru_trainer_destroy", "ssp_gru_trainer_epoch", "ssp_gru_trainer_evaluate", "ssp_gru_trainer_read",
                "ssp_gru_trainer_steps", "ssp_gru_trainer_step_times")


def test_header_bindings_and_sources_declare_the_trainer():
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    from speech_signal_processing_amd import _lib, api, build, d_vector
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "gru_train.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "speech_signal_processing_amd", "csrc", "gru_train.hip"))
    for word in ("regulariser", "reset_after = 1", "SSP_ERR_UNSUPPORTED", "Unpinned"):
        assert word in header[header.index("conv + GRU d-vector network training"):], word
    assert hasattr(api, "GruTrainer") and hasattr(d_vector.nn_model, "inference_gru")
    import inspect
    sig = inspect.signature(d_vector.nn_model.inference_gru)
    assert list(sig.parameters)[:5] == ["self", "X_train", "Y_train", "X_val", "Y_val"]
    want = dict(epochs=50, batch_size=128, lr=1e-4, seed=0, recurrent_activation="hard_sigmoid", reset_after=False, filters=64, units=1024, n_gru=3,
                embedding=512, model_dir=None)
    for k, v in want.items():
        assert sig.parameters[k].default == v and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k


def test_create_refuses_before_any_gpu_work():
    """every limit of ssp_gru_trainer_create, and reset_after = 1 with either bias layout, is answered before the context is touched: a
    context that holds no device gets the refusal, NotImplementedError for what is unsupported and ValueError for what is malformed"""
    import types
    from speech_signal_processing_amd import _lib, api
    ctx = types.SimpleNamespace(_lib=_lib.load(), _h=None)
    T, D, F, H, E, C = 7, 5, 4, 48, 24, 5                  # 5 x 5, strides 2: To 4, Do 3, 12 features
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    conv, g, dense, head = (z(5, 5, 1, F), z(F), (2, 2)), (z(12, 3 * H), z(H, 3 * H), z(3 * H)), (z(H, E), z(E)), (z(E, C), z(C))

    def make(conv=conv, grus=(g,), dense=dense, head=head, **kw):
        args = dict(T=T, D=D, recurrent_activation="sigmoid", reset_after=False, max_batch=16)
        args.update(kw)
        return api.GruTrainer(ctx, conv, list(grus), dense, head, **args)
    for kw in (dict(recurrent_activation="relu"), dict(reset_after=1), dict(grus=[g[:2] + (z(2, 3 * H),)]), dict(grus=[(z(11, 3 * H),) + g[1:]])):
        with pytest.raises(ValueError):
            make(**kw)
    unsupported = (dict(reset_after=True), dict(reset_after=True, grus=[g[:2] + (z(2, 3 * H),)]), dict(reset_after=True, grus=[g[:2] + (None,)]),
                   dict(T=0), dict(T=1025), dict(max_batch=0), dict(max_batch=1025),
                   dict(conv=(z(8, 5, 1, F), None, (2, 2))), dict(conv=(z(5, 8, 1, F), None, (2, 2))),
                   dict(conv=(z(5, 5, 1, 257), None, (2, 2)), grus=[(z(3 * 257, 3 * H),) + g[1:]]),
                   dict(conv=(z(5, 5, 1, F), None, (3, 3)), grus=[(z(8, 3 * H),) + g[1:]]),
                   dict(grus=[g] + [(z(H, 3 * H), z(H, 3 * H), None)] * 4),
                   dict(grus=[(z(12, 72), z(24, 72), None)], dense=(z(24, E), None)),
                   dict(grus=[(z(12, 3 * 1040), z(1040, 3 * 1040), None)], dense=(z(1040, E), None)),
                   dict(head=(z(E, 1), None)), dict(head=(z(E, 4097), None)),
                   dict(grus=[(z(12, 3072), z(1024, 3072), None)], dense=(z(1024, E), None), T=1024, max_batch=1024))   # 24 GiB of workspace
    for kw in unsupported:
        with pytest.raises(NotImplementedError):
            make(**kw)
