"""CPU-side tests of the dense d-vector network's training: the float64 restatement (tests/dnn_train_oracle.py) against torch.autograd,
finite differences and hand-computed Adam / plateau tables; the library's surface; and the dropout generator, which runs without a device.
(Unpinned against Keras: the reference tree holds no weights or logs of this network and Keras is not a dependency.)"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dnn_train_oracle as DO  # noqa: E402

NEW = ("ssp_dnn_trainer_create", "ssp_dnn_trainer_destroy", "ssp_dnn_trainer_epoch", "ssp_dnn_trainer_evaluate", "ssp_dnn_trainer_read",
       "ssp_dnn_trainer_steps", "ssp_dropout_keep")
DIMS = (37, 50, 33, 16, 5)
RATES = (0.5, 0.2, 0.5, 0.0)


def _small_net(rng, dims=DIMS, rates=RATES, dtype=np.float64):
    L = len(dims) - 1
    layers = []
    for l in range(L):
        W = rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])
        layers.append((W, 0.1 * rng.standard_normal(dims[l + 1]), l < L - 1, rates[l]))
    return DO.Net(layers, dtype)


def _lib():
    from speech_signal_processing_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)   # (no torch, no device: the generator is host code)
    res, args = L.SIGNATURES["ssp_dropout_keep"]
    lib.ssp_dropout_keep.restype, lib.ssp_dropout_keep.argtypes = res, args
    return lib


def _keep(lib, seed, step, layer, rows, width, rate):
    out = np.empty((rows, width), np.uint8)
    rc = lib.ssp_dropout_keep(seed, step, layer, rows, width, rate, out.ctypes.data)
    assert rc == 0, rc
    return out.astype(bool)


def test_oracle_gradients_match_torch_autograd_float64():
    import torch
    rng = np.random.default_rng(11)
    net = _small_net(rng)
    B = 19
    X = rng.standard_normal((B, DIMS[0]))
    y = rng.integers(0, DIMS[-1], B)
    masks = net.masks(5, 3, B)
    xs, ys = net.forward(X, masks)
    loss, _, g = net.loss(ys[-1], y)
    dW, db = net.backward(xs, ys, masks, g)
    Wt = [torch.tensor(W, requires_grad=True) for W in net.W]
    bt = [torch.tensor(b, requires_grad=True) for b in net.b]
    h = torch.from_numpy(X)
    for l in range(net.L):
        h = h @ Wt[l] + bt[l]
        if net.relu[l]:
            h = torch.relu(h)
        if masks[l] is not None:
            h = h * torch.from_numpy(masks[l].astype(np.float64)) / (1.0 - net.rate[l])
    tl = torch.nn.functional.cross_entropy(h, torch.from_numpy(y), reduction="mean")
    tl.backward()
    assert abs(loss / B - tl.item()) <= 1e-12 * max(1.0, abs(tl.item()))
    worst = 0.0
    for l in range(net.L):
        for got, ref in ((dW[l], Wt[l].grad.numpy()), (db[l], bt[l].grad.numpy())):
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print("oracle vs torch.autograd float64: %.3e relative" % worst)
    assert worst <= 1e-10


def test_oracle_gradients_match_central_differences():
    rng = np.random.default_rng(12)
    net = _small_net(rng)
    B = 19
    X = rng.standard_normal((B, DIMS[0]))
    y = rng.integers(0, DIMS[-1], B)
    masks = net.masks(1, 0, B)

    def mean_loss():
        return net.loss(net.forward(X, masks)[1][-1], y)[0] / B

    xs, ys = net.forward(X, masks)
    dW, db = net.backward(xs, ys, masks, net.loss(ys[-1], y)[2])
    h = 1e-6
    for _ in range(20):
        l = int(rng.integers(0, net.L))
        P, G = (net.W[l], dW[l]) if rng.random() < 0.7 else (net.b[l], db[l])
        i = tuple(int(rng.integers(0, n)) for n in P.shape)
        keep = P[i]
        P[i] = keep + h
        up = mean_loss()
        P[i] = keep - h
        dn = mean_loss()
        P[i] = keep
        assert abs((up - dn) / (2 * h) - G[i]) <= 1e-6 * max(1.0, abs(G[i])) + 1e-8, (l, i)


def test_oracle_adam_three_steps_by_hand():
    """one parameter, gradients 0.5, -0.25, 0.0 at lr 0.1: Keras 2's update with eps OUTSIDE the root and t's bias correction"""
    net = DO.Net([(np.array([[1.0]]), None, False, 0.0)])
    p, m, v = 1.0, 0.0, 0.0
    for t, g in enumerate((0.5, -0.25, 0.0), start=1):
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        lr_t = 0.1 * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t)
        p = p - lr_t * m / (v ** 0.5 + 1e-7)
        net.dW, net.db = [np.array([[g]])], [None]
        net.adam(0.1)
        assert net.t == t
        assert abs(net.W[0][0, 0] - p) <= 1e-15 and abs(net.mW[0][0, 0] - m) <= 1e-15 and abs(net.vW[0][0, 0] - v) <= 1e-15
    # the first step written out: m = 0.05, v = 2.5e-4, lr_1 = 0.1 sqrt(0.001) / 0.1 -> p = 1 - sqrt(0.001) 0.05 / (sqrt(2.5e-4) + 1e-7)
    first = 1.0 - 0.001 ** 0.5 * 0.05 / (0.00025 ** 0.5 + 1e-7)
    net = DO.Net([(np.array([[1.0]]), None, False, 0.0)])
    net.dW, net.db = [np.array([[0.5]])], [None]
    net.adam(0.1)
    assert abs(net.W[0][0, 0] - first) <= 1e-15
    # eps inside the root (torch's form divided through) would give a different number at a tiny gradient
    g = 1e-7
    net = DO.Net([(np.array([[1.0]]), None, False, 0.0)])
    net.dW, net.db = [np.array([[g]])], [None]
    net.adam(0.1)
    lr1 = 0.1 * 0.001 ** 0.5 / 0.1
    assert abs(net.W[0][0, 0] - (1.0 - lr1 * 0.1 * g / ((0.001 * g * g) ** 0.5 + 1e-7))) <= 1e-15
    assert abs(net.W[0][0, 0] - (1.0 - 0.1 * g / (g + 1e-8))) > 1e-3     # torch.optim.Adam's answer (eps 1e-8 on sqrt(v_hat))


def test_oracle_plateau_schedule_by_hand():
    """val_loss -> the lr of the NEXT epoch; patience 2, factor 0.5, min_delta 1e-4, min_lr 1e-7"""
    table = [                      # val_loss, lr after the epoch, why
        (1.00000, 1e-4),           # first value: an improvement
        (0.99995, 1e-4),           # better by 5e-5 < min_delta: no improvement, wait = 1
        (0.99991, 5e-5),           # best is still 1.0 and 9e-5 < min_delta; wait = 2 -> reduced, wait = 0
        (1.10000, 5e-5),           # wait = 1
        (1.20000, 2.5e-5),         # wait = 2 -> reduced again: two reductions in a row, no improvement between them
        (0.50000, 2.5e-5),         # improvement: best = 0.5, wait = 0
        (0.60000, 2.5e-5),
        (0.60000, 1.25e-5),
    ]
    s = DO.ReduceLROnPlateau()
    lr = 1e-4
    for i, (vl, want) in enumerate(table):
        lr = s.update(vl, lr)
        assert lr == pytest.approx(want, rel=1e-12), (i, lr, want)
    # the floor: from 1.5e-7 one reduction lands on min_lr, and there it stays
    s = DO.ReduceLROnPlateau()
    lr = 1.5e-7
    seen = []
    for vl in (1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0):
        lr = s.update(vl, lr)
        seen.append(lr)
    assert seen == [1.5e-7, 1.5e-7, 1e-7, 1e-7, 1e-7, 1e-7, 1e-7]


def test_oracle_csv_rows():
    rows = DO.csv_rows({"acc": [0.25, 0.5], "loss": [2.0, 1.5], "lr": [1e-4, 5e-5], "val_acc": [0.125, 0.25], "val_loss": [2.5, 2.25]})
    assert rows[0] == "epoch,acc,loss,lr,val_acc,val_loss"
    assert rows[1] == "0,0.25,2.0,0.0001,0.125,2.5" and rows[2] == "1,0.5,1.5,5e-05,0.25,2.25"


def test_header_and_bindings_declare_the_trainer():
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
    # the entries cite the reference lines they replace
    for cite in ("d_vector.py:168-206", "d_vector.py:205-206", ":198-203", ":171-194"):
        assert cite in hdr, cite
    src = open(os.path.join(ROOT, "speech_signal_processing_amd", "csrc", "dnn_train.hip")).read()
    assert "d_vector.py:168-206" in src
    from speech_signal_processing_amd import build
    assert "dnn_train.hip" in build.SOURCES
    # no floating-point atomic in any reduction of the new file
    assert re.findall(r"atomicAdd\(([^,]+),", src) == ["a.ticket"]   # the one atomic is the integer ticket


def test_dropout_generator_equals_the_restatement_bit_for_bit():
    lib = _lib()
    cases = [(0, 0, 0, 19, 50, 0.5), (7, 3, 2, 128, 256, 0.5), (2 ** 40 + 5, 2 ** 33 + 1, 4, 3, 16, 0.2), (123456789, 468, 3, 44, 1251, 0.2),
             (2 ** 64 - 1, 10 ** 12, 63, 1, 13, 0.75), (1, 1, 1, 1024, 7, 0.1), (9, 9, 0, 2, 4096, 0.5)]
    for seed, step, layer, rows, width, rate in cases:
        got = _keep(lib, seed, step, layer, rows, width, rate)
        assert np.array_equal(got, DO.dropout_keep(seed, step, layer, rows, width, rate)), (seed, step, layer, rows, width, rate)
    assert _keep(lib, 3, 4, 1, 128, 256, 0.0).all()          # rate 0 keeps everything
    out = np.empty(4, np.uint8)
    assert lib.ssp_dropout_keep(0, 0, 0, 2, 2, 1.0, out.ctypes.data) == -1       # rate outside [0, 1)
    assert lib.ssp_dropout_keep(0, 0, 0, 2, 2, -0.1, out.ctypes.data) == -1
    assert lib.ssp_dropout_keep(0, 0, 0, 2, 4097, 0.5, out.ctypes.data) == -2    # beyond the widths the trainer covers
    assert lib.ssp_dropout_keep(0, 0, 0, 1025, 2, 0.5, out.ctypes.data) == -2


@pytest.mark.parametrize("rate", [0.5, 0.2])
def test_dropout_generator_statistics(rate):
    """10^6 draws per mask: the kept share within 4 binomial standard deviations of 1 - rate, and masks of two steps, two layers and two
    seeds agree on rate^2 + (1 - rate)^2 of the elements within 4 standard deviations (independence)"""
    lib = _lib()
    rows, width = 1000, 1000
    n = rows * width
    base = _keep(lib, 17, 5, 2, rows, width, rate)
    sd = np.sqrt(rate * (1 - rate) / n)
    share = base.mean()
    print("rate %.1f: kept share %.6f" % (rate, share))
    assert abs(share - (1 - rate)) <= 4 * sd
    q = rate * rate + (1 - rate) * (1 - rate)
    sdq = np.sqrt(q * (1 - q) / n)
    for name, other in (("step", _keep(lib, 17, 6, 2, rows, width, rate)), ("layer", _keep(lib, 17, 5, 3, rows, width, rate)),
                        ("seed", _keep(lib, 18, 5, 2, rows, width, rate))):
        agree = (base == other).mean()
        print("rate %.1f: agreement with another %s %.6f (independent: %.6f)" % (rate, name, agree, q))
        assert abs(agree - q) <= 4 * sdq, name
        assert abs(other.mean() - (1 - rate)) <= 4 * sd, name
