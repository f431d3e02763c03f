"""GPU tests of the dense d-vector network's training (csrc/dnn_train.hip, api.DnnTrainer, d_vector.nn_model.inference) against the
float64 restatement tests/dnn_train_oracle.py.  Unpinned against Keras (see the oracle).

The limits are scale-free.  Gradients, and Adam's m and v: per tensor max|gpu - ref| <= 1e-4 max|ref|.  Loss sums: 1e-4 max(1, |ref|).
Correct counts: exact.  Weights after a dozen steps at lr = 1e-4: max|gpu - ref| <= 0.05 lr — one step with the wrong sign moves a
parameter by up to 2 lr.  Each case first asserts on the CPU, on its very inputs, that single precision alone stays well inside these
limits (the float32 restatement within 1e-5 max|ref| of float64 on the gradients, within 0.01 lr on the weights) and that no row's
label sits within 1e-3 of the best other logit: a case that fails a precondition gets another seed, never another limit."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dnn_train_oracle as DO  # noqa: E402
import skewed  # noqa: E402
import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

LR = float(np.float32(1e-4))
REF = (1274, 256, 256, 256, 256)
REF_RATES = (0.0, 0.0, 0.5, 0.5, 0.0)
ODD = (37, 50, 33, 16, 5)
ODD_RATES = (0.5, 0.2, 0.5, 0.0)
TINY = (13, 16, 16, 3)
TINY_RATES = (0.2, 0.5, 0.0)
# name -> dims, dropout rates, layers without bias, rows, batch size, epoch calls (every call runs ceil(rows / batch) steps), seed
CASES = {
    "reference-40": (REF + (40,), REF_RATES, (), 128, 128, 12, 1),
    "reference-1251": (REF + (1251,), REF_RATES, (), 128, 128, 6, 2),
    "odd-batch19": (ODD, ODD_RATES, (), 19, 19, 12, 3),
    "tiny-batch1": (TINY, TINY_RATES, (), 1, 1, 12, 4),
    "tiny-batch3": (TINY, TINY_RATES, (), 3, 3, 12, 5),
    "reference-tail44": (REF + (40,), REF_RATES, (), 300, 128, 4, 6),
    "odd-no-bias": (ODD, ODD_RATES, (1, 2), 19, 19, 12, 7),
    "odd-no-dropout": (ODD, (0.0, 0.0, 0.0, 0.0), (), 19, 19, 12, 8),
}
_CACHE = {}


def _api():
    from speech_signal_processing_amd import api
    return api


def _make(dims, rates, no_bias, N, seed):
    rng = np.random.default_rng(1000 + seed)
    L = len(dims) - 1
    layers = []
    for l, (W, _) in enumerate(DO.glorot_uniform(rng, dims)):
        b = None if l in no_bias else (0.05 * rng.standard_normal(dims[l + 1])).astype(np.float32)
        layers.append((W, b, l < L - 1, rates[l]))
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    y = rng.integers(0, dims[-1], N).astype(np.int32)
    return layers, X, y


def _snapshot(net):
    return {"W": [w.copy() for w in net.W], "b": [None if b is None else b.copy() for b in net.b],
            "dW": [g.copy() for g in net.dW], "db": [None if g is None else g.copy() for g in net.db],
            "mW": [m.copy() for m in net.mW], "mb": [None if m is None else m.copy() for m in net.mb],
            "vW": [v.copy() for v in net.vW], "vb": [None if v is None else v.copy() for v in net.vb]}


def _gap(a, b, keys):
    """largest max|a - b| / max|b| over the tensors of ``keys``"""
    worst = 0.0
    for k in keys:
        for x, r in zip(a[k], b[k]):
            if r is not None:
                worst = max(worst, float(np.abs(np.asarray(x, np.float64) - r).max() / max(np.abs(r).max(), 1e-300)))
    return worst


def _reference(name):
    """the case's inputs and its float64 run (after the first call and after the last), computed once; the preconditions are asserted here"""
    if name in _CACHE:
        return _CACHE[name]
    dims, rates, no_bias, N, B, calls, seed = CASES[name]
    layers, X, y = _make(dims, rates, no_bias, N, seed)
    keep = _api().dropout_keep       # the masks come from the library's own generator (ssp_dropout_keep, host code)
    out = {}
    for dt in (np.float64, np.float32):
        net = DO.Net(layers, dt)
        net.keep_fn = keep
        first = None
        for c in range(calls):
            res = net.epoch(X, y, None, B, LR, seed)
            if c == 0:
                first = (res, _snapshot(net))
        out[dt] = (first, _snapshot(net), net)
    (res64, one64), end64, net64 = out[np.float64]
    (_, one32), end32, _ = out[np.float32]
    drift_g = _gap(one32, one64, ("dW", "db", "mW", "mb", "vW", "vb"))
    drift_w = max(float(np.abs(a.astype(np.float64) - r).max()) for k in ("W", "b") for a, r in zip(end32[k], end64[k]) if r is not None) / LR
    print("[precondition] %s: float32 gradients within %.2e max|ref|, weights after %d steps within %.4f lr, margin %.2e" % (
        name, drift_g, net64.t, drift_w, net64.min_margin))
    assert drift_g <= 1e-5, "precondition: change the case's seed"
    assert drift_w <= 0.01, "precondition: change the case's seed"
    assert net64.min_margin > 1e-3, "precondition: change the case's seed"
    _CACHE[name] = (layers, X, y, res64, one64, end64, net64.t)
    return _CACHE[name]


def _read_all(tr):
    L = len(tr.dims) - 1
    snap = {}
    for k in ("W", "dW", "mW", "vW"):
        snap[k] = [tr.read(k, l) for l in range(L)]
    for k in ("b", "db", "mb", "vb"):
        snap[k] = [tr.read(k, l) if tr.has_bias[l] else None for l in range(L)]
    return snap


def _same_bits(a, b, keys=("W", "b")):
    for k in keys:
        for l, (x, r) in enumerate(zip(a[k], b[k])):
            assert (x is None) == (r is None)
            if x is not None:
                assert np.array_equal(x, r), "%s of layer %d differs on %d elements" % (k, l, int((x != r).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_step_gradients_loss_and_weights(name):
    dims, rates, no_bias, N, B, calls, seed = CASES[name]
    layers, X, y, (loss64, corr64), one64, end64, t64 = _reference(name)
    api = _api()
    tr = api.DnnTrainer(api.default_context(), layers, max_batch=max(B, 2))
    loss, corr = tr.epoch(X, y, None, batch_size=B, lr=LR, seed=seed)
    one = _read_all(tr)
    print("[measured] %s: loss sum %.6f (ref %.6f), correct %d (ref %d)" % (name, loss, loss64, corr, corr64))
    for k in ("dW", "db", "mW", "mb", "vW", "vb"):
        g = _gap(one, one64, (k,))
        print("[measured] %s: %s max|gpu - ref| / max|ref| = %.3e" % (name, k, g))
        assert g <= 1e-4, k
    assert abs(loss - loss64) <= 1e-4 * max(1.0, abs(loss64))
    assert corr == corr64
    for l in no_bias:
        with pytest.raises(ValueError):
            tr.read("b", l)
    for _ in range(calls - 1):
        tr.epoch(X, y, None, batch_size=B, lr=LR, seed=seed)
    assert tr.steps == t64
    end = _read_all(tr)
    worst = max(float(np.abs(a.astype(np.float64) - r).max()) for k in ("W", "b") for a, r in zip(end[k], end64[k]) if r is not None) / LR
    print("[measured] %s: weights after %d steps max|gpu - ref| = %.4f lr" % (name, t64, worst))
    assert worst <= 0.05
    for k in ("mW", "mb", "vW", "vb"):
        assert _gap(end, end64, (k,)) <= 1e-4, k
    tr.close()


def _odd(seed=3, N=100):
    return _make(ODD, ODD_RATES, (), N, seed)


def test_an_epoch_equals_its_steps():
    """one call over an order = the same batches gathered beforehand and issued one per call: the same bits, t continues across calls"""
    api = _api()
    layers, X, y = _odd(N=100)
    order = np.random.default_rng(5).permutation(100)
    a = api.DnnTrainer(api.default_context(), layers, max_batch=19)
    b = api.DnnTrainer(api.default_context(), layers, max_batch=19)
    la, ca = a.epoch(X, y, order, batch_size=19, lr=LR, seed=9)
    lb, cb = 0.0, 0
    for r0 in range(0, 100, 19):       # (the last batch has 5 rows)
        rows = order[r0:r0 + 19]
        l1, c1 = b.epoch(X[rows], y[rows], None, batch_size=19, lr=LR, seed=9)
        lb, cb = lb + l1, cb + c1
    assert a.steps == b.steps == 6
    assert la == lb and ca == cb
    _same_bits(_read_all(a), _read_all(b), ("W", "b", "dW", "db", "mW", "mb", "vW", "vb"))
    # and against the oracle run over the same order
    net = DO.Net(layers)
    lo, co = net.epoch(X, y, order, 19, LR, 9)
    assert abs(la - lo) <= 1e-4 * max(1.0, abs(lo)) and net.min_margin > 1e-3 and ca == co


def test_determinism_and_seed():
    api = _api()
    layers, X, y = _make(REF + (40,), REF_RATES, (), 256, 11)
    runs = []
    for seed in (4, 4, 5):
        tr = api.DnnTrainer(api.default_context(), layers, max_batch=128)
        for _ in range(10):             # 20 steps
            tr.epoch(X, y, None, batch_size=128, lr=LR, seed=seed)
        assert tr.steps == 20
        runs.append(_read_all(tr))
        tr.close()
    _same_bits(runs[0], runs[1], ("W", "b", "mW", "mb", "vW", "vb"))
    assert any(not np.array_equal(a, b) for a, b in zip(runs[0]["W"], runs[2]["W"]))   # the dropout seed matters


def test_evaluate_against_the_oracle_and_changes_nothing():
    api = _api()
    layers, X, y = _make(REF + (40,), REF_RATES, (), 300, 12)
    tr = api.DnnTrainer(api.default_context(), layers, max_batch=128)
    tr.epoch(X, y, None, batch_size=128, lr=LR, seed=1)
    before = _read_all(tr)
    t = tr.steps
    loss, corr = tr.evaluate(X, y)       # three chunks of the trainer's max_batch, the last of 44 rows
    after = _read_all(tr)
    assert tr.steps == t == 3
    _same_bits(before, after, ("W", "b", "dW", "db", "mW", "mb", "vW", "vb"))
    net = DO.Net([(before["W"][l], before["b"][l], layers[l][2], layers[l][3]) for l in range(len(layers))])   # the GPU's weights
    lo, co = net.evaluate(X, y)
    print("[measured] evaluate: loss sum %.6f (ref %.6f), correct %d (ref %d), margin %.2e" % (loss, lo, corr, co, net.min_margin))
    assert net.min_margin > 1e-3, "precondition: change the seed"
    assert abs(loss - lo) <= 1e-4 * max(1.0, abs(lo)) and corr == co
    # dropout is off: a second pass gives the same bits
    assert tr.evaluate(X, y) == (loss, corr)


def test_host_arrays_equal_device_tensors():
    import torch
    api = _api()
    layers, X, y = _odd(N=100)
    order = np.random.default_rng(6).permutation(100)
    a = api.DnnTrainer(api.default_context(), layers, max_batch=32)
    b = api.DnnTrainer(api.default_context(), layers, max_batch=32)
    ra = a.epoch(X, y, order, batch_size=32, lr=LR, seed=2)
    rb = b.epoch(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), order, batch_size=32, lr=LR, seed=2)
    assert ra == rb
    _same_bits(_read_all(a), _read_all(b), ("W", "b", "dW", "db", "mW", "mb", "vW", "vb"))
    assert a.evaluate(X, y) == b.evaluate(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())


@pytest.mark.parametrize("name", ["odd", "reference"])
def test_device_arrays_off_16_byte_alignment(name):
    """X and labels 4 bytes past a 16-byte line give the bits of aligned ones (rows of 37 and of 1274 floats), and nothing around them
    is read into the result (NaN guards) or written"""
    api = _api()
    layers, X, y = _odd(N=100) if name == "odd" else _make(REF + (40,), REF_RATES, (), 150, 13)
    N = len(y)
    order = np.random.default_rng(7).permutation(N)
    got = []
    for skew in (0, 4):
        xv, xg = skewed.view(X.size, "float32", skew, fill=X)
        yv, yg = skewed.view(N, "int32", skew, fill=y)
        tr = api.DnnTrainer(api.default_context(), layers, max_batch=64)
        res = tr.epoch(xv.view(N, -1), yv, order, batch_size=64, lr=LR, seed=3)
        ev = tr.evaluate(xv.view(N, -1), yv)
        got.append((res, ev, _read_all(tr)))
        skewed.check_guards(xg, "X skew %d" % skew)
        skewed.check_guards(yg, "labels skew %d" % skew)
        assert np.isfinite(res[0]) and np.isfinite(ev[0])
        tr.close()
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1]
    _same_bits(got[0][2], got[1][2], ("W", "b", "dW", "db", "mW", "mb", "vW", "vb"))


@pytest.mark.parametrize("mode", SO.MODES)
def test_stream_order(mode):
    """X and labels produced on another torch stream just before the call: the epoch and the evaluation see them"""
    cfg = SO.Config(mode)
    try:
        layers, X, y = _odd(N=100)
        C = ODD[-1]

        # fresh trainers made ahead (allocations, the upload and its host wait), so that nothing but the epoch and the evaluation sits
        # between the producer and the reads of X and labels; the harness calls once for the baseline and once per racing run
        pool = [cfg.api.DnnTrainer(cfg.ctx, layers, max_batch=32) for _ in range(8)]

        def call(dv, _):
            tr = pool.pop()
            loss, corr = tr.epoch(dv["X"], dv["labels"], None, batch_size=32, lr=LR, seed=4)
            vl, vc = tr.evaluate(dv["X"], dv["labels"])
            out = {"sums": np.array([loss, corr, vl, vc]), "W0": tr.read("W", 0), "b3": tr.read("b", 3)}
            tr.close()
            return out
        base = cfg.race("dnn trainer epoch", {"X": X, "labels": y}, call, poison={"labels": ((y + 1) % C).astype(np.int32)}, waits=True)
        assert np.isfinite(base["sums"]).all()
    finally:
        cfg.close()


def test_refusals_launch_nothing():
    api = _api()
    from speech_signal_processing_amd import _lib
    ctx = api.default_context()
    layers, X, y = _odd(N=40)
    W = [l[0] for l in layers]
    with pytest.raises(ValueError):
        api.DnnTrainer(ctx, [(W[0], None, True, 1.0)] + layers[1:], max_batch=8)           # rate outside [0, 1)
    with pytest.raises(ValueError):
        api.DnnTrainer(ctx, [(W[0], None, True, -0.5)] + layers[1:], max_batch=8)
    with pytest.raises(NotImplementedError):
        api.DnnTrainer(ctx, layers, max_batch=1025)
    wide = np.zeros((4097, 4), np.float32)
    with pytest.raises(NotImplementedError):
        api.DnnTrainer(ctx, [(wide, None, False, 0.0)], max_batch=8)
    # a null kernel, through the C-ABI itself
    n = len(layers)
    h = ctypes.c_void_p()
    c_w = (ctypes.c_void_p * n)(*[w.ctypes.data for w in W])
    c_w[2] = None
    rc = ctx._lib.ssp_dnn_trainer_create(ctx._h, n, (ctypes.c_int32 * (n + 1))(*ODD), (ctypes.c_int32 * n)(1, 1, 1, 0), (ctypes.c_float * n)(0, 0, 0, 0),
                                         c_w, None, 8, ctypes.byref(h))
    assert rc == _lib.SSP_ERR_INVALID and not h.value
    tr = api.DnnTrainer(ctx, layers, max_batch=16)
    before = _read_all(tr)
    bad = y.copy()
    bad[17] = ODD[-1]
    for kw in (dict(labels=bad), dict(batch_size=0), dict(batch_size=17), dict(order=np.arange(40) + 1)):
        args = dict(labels=y, order=None, batch_size=16)
        args.update(kw)
        with pytest.raises(ValueError):
            tr.epoch(X, args["labels"], args["order"], batch_size=args["batch_size"], lr=LR, seed=0)
    bad[17] = -1
    with pytest.raises(ValueError):
        tr.evaluate(X, bad)
    assert tr.steps == 0
    _same_bits(before, _read_all(tr), ("W", "b", "dW", "db", "mW", "mb", "vW", "vb"))


def test_nn_model_inference_end_to_end(tmp_path):
    """8 Gaussian clusters in 64 dimensions, centres 3 apart, unit noise: three epochs through nn_model.inference against the oracle's float64
    run with the same seed; then the saved network scores"""
    from speech_signal_processing_amd import d_vector as dv
    rng = np.random.default_rng(21)
    C, d = 8, 64
    centres = np.linalg.qr(rng.standard_normal((d, C)))[0].T * (3.0 / np.sqrt(2.0))   # orthogonal, of length 3 / sqrt(2): 3 apart
    yt, yv = rng.integers(0, C, 640), rng.integers(0, C, 160)
    Xt = (centres[yt] + rng.standard_normal((640, d))).astype(np.float32)
    Xv = (centres[yv] + rng.standard_normal((160, d))).astype(np.float32)
    Yt, Yv = np.eye(C)[yt], np.eye(C)[yv]
    model = dv.nn_model(n_class=C)
    hist = model.inference(Xt, Yt, Xv, Yv, epochs=3, batch_size=50, seed=7, model_dir=str(tmp_path))
    ref, net = DO.fit([d, 256, 256, 256, 256, C], Xt, yt, Xv, yv, 3, 50, 1e-4, 7)
    rows = open(os.path.join(str(tmp_path), "nn_training.log")).read().strip().split("\n")
    assert rows[0] == DO.LOG_HEADER and len(rows) == 4
    for e in range(3):
        logged = dict(zip(DO.LOG_HEADER.split(","), rows[e + 1].split(",")))
        assert int(logged["epoch"]) == e
        print("[measured] epoch %d: %s | oracle loss %.6f val_loss %.6f" % (e, rows[e + 1], ref["loss"][e], ref["val_loss"][e]))
        for k, n in (("loss", 640), ("val_loss", 160)):
            assert abs(hist[k][e] - ref[k][e]) <= 1e-4 * max(1.0, abs(ref[k][e])), (k, e)
            assert float(logged[k]) == hist[k][e]
        for k, n in (("acc", 640), ("val_acc", 160)):
            assert abs(hist[k][e] - ref[k][e]) * n <= 1.0 + 1e-9, (k, e)
            assert float(logged[k]) == hist[k][e]
        assert hist["lr"][e] == ref["lr"][e] == float(logged["lr"])
    assert hist["loss"][2] < hist["loss"][0]
    # the saved embedding network: the trainer's first four layers
    tr = model.trainer_
    h = Xv.astype(np.float64)
    for l in range(4):
        h = h @ tr.read("W", l).astype(np.float64) + tr.read("b", l)
        if l < 3:
            h = np.maximum(h, 0)
    registered = dv.load_model("nn").predict(Xv)
    dv._MODELS.pop("nn")
    loaded = dv.load_model("nn", str(tmp_path))
    assert isinstance(loaded, dv.DenseNet) and loaded.output_dim == 256
    emb = loaded.predict(Xv)
    assert np.array_equal(emb, registered)
    assert np.abs(emb - h).max() <= 1e-4 * np.abs(h).max()
    acc = dv.nn_model(n_class=C).test(Xt, Yt, Xv, Yv, model_name="nn")
    print("[measured] nn_model.test accuracy with the trained embedding: %.3f" % acc)
    assert 0.0 <= acc <= 1.0
    dv._MODELS.pop("nn", None)
