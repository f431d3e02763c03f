"""GPU tests of the recurrent d-vector network's training (csrc/lstm_train.hip, api.LstmTrainer, d_vector.nn_model.inference_lstm) against
the float64 restatement tests/lstm_train_oracle.py.  Unpinned against Keras (see the oracle).

The limits are the dense trainer's (tests/test_dnn_train_gpu.py), scale-free.  Gradients, and Adam's m and v: per tensor max|gpu - ref| <=
1e-4 max|ref|; a tensor whose reference is all zero (dU at T = 1) must be exactly zero.  Loss sums: 1e-4 max(1, |ref|).  Correct counts:
exact.  Weights after the case's steps at lr = 1e-4: max|gpu - ref| <= 0.05 lr.  Each case first asserts on the CPU, on its very inputs,
that single precision alone stays well inside these limits (the float32 restatement within 1e-5 max|ref| of float64 on the gradients,
within 0.01 lr on the weights), that no row's label sits within 1e-3 of the best other logit and, for hard_sigmoid gates, that no i, f or o
pre-activation of the float64 run comes within 1e-5 of a clip bound (one flipped clip decision is not a rounding error): a case that
fails a precondition gets another seed, never another limit.

Inputs: Keras-initialised weights, noise of 0.1 on the biases, inputs of standard deviation 3.  The reference shape runs its steps at the full
batch of 128 on sigmoid gates and at a batch of 16 on hard_sigmoid gates: three hard_sigmoid steps at batch 128 rarely stay 1e-5 away from
every clip bound (12 544 x 384 pre-activations per step).  ONE hard_sigmoid step at batch 128 does for two of the eight seeds tried
(100 .. 107: 105 and 107), and seed 107 is a case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_train_oracle as LO  # noqa: E402
import skewed  # noqa: E402
import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

LR = float(np.float32(1e-4))
KEYS = tuple(p + k for p in ("", "d", "m", "v") for k in LO.NAMES)
GRAD_KEYS = tuple(p + k for p in ("d", "m", "v") for k in LO.NAMES)
# name -> d_in, units, T, batch, n_class, activation, rows, epoch calls (each runs ceil(rows / batch) steps), random order, absent biases, seed
CASES = {
    "reference-sigmoid-40": (13, 128, 98, 128, 40, "sigmoid", 128, 3, False, (), 1),
    "reference-sigmoid-1251": (13, 128, 98, 128, 1251, "sigmoid", 128, 2, False, (), 2),
    "reference-hard-batch16": (13, 128, 98, 16, 40, "hard_sigmoid", 16, 3, False, (), 3),
    "reference-hard-batch128-one-step": (13, 128, 98, 128, 40, "hard_sigmoid", 128, 1, False, (), 107),
    "odd-26-48-hard": (26, 48, 7, 19, 5, "hard_sigmoid", 19, 12, False, (), 23),
    "odd-26-48-sigmoid": (26, 48, 7, 19, 5, "sigmoid", 19, 12, False, (), 5),
    "odd-39-64-hard": (39, 64, 5, 33, 7, "hard_sigmoid", 33, 12, False, (), 22),
    "odd-39-64-sigmoid": (39, 64, 5, 33, 7, "sigmoid", 33, 12, False, (), 20),
    "tiny-batch1-hard": (13, 16, 1, 1, 3, "hard_sigmoid", 1, 12, False, (), 8),
    "tiny-batch1-sigmoid": (13, 16, 1, 1, 3, "sigmoid", 1, 12, False, (), 9),
    "tiny-batch3-hard": (13, 16, 2, 3, 3, "hard_sigmoid", 3, 12, False, (), 10),
    "tiny-batch3-sigmoid": (13, 16, 2, 3, 3, "sigmoid", 3, 12, False, (), 11),
    "tail44-order": (13, 32, 9, 128, 40, "sigmoid", 300, 4, True, (), 12),
    "no-lstm-bias": (26, 48, 7, 19, 5, "sigmoid", 19, 12, False, ("b",), 20),
    "no-dense-bias": (26, 48, 7, 19, 5, "hard_sigmoid", 19, 12, False, ("bd",), 28),
}
_CACHE = {}


def _api():
    from speech_signal_processing_amd import api
    return api


def _make(d_in, units, T, C, N, seed, absent=()):
    rng = np.random.default_rng(2000 + seed)
    W, U, b, Wd, bd = LO.keras_init(rng, d_in, units, C)
    b = (b + 0.1 * rng.standard_normal(b.shape)).astype(np.float32)
    bd = (0.1 * rng.standard_normal(bd.shape)).astype(np.float32)
    X = (3.0 * rng.standard_normal((N, T, d_in))).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int32)
    order = rng.permutation(N)
    return (W, U, None if "b" in absent else b, Wd, None if "bd" in absent else bd), X, y, order


def _gap(a, b, keys):
    """largest max|a - b| / max|b| over the tensors of ``keys``; a tensor whose reference is all zero must be zero itself"""
    worst = 0.0
    for k in keys:
        if b[k] is None:
            continue
        x, r = np.asarray(a[k], np.float64), b[k]
        if not r.any():
            assert not x.any(), "%s: the reference is exactly zero" % k
            continue
        worst = max(worst, float(np.abs(x - r).max() / np.abs(r).max()))
    return worst


def _weights_gap(a, b):
    return max(float(np.abs(np.asarray(a[k], np.float64) - b[k]).max()) for k in LO.NAMES if b[k] is not None) / LR


def _measure(name):
    """the case's float64 and float32 runs -> inputs, float64 results and the precondition figures"""
    d_in, units, T, B, C, act, N, calls, use_order, absent, seed = CASES[name]
    params, X, y, order = _make(d_in, units, T, C, N, seed, absent)
    order = order if use_order else None
    out = {}
    for dt in (np.float64, np.float32):
        net = LO.Net(*params, act, dt)
        first = None
        for c in range(calls):
            res = net.epoch(X, y, order, B, LR)
            if c == 0:
                first = (res, net.snapshot())
        out[dt] = (first, net.snapshot(), net)
    (res64, one64), end64, net64 = out[np.float64]
    (_, one32), end32, _ = out[np.float32]
    figures = {"drift_g": _gap(one32, one64, GRAD_KEYS), "drift_w": _weights_gap(end32, end64), "margin": net64.min_margin, "clip": net64.min_clip}
    return (params, X, y, order, res64, one64, end64, net64.t), figures


def _reference(name):
    """computed once per case; the preconditions are asserted here"""
    if name not in _CACHE:
        data, f = _measure(name)
        print("[precondition] %s: float32 gradients within %.2e max|ref|, weights after %d steps within %.4f lr, margin %.2e, clip margin %.2e" % (
            name, f["drift_g"], data[-1], f["drift_w"], f["margin"], f["clip"]))
        assert f["drift_g"] <= 1e-5, "precondition: change the case's seed"
        assert f["drift_w"] <= 0.01, "precondition: change the case's seed"
        assert f["margin"] > 1e-3, "precondition: change the case's seed"
        assert f["clip"] > 1e-5, "precondition: change the case's seed"
        _CACHE[name] = data
    return _CACHE[name]


def _trainer(params, T, act, max_batch, ctx=None):
    api = _api()
    return api.LstmTrainer(ctx or api.default_context(), *params, T=T, recurrent_activation=act, max_batch=max_batch)


def _tensor(key):
    """'dWd' -> 'Wd': the tensor a key of KEYS names"""
    return key if key in LO.NAMES else key[1:]


def _read_all(tr):
    return {k: (tr.read(k) if tr.has_bias.get(_tensor(k), True) else None) for k in KEYS}


def _same_bits(a, b, keys=KEYS):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), "%s differs on %d elements" % (k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_step_gradients_loss_and_weights(name):
    d_in, units, T, B, C, act, N, calls, use_order, absent, seed = CASES[name]
    params, X, y, order, (loss64, corr64), one64, end64, t64 = _reference(name)
    tr = _trainer(params, T, act, max(B, 2))
    loss, corr = tr.epoch(X, y, order, batch_size=B, lr=LR)
    one = _read_all(tr)
    print("[measured] %s: loss sum %.6f (ref %.6f), correct %d (ref %d)" % (name, loss, loss64, corr, corr64))
    for k in GRAD_KEYS:
        if one64[k] is None:
            continue
        g = _gap(one, one64, (k,))
        print("[measured] %s: %s max|gpu - ref| / max|ref| = %.3e" % (name, k, g))
        assert g <= 1e-4, k
    assert abs(loss - loss64) <= 1e-4 * max(1.0, abs(loss64))
    assert corr == corr64
    for k in absent:
        for prefix in ("", "d", "m", "v"):
            with pytest.raises(ValueError):
                tr.read(prefix + k)
    for _ in range(calls - 1):
        tr.epoch(X, y, order, batch_size=B, lr=LR)
    assert tr.steps == t64
    end = _read_all(tr)
    worst = _weights_gap(end, end64)
    print("[measured] %s: weights after %d steps max|gpu - ref| = %.4f lr" % (name, t64, worst))
    assert worst <= 0.05
    for k in ("m", "v"):
        assert _gap(end, end64, tuple(k + n for n in LO.NAMES)) <= 1e-4, k
    tr.close()


# ---- properties, on a small shape: two workgroups, the second with three sequences, three waves each, d_in over one group of 16
SMALL = (26, 48, 7, 5)      # d_in, units, T, n_class


def _small(act="sigmoid", N=100, seed=31):
    return _make(SMALL[0], SMALL[1], SMALL[2], SMALL[3], N, seed)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_same_call_same_bits_and_an_epoch_equals_its_steps(act):
    params, X, y, order = _small()
    T = SMALL[2]
    a, a2, b = (_trainer(params, T, act, 19) for _ in range(3))
    ra = a.epoch(X, y, order, batch_size=19, lr=LR)
    assert a2.epoch(X, y, order, batch_size=19, lr=LR) == ra          # the same call from the same state
    _same_bits(_read_all(a), _read_all(a2))
    lb, cb = 0.0, 0
    for r0 in range(0, 100, 19):       # (the last batch has 5 rows)
        rows = order[r0:r0 + 19]
        l1, c1 = b.epoch(X[rows], y[rows], None, batch_size=19, lr=LR)   # order against pre-permuted rows, one batch per call
        lb, cb = lb + l1, cb + c1
    assert a.steps == b.steps == 6
    assert ra == (lb, cb)
    _same_bits(_read_all(a), _read_all(b))
    # a row's contribution does not depend on its place among the workgroups beyond the fixed order of the sums: a permuted X under the
    # inverse order is the same epoch
    perm = np.random.default_rng(3).permutation(100)
    inv = np.argsort(perm)
    c = _trainer(params, T, act, 19)
    assert c.epoch(X[perm], y[perm], inv[order], batch_size=19, lr=LR) == ra
    _same_bits(_read_all(a), _read_all(c))
    net = LO.Net(*params, act)
    lo, co = net.epoch(X, y, order, 19, LR)
    if net.min_margin > 1e-3:
        assert ra[1] == co
    if net.min_clip > 1e-5:
        assert abs(ra[0] - lo) <= 1e-4 * max(1.0, abs(lo))


def test_host_arrays_equal_device_tensors():
    import torch
    params, X, y, order = _small()
    a, b = _trainer(params, SMALL[2], "sigmoid", 32), _trainer(params, SMALL[2], "sigmoid", 32)
    xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    assert a.epoch(X, y, order, batch_size=32, lr=LR) == b.epoch(xd, yd, order, batch_size=32, lr=LR)
    _same_bits(_read_all(a), _read_all(b))
    assert a.evaluate(X, y) == b.evaluate(xd, yd)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_evaluate_against_the_oracle_changes_nothing_and_the_embedding_agrees(act):
    from speech_signal_processing_amd import d_vector as dv
    params, X, y, order = _small(seed=32)
    tr = _trainer(params, SMALL[2], act, 32)
    tr.epoch(X, y, order, batch_size=32, lr=LR)
    before, t = _read_all(tr), tr.steps
    loss, corr = tr.evaluate(X, y)        # four chunks of the trainer's max_batch, the last of 4 rows
    assert tr.steps == t == 4
    _same_bits(before, _read_all(tr))
    net = LO.Net(*(before[k] for k in LO.NAMES), act)       # the GPU's weights
    lo, co = net.evaluate(X, y)
    print("[measured] evaluate %s: loss sum %.6f (ref %.6f), correct %d (ref %d), margin %.2e" % (act, loss, lo, corr, co, net.min_margin))
    assert net.min_margin > 1e-3, "precondition: change the seed"
    assert abs(loss - lo) <= 1e-4 * max(1.0, abs(lo)) and corr == co
    assert tr.evaluate(X, y) == (loss, corr)
    # the embedding LstmNet computes from the trained weights against the oracle's forward: the project's feature rule
    h, _ = net.forward(X)
    emb = dv.LstmNet(before["W"], before["U"], before["b"], recurrent_activation=act).predict(X)
    assert np.abs(emb - h).max() <= 1e-4 * max(1.0, np.abs(h).max())


def test_refusals_launch_nothing():
    api = _api()
    ctx = api.default_context()
    params, X, y, order = _small(N=40)
    W, U, b, Wd, bd = params
    T = SMALL[2]
    with pytest.raises(ValueError):
        api.LstmTrainer(ctx, W, U, b, Wd, bd, T=T, recurrent_activation="relu")
    for kw in (dict(T=0), dict(T=1025), dict(max_batch=0), dict(max_batch=1025)):
        args = dict(T=T, max_batch=16)
        args.update(kw)
        with pytest.raises(NotImplementedError):
            api.LstmTrainer(ctx, W, U, b, Wd, bd, recurrent_activation="sigmoid", **args)
    with pytest.raises(NotImplementedError):
        api.LstmTrainer(ctx, np.zeros((65, 192), np.float32), U, b, Wd, bd, T=T, recurrent_activation="sigmoid")        # d_in
    with pytest.raises(NotImplementedError):
        api.LstmTrainer(ctx, np.zeros((26, 96), np.float32), np.zeros((24, 96), np.float32), None, np.zeros((24, 5), np.float32), None, T=T,
                        recurrent_activation="sigmoid")                                                                 # units off 16
    with pytest.raises(NotImplementedError):
        api.LstmTrainer(ctx, W, U, b, np.zeros((48, 1), np.float32), None, T=T, recurrent_activation="sigmoid")         # one class
    with pytest.raises(NotImplementedError):
        api.LstmTrainer(ctx, W, U, b, np.zeros((48, 4097), np.float32), None, T=T, recurrent_activation="sigmoid")
    tr = _trainer(params, T, "sigmoid", 16)
    before = _read_all(tr)
    bad = y.copy()
    bad[17] = SMALL[3]
    for kw in (dict(labels=bad), dict(batch_size=0), dict(batch_size=17), dict(order=np.arange(40) + 1), dict(order=np.arange(40) - 1)):
        args = dict(labels=y, order=None, batch_size=16)
        args.update(kw)
        with pytest.raises(ValueError):
            tr.epoch(X, args["labels"], args["order"], batch_size=args["batch_size"], lr=LR)
    bad[17] = -1
    with pytest.raises(ValueError):
        tr.evaluate(X, bad)
    assert tr.steps == 0
    _same_bits(before, _read_all(tr))


@pytest.mark.parametrize("skew", [4, 8, 12])
def test_arrays_off_16_byte_alignment(skew):
    """X, the labels and the read-back buffers 4 / 8 / 12 bytes past a 16-byte line give the bits of aligned ones, and nothing around them
    is read into the result (NaN guards) or written"""
    params, X, y, order = _small()
    N = len(y)
    got = []
    for s in (0, skew):
        xv, xg = skewed.view(X.size, "float32", s, fill=X)
        yv, yg = skewed.view(N, "int32", s, fill=y)
        tr = _trainer(params, SMALL[2], "sigmoid", 64)
        res = tr.epoch(xv.view(N, SMALL[2], SMALL[0]), yv, order, batch_size=64, lr=LR)
        ev = tr.evaluate(xv.view(N, SMALL[2], SMALL[0]), yv)
        snap = {}
        for k in KEYS:
            ov, og = skewed.view(int(np.prod(tr.shapes[_tensor(k)])), "float32", s, backend="numpy")
            tr.read(k, out=ov)
            skewed.check_guards(og, "%s skew %d" % (k, s))
            snap[k] = ov.copy()
        got.append((res, ev, snap))
        skewed.check_guards(xg, "X skew %d" % s)
        skewed.check_guards(yg, "labels skew %d" % s)
        assert np.isfinite(res[0]) and np.isfinite(ev[0])
        tr.close()
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1]
    _same_bits(got[0][2], got[1][2])


@pytest.mark.parametrize("mode", SO.MODES)
def test_stream_order(mode):
    """X and labels produced on another torch stream just before the call: the epoch and the evaluation see them"""
    cfg = SO.Config(mode)
    try:
        params, X, y, _ = _small()
        C = SMALL[3]
        # fresh trainers made ahead (allocations, the upload and its host wait), so that nothing but the epoch and the evaluation sits
        # between the producer and the reads of X and labels; the harness calls once for the baseline and once per racing run
        pool = [_trainer(params, SMALL[2], "sigmoid", 32, cfg.ctx) for _ in range(8)]

        def call(dv, _):
            tr = pool.pop()
            loss, corr = tr.epoch(dv["X"], dv["labels"], None, batch_size=32, lr=LR)
            vl, vc = tr.evaluate(dv["X"], dv["labels"])
            out = {"sums": np.array([loss, corr, vl, vc]), "W": tr.read("W"), "U": tr.read("U"), "bd": tr.read("bd")}
            tr.close()
            return out
        base = cfg.race("lstm trainer epoch", {"X": X, "labels": y}, call, poison={"labels": ((y + 1) % C).astype(np.int32)}, waits=True)
        assert np.isfinite(base["sums"]).all()
    finally:
        cfg.close()


# ---- nn_model.inference_lstm end to end
TOY_EPOCHS_FAST = 3     # epochs at lr = 1e-2 over which the float64 oracle's loss falls by more than half (asserted on the CPU below)


def _toy(seed=41):
    rng = np.random.default_rng(seed)
    C, T, D = 4, 12, 13
    means = 1.5 * rng.standard_normal((C, D))
    yt, yv = rng.integers(0, C, 256), rng.integers(0, C, 64)
    Xt = (means[yt][:, None, :] + rng.standard_normal((256, T, D))).astype(np.float32)
    Xv = (means[yv][:, None, :] + rng.standard_normal((64, T, D))).astype(np.float32)
    return C, Xt, yt, Xv, yv


def test_nn_model_inference_lstm_end_to_end(tmp_path):
    """4 classes told apart by class-dependent feature means: three epochs through nn_model.inference_lstm against the oracle's float64 fit
    with the same seed, draws and permutations; then a faster fit learns, and enroll / eval find the saved network by themselves"""
    from speech_signal_processing_amd import d_vector as dv
    C, Xt, yt, Xv, yv = _toy()
    Yt, Yv = np.eye(C)[yt], np.eye(C)[yv]
    model = dv.nn_model(n_class=C)
    d1 = str(tmp_path / "slow")
    hist = model.inference_lstm(Xt, Yt, Xv, Yv, epochs=3, seed=12, model_dir=d1)
    ref, net = LO.fit(Xt, yt, Xv, yv, C, 3, 128, 1e-4, 12)
    assert net.min_clip > 1e-5 and net.min_margin > 1e-3, "precondition: change the seed"
    rows = open(os.path.join(d1, "lstm_training.log")).read().strip().split("\n")
    assert rows[0] == LO.LOG_HEADER and len(rows) == 4
    for e in range(3):
        logged = dict(zip(LO.LOG_HEADER.split(","), rows[e + 1].split(",")))
        assert int(logged["epoch"]) == e
        print("[measured] epoch %d: %s | oracle loss %.6f val_loss %.6f" % (e, rows[e + 1], ref["loss"][e], ref["val_loss"][e]))
        for k, n in (("loss", 256), ("val_loss", 64)):
            assert abs(hist[k][e] * n - ref[k][e] * n) <= 1e-4 * max(1.0, abs(ref[k][e] * n)), (k, e)
            assert float(logged[k]) == hist[k][e]
        for k, n in (("acc", 256), ("val_acc", 64)):
            assert round(hist[k][e] * n) == round(ref[k][e] * n), (k, e)
            assert float(logged[k]) == hist[k][e]
        assert hist["lr"][e] == ref["lr"][e] == float(logged["lr"])
    z = np.load(os.path.join(d1, "d_vector_lstm.npz"))
    assert str(z["kind"]) == "lstm" and str(z["recurrent_activation"]) == "hard_sigmoid"
    assert np.array_equal(z["W"], model.trainer_.read("W")) and np.array_equal(z["U"], model.trainer_.read("U"))
    dv._MODELS.pop("lstm")
    loaded = dv.load_model("lstm", d1)
    assert isinstance(loaded, dv.LstmNet) and loaded.output_dim == 128 and loaded.recurrent_activation == "hard_sigmoid"
    dv._MODELS.pop("lstm")
    # at lr = 1e-2 the network learns: the oracle first, on the CPU
    fast, _ = LO.fit(Xt, yt, Xv, yv, C, TOY_EPOCHS_FAST, 128, 1e-2, 12)
    assert fast["loss"][-1] < 0.5 * fast["loss"][0], "precondition: more epochs"
    d2 = str(tmp_path / "fast")
    model = dv.nn_model(n_class=C)
    hist = model.inference_lstm(Xt.reshape(256, -1), Yt, Xv.reshape(64, -1), Yv, epochs=TOY_EPOCHS_FAST, lr=1e-2, seed=12, D=13, model_dir=d2)
    print("[measured] lr 1e-2: loss %s (oracle %s)" % (["%.4f" % v for v in hist["loss"]], ["%.4f" % v for v in fast["loss"]]))
    assert hist["loss"][-1] < 0.5 * hist["loss"][0]
    # enroll two toy speakers and evaluate a held-out chunk of each with the default model: the registered 'lstm'
    who = dv.nn_model(n_class=C)
    for s, name in ((0, "anna"), (1, "ben")):
        who.enroll(Xt[yt == s], name)
    for s, name in ((0, "anna"), (1, "ben")):
        assert who.eval(Xv[yv == s][0]) == name
    dv._MODELS.pop("lstm", None)
