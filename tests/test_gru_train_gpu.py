"""GPU tests of the conv + GRU d-vector network's training (csrc/gru_train.hip, api.GruTrainer, d_vector.nn_model.inference_gru) against
the float64 restatement tests/gru_train_oracle.py.  Unpinned against Keras (see the oracle).

The limits are the LSTM trainer's (tests/test_lstm_train_gpu.py), scale-free.  Gradients, and Adam's m and v: per tensor max|gpu - ref| <=
1e-4 max|ref|; a tensor whose reference is all zero must be exactly zero.  Loss sums: 1e-4 max(1, |ref|).  Correct counts: exact.  Weights
after the case's steps at lr = 1e-4: max|gpu - ref| <= 0.05 lr.  Each case first asserts on the CPU, on its very inputs, that single
precision alone stays well inside these limits (the float32 restatement within 1e-5 max|ref| of float64 on the gradients, within 0.01 lr
on the weights), that no row's label sits within 1e-3 of the best other logit and, for hard_sigmoid gates, that no z or r pre-activation
of the float64 run comes within 1e-5 of a clip bound (one flipped clip decision is not a rounding error): a case that fails a
precondition gets another seed, never another limit.

Inputs: Keras-initialised weights, inputs of standard deviation 3, noise of 0.1 on the conv and Dense biases and of 1.5 on the GRU biases:
with Keras' zero biases no gate of these small networks leaves the linear part of hard_sigmoid, with the noise about one gate in ten
is clipped at either bound and the zero branch of s' is exercised.  (At 1024 units the GRU biases get 0.1 like the others: of the
two million pre-activations of `reference-width`, with one in ten near a bound, none of the eight seeds 100 .. 107 stayed 1e-5 away from
every bound.)  A case is T, D / kernel, strides, filters / units x layers / E /
n_class / batch.  The step kernels' tile is 16 sequences x 64 units per workgroup (16 x 16 per wave): `over-the-blocks`
has 144 units (two workgroups and a third with one wave) and 70 sequences (four tiles and six rows).

reference-shape-one-step runs at the batch of 128 the reference trains with; its float64 and float32 restatements take about 13 s
together on 16 threads (measured where the case was chosen): the batch is not halved."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_train_oracle as TO  # noqa: E402
import skewed  # noqa: E402
import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

LR = float(np.float32(1e-4))
PREFIXES = ("", "d", "m", "v")
# name -> T, D, kernel, strides, filters, units, layers, E, n_class, batch, activation, rows, epoch calls (each ceil(rows / batch) steps),
#         random order, absent biases, seed
ODD = (7, 5, (5, 5), (2, 2), 4, 48, 2, 24, 5, 19)      # To 4, 12 features per step; the `same` padding is asymmetric (1 in front, 2 behind)
CASES = {
    "tiny-batch1-hard": (3, 4, (3, 3), (2, 2), 2, 16, 1, 8, 3, 1, "hard_sigmoid", 1, 12, False, (), 10),
    "tiny-batch1-sigmoid": (3, 4, (3, 3), (2, 2), 2, 16, 1, 8, 3, 1, "sigmoid", 1, 12, False, (), 1),
    "odd-48-two-layers-hard": ODD + ("hard_sigmoid", 19, 12, False, (), 5),
    "odd-48-two-layers-sigmoid": ODD + ("sigmoid", 19, 12, False, (), 1),
    "over-the-blocks": (9, 13, (5, 5), (2, 2), 8, 144, 3, 40, 7, 70, "hard_sigmoid", 70, 4, False, (), 36),
    "stride-1": (6, 5, (3, 3), (1, 1), 4, 32, 1, 16, 4, 9, "sigmoid", 9, 4, False, (), 1),
    "tail44-order": (7, 5, (5, 5), (2, 2), 4, 32, 1, 16, 40, 128, "sigmoid", 300, 2, True, (), 1),
    "no-gru-bias": ODD + ("sigmoid", 19, 12, False, ("gru0_b", "gru1_b"), 1),
    "no-conv-bias": ODD + ("hard_sigmoid", 19, 12, False, ("conv_b",), 19),
    "no-dense-bias": ODD + ("sigmoid", 19, 12, False, ("dense_b", "head_b"), 1),
    "reference-width": (20, 13, (5, 5), (2, 2), 64, 1024, 3, 512, 40, 16, "hard_sigmoid", 16, 2, False, (), 100),
    "reference-shape-one-step": (98, 13, (5, 5), (2, 2), 64, 1024, 3, 512, 1251, 128, "sigmoid", 128, 1, False, (), 11),
}
_CACHE = {}


def _api():
    from speech_signal_processing_amd import api
    return api


def _make(T, D, kernel, strides, F, units, layers, E, C, N, seed, absent=()):
    rng = np.random.default_rng(3000 + seed)
    p = TO.keras_init(rng, T, D, F, units, layers, E, C, kernel, strides)
    for k in list(p):
        if k.endswith("_b"):
            noise = 1.5 if k.startswith("gru") and units < 1024 else 0.1
            p[k] = None if k in absent else (noise * rng.standard_normal(p[k].shape)).astype(np.float32)
    X = (3.0 * rng.standard_normal((N, T, D))).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int32)
    order = rng.permutation(N)
    return p, X, y, order


def _keys(names, prefixes=PREFIXES):
    return tuple(pre + k for pre in prefixes for k in names)


def _gap(a, b, keys):
    """largest max|a - b| / max|b| over the tensors of ``keys``; a tensor whose reference is all zero must be zero itself"""
    worst = 0.0
    for k in keys:
        if b[k] is None:
            continue
        x, r = np.asarray(a[k], np.float64).reshape(b[k].shape), b[k]
        if not r.any():
            assert not x.any(), "%s: the reference is exactly zero" % k
            continue
        worst = max(worst, float(np.abs(x - r).max() / np.abs(r).max()))
    return worst


def _weights_gap(a, b, names):
    return max(float(np.abs(np.asarray(a[k], np.float64).reshape(b[k].shape) - b[k]).max()) for k in names if b[k] is not None) / LR


def _measure(name):
    """the case's float64 and float32 runs -> inputs, float64 results and the precondition figures"""
    T, D, kernel, strides, F, units, layers, E, C, B, act, N, calls, use_order, absent, seed = CASES[name]
    p, X, y, order = _make(T, D, kernel, strides, F, units, layers, E, C, N, seed, absent)
    order = order if use_order else None
    out = {}
    for dt in (np.float64, np.float32):
        net = TO.Net(p, strides, act, dt)
        first = None
        for c in range(calls):
            res = net.epoch(X, y, order, B, LR)
            if c == 0:
                first = (res, net.snapshot())
        out[dt] = (first, net.snapshot(), net)
    (res64, one64), end64, net64 = out[np.float64]
    (_, one32), end32, _ = out[np.float32]
    nm = net64.names
    figures = {"drift_g": _gap(one32, one64, _keys(nm, ("d", "m", "v"))), "drift_w": _weights_gap(end32, end64, nm), "margin": net64.min_margin,
               "clip": net64.min_clip}
    return (p, X, y, order, res64, one64, end64, net64.t, nm), figures


def _reference(name):
    """computed once per case; the preconditions are asserted here"""
    if name not in _CACHE:
        data, f = _measure(name)
        print("[precondition] %s: float32 gradients within %.2e max|ref|, weights after %d steps within %.4f lr, margin %.2e, clip margin %.2e" % (
            name, f["drift_g"], data[7], f["drift_w"], f["margin"], f["clip"]))
        assert f["drift_g"] <= 1e-5, "precondition: change the case's seed"
        assert f["drift_w"] <= 0.01, "precondition: change the case's seed"
        assert f["margin"] > 1e-3, "precondition: change the case's seed"
        assert f["clip"] > 1e-5, "precondition: change the case's seed"
        _CACHE[name] = data
    return _CACHE[name]


def _trainer(p, strides, T, D, act, max_batch, ctx=None):
    api = _api()
    n = len([k for k in p if k.endswith("_U")])
    return api.GruTrainer(ctx or api.default_context(), (p["conv_K"], p["conv_b"], strides),
                          [(p["gru%d_W" % i], p["gru%d_U" % i], p["gru%d_b" % i]) for i in range(n)], (p["dense_W"], p["dense_b"]),
                          (p["head_W"], p["head_b"]), T=T, D=D, recurrent_activation=act, reset_after=False, max_batch=max_batch)


def _read_all(tr, names):
    return {pre + k: (tr.read(pre + k) if tr.has_bias.get(k, True) else None) for pre in PREFIXES for k in names}


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), "%s differs on %d elements" % (k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_step_gradients_loss_and_weights(name):
    T, D, kernel, strides, F, units, layers, E, C, B, act, N, calls, use_order, absent, seed = CASES[name]
    p, X, y, order, (loss64, corr64), one64, end64, t64, nm = _reference(name)
    tr = _trainer(p, strides, T, D, act, max(B, 2))
    loss, corr = tr.epoch(X, y, order, batch_size=B, lr=LR)
    one = _read_all(tr, nm)
    print("[measured] %s: loss sum %.6f (ref %.6f), correct %d (ref %d)" % (name, loss, loss64, corr, corr64))
    failed = []
    for k in _keys(nm, ("d", "m", "v")):
        if one64[k] is None:
            continue
        g = _gap(one, one64, (k,))
        print("[measured] %s: %s max|gpu - ref| / max|ref| = %.3e" % (name, k, g))
        if g > 1e-4:
            failed.append((k, g))
    assert not failed, failed
    assert abs(loss - loss64) <= 1e-4 * max(1.0, abs(loss64))
    assert corr == corr64
    for k in absent:
        for prefix in PREFIXES:
            with pytest.raises(ValueError):
                tr.read(prefix + k)
    for _ in range(calls - 1):
        tr.epoch(X, y, order, batch_size=B, lr=LR)
    assert tr.steps == t64
    end = _read_all(tr, nm)
    worst = _weights_gap(end, end64, nm)
    print("[measured] %s: weights after %d steps max|gpu - ref| = %.4f lr" % (name, t64, worst))
    assert worst <= 0.05
    for k in ("m", "v"):
        assert _gap(end, end64, _keys(nm, (k,))) <= 1e-4, k
    tr.close()


# ---- properties, on the 48 x 2 shape: two sequence tiles, the second with three rows, one workgroup of three waves
ST, SD, SKERNEL, SSTRIDES, SF, SUNITS, SLAYERS, SE, SC = ODD[:9]


def _small(N=100, seed=31):
    return _make(ST, SD, SKERNEL, SSTRIDES, SF, SUNITS, SLAYERS, SE, SC, N, seed)


def _small_trainer(p, act, max_batch, ctx=None):
    return _trainer(p, SSTRIDES, ST, SD, act, max_batch, ctx)


NAMES = TO.names(SLAYERS)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_same_call_same_bits_and_an_epoch_equals_its_steps(act):
    p, X, y, order = _small()
    a, a2, b = (_small_trainer(p, act, 19) for _ in range(3))
    ra = a.epoch(X, y, order, batch_size=19, lr=LR)
    assert a2.epoch(X, y, order, batch_size=19, lr=LR) == ra          # the same call from the same state
    _same_bits(_read_all(a, NAMES), _read_all(a2, NAMES))
    lb, cb = 0.0, 0
    for r0 in range(0, 100, 19):       # (the last batch has 5 rows)
        rows = order[r0:r0 + 19]
        l1, c1 = b.epoch(X[rows], y[rows], None, batch_size=19, lr=LR)   # order against pre-permuted rows, one batch per call
        lb, cb = lb + l1, cb + c1
    assert a.steps == b.steps == 6
    assert ra == (lb, cb)
    _same_bits(_read_all(a, NAMES), _read_all(b, NAMES))
    # a row's contribution does not depend on where it sits in X: a permuted X under the inverse order is the same epoch
    perm = np.random.default_rng(3).permutation(100)
    inv = np.argsort(perm)
    c = _small_trainer(p, act, 19)
    assert c.epoch(X[perm], y[perm], inv[order], batch_size=19, lr=LR) == ra
    _same_bits(_read_all(a, NAMES), _read_all(c, NAMES))
    net = TO.Net(p, SSTRIDES, act)
    lo, co = net.epoch(X, y, order, 19, LR)
    if net.min_margin > 1e-3:
        assert ra[1] == co
    if net.min_clip > 1e-5:
        assert abs(ra[0] - lo) <= 1e-4 * max(1.0, abs(lo))


def test_host_arrays_equal_device_tensors():
    import torch
    p, X, y, order = _small()
    a, b = _small_trainer(p, "sigmoid", 32), _small_trainer(p, "sigmoid", 32)
    xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    assert a.epoch(X, y, order, batch_size=32, lr=LR) == b.epoch(xd, yd, order, batch_size=32, lr=LR)
    _same_bits(_read_all(a, NAMES), _read_all(b, NAMES))
    assert a.evaluate(X, y) == b.evaluate(xd, yd)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_evaluate_against_the_oracle_changes_nothing_and_the_embedding_agrees(act):
    from speech_signal_processing_amd import d_vector as dv
    p, X, y, order = _small(seed=32)
    tr = _small_trainer(p, act, 32)
    tr.epoch(X, y, order, batch_size=32, lr=LR)
    before, t = _read_all(tr, NAMES), tr.steps
    loss, corr = tr.evaluate(X, y)        # four chunks of the trainer's max_batch, the last of 4 rows
    assert tr.steps == t == 4
    _same_bits(before, _read_all(tr, NAMES))
    net = TO.Net({k: before[k] for k in NAMES}, SSTRIDES, act)       # the GPU's weights
    lo, co = net.evaluate(X, y)
    print("[measured] evaluate %s: loss sum %.6f (ref %.6f), correct %d (ref %d), margin %.2e" % (act, loss, lo, corr, co, net.min_margin))
    assert net.min_margin > 1e-3, "precondition: change the seed"
    assert abs(loss - lo) <= 1e-4 * max(1.0, abs(lo)) and corr == co
    assert tr.evaluate(X, y) == (loss, corr)
    # the embedding ConvGruNet computes from the trained weights against the oracle's forward: the project's feature rule
    ref = net.embedding(X)
    spk = dv.ConvGruNet((before["conv_K"], before["conv_b"], SSTRIDES), [(before["gru%d_W" % i], before["gru%d_U" % i], before["gru%d_b" % i])
                                                                         for i in range(SLAYERS)], (before["dense_W"], before["dense_b"]),
                        recurrent_activation=act, reset_after=False)
    emb = spk.predict(X)
    assert np.abs(emb - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_refusals_launch_nothing():
    api = _api()
    ctx = api.default_context()
    p, X, y, order = _small(N=40)
    conv = (p["conv_K"], p["conv_b"], SSTRIDES)
    grus = [(p["gru%d_W" % i], p["gru%d_U" % i], p["gru%d_b" % i]) for i in range(SLAYERS)]
    dense, head = (p["dense_W"], p["dense_b"]), (p["head_W"], p["head_b"])
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731

    def make(conv=conv, grus=grus, dense=dense, head=head, **kw):
        args = dict(T=ST, D=SD, recurrent_activation="sigmoid", reset_after=False, max_batch=16)
        args.update(kw)
        return api.GruTrainer(ctx, conv, grus, dense, head, **args)
    with pytest.raises(ValueError):
        make(recurrent_activation="relu")
    with pytest.raises(ValueError):
        make(reset_after=1)
    with pytest.raises(NotImplementedError):
        make(reset_after=True)            # the other cell is not trained
    for kw in (dict(T=0), dict(T=1025), dict(max_batch=0), dict(max_batch=1025)):
        with pytest.raises(NotImplementedError):
            make(**kw)
    g48 = [(z(12, 144), z(48, 144), None)]
    with pytest.raises(NotImplementedError):
        make(conv=(z(8, 5, 1, 4), None, SSTRIDES), grus=g48)                                   # kernel height
    with pytest.raises(NotImplementedError):
        make(conv=(z(5, 5, 1, 257), None, SSTRIDES), grus=[(z(3 * 257, 144), z(48, 144), None)])   # filters
    with pytest.raises(NotImplementedError):
        make(conv=(p["conv_K"], None, (3, 3)), grus=[(z(8, 144), z(48, 144), None)])            # strides
    with pytest.raises(NotImplementedError):
        make(grus=g48 + [(z(48, 144), z(48, 144), None)] * 4)                                   # five layers
    with pytest.raises(NotImplementedError):
        make(grus=[(z(12, 72), z(24, 72), None)], dense=(z(24, SE), None))                     # units off 16
    with pytest.raises(NotImplementedError):
        make(grus=[(z(12, 3 * 1040), z(1040, 3 * 1040), None)], dense=(z(1040, SE), None))     # units above 1024
    with pytest.raises(NotImplementedError):
        make(head=(z(SE, 1), None))                                                            # one class
    with pytest.raises(NotImplementedError):
        make(head=(z(SE, 4097), None))
    with pytest.raises(NotImplementedError):                                                   # the workspace cap (25 GB)
        make(grus=[(z(12, 3072), z(1024, 3072), None)], dense=(z(1024, SE), None), T=1024, max_batch=1024)
    tr = make()
    before = _read_all(tr, NAMES)
    bad = y.copy()
    bad[17] = SC
    for kw in (dict(labels=bad), dict(batch_size=0), dict(batch_size=17), dict(order=np.arange(40) + 1), dict(order=np.arange(40) - 1)):
        args = dict(labels=y, order=None, batch_size=16)
        args.update(kw)
        with pytest.raises(ValueError):
            tr.epoch(X, args["labels"], args["order"], batch_size=args["batch_size"], lr=LR)
    bad[17] = -1
    with pytest.raises(ValueError):
        tr.evaluate(X, bad)
    assert tr.steps == 0
    _same_bits(before, _read_all(tr, NAMES))


@pytest.mark.parametrize("skew", [4, 8, 12])
def test_arrays_off_16_byte_alignment(skew):
    """X, the labels and the read-back buffers 4 / 8 / 12 bytes past a 16-byte line give the bits of aligned ones, and nothing around them
    is read into the result (NaN guards) or written"""
    p, X, y, order = _small()
    N = len(y)
    got = []
    for s in (0, skew):
        xv, xg = skewed.view(X.size, "float32", s, fill=X)
        yv, yg = skewed.view(N, "int32", s, fill=y)
        tr = _small_trainer(p, "sigmoid", 64)
        res = tr.epoch(xv.view(N, ST, SD), yv, order, batch_size=64, lr=LR)
        ev = tr.evaluate(xv.view(N, ST, SD), yv)
        snap = {}
        for k in _keys(NAMES):
            ov, og = skewed.view(int(np.prod(tr.shapes[k if k in NAMES else k[1:]])), "float32", s, backend="numpy")
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
        p, X, y, _ = _small()
        # fresh trainers made ahead (allocations, the upload and its host wait), so that nothing but the epoch and the evaluation sits
        # between the producer and the reads of X and labels; the harness calls once for the baseline and once per racing run
        pool = [_small_trainer(p, "sigmoid", 32, cfg.ctx) for _ in range(8)]

        def call(dv, _):
            tr = pool.pop()
            loss, corr = tr.epoch(dv["X"], dv["labels"], None, batch_size=32, lr=LR)
            vl, vc = tr.evaluate(dv["X"], dv["labels"])
            out = {"sums": np.array([loss, corr, vl, vc]), "K": tr.read("conv_K"), "U": tr.read("gru1_U"), "b": tr.read("head_b")}
            tr.close()
            return out
        base = cfg.race("gru trainer epoch", {"X": X, "labels": y}, call, poison={"labels": ((y + 1) % SC).astype(np.int32)}, waits=True)
        assert np.isfinite(base["sums"]).all()
    finally:
        cfg.close()


# ---- nn_model.inference_gru end to end
TOY = dict(units=32, filters=4, embedding=16, n_gru=2)
TOY_SEED = 19              # (12 .. 18 leave a label within 1e-3 of the best other logit, or a gate within 1e-4 of a clip bound)
TOY_FAST_LR, TOY_FAST_EPOCHS, TOY_FAST_BATCH = 1e-2, 6, 32   # over which the float64 oracle's loss falls by more than half (asserted below)


def _toy(seed=41):
    rng = np.random.default_rng(seed)
    C, T, D = 4, 12, 13
    means = 1.5 * rng.standard_normal((C, D))
    yt, yv = rng.integers(0, C, 256), rng.integers(0, C, 64)
    Xt = (means[yt][:, None, :] + rng.standard_normal((256, T, D))).astype(np.float32)
    Xv = (means[yv][:, None, :] + rng.standard_normal((64, T, D))).astype(np.float32)
    return C, Xt, yt, Xv, yv


def test_nn_model_inference_gru_end_to_end(tmp_path):
    """4 classes told apart by class-dependent feature means: three epochs through nn_model.inference_gru against the oracle's float64 fit
    with the same seed, draws and permutations; then a faster fit learns, and enroll / eval name two toy speakers with the saved network"""
    from speech_signal_processing_amd import d_vector as dv
    C, Xt, yt, Xv, yv = _toy()
    Yt, Yv = np.eye(C)[yt], np.eye(C)[yv]
    model = dv.nn_model(n_class=C)
    d1 = str(tmp_path / "slow")
    hist = model.inference_gru(Xt[..., None], Yt, Xv[..., None], Yv, epochs=3, seed=TOY_SEED, model_dir=d1, **TOY)
    ref, net = TO.fit(Xt, yt, Xv, yv, C, 3, 128, 1e-4, TOY_SEED, **TOY)
    assert net.min_clip > 1e-5 and net.min_margin > 1e-3, "precondition: change the seed"
    rows = open(os.path.join(d1, "gru_training.log")).read().strip().split("\n")
    assert rows[0] == TO.LOG_HEADER and len(rows) == 4
    for e in range(3):
        logged = dict(zip(TO.LOG_HEADER.split(","), rows[e + 1].split(",")))
        assert int(logged["epoch"]) == e
        print("[measured] epoch %d: %s | oracle loss %.6f val_loss %.6f" % (e, rows[e + 1], ref["loss"][e], ref["val_loss"][e]))
        for k, n in (("loss", 256), ("val_loss", 64)):
            assert abs(hist[k][e] * n - ref[k][e] * n) <= 1e-4 * max(1.0, abs(ref[k][e] * n)), (k, e)
            assert float(logged[k]) == hist[k][e]
        for k, n in (("acc", 256), ("val_acc", 64)):
            assert round(hist[k][e] * n) == round(ref[k][e] * n), (k, e)
            assert float(logged[k]) == hist[k][e]
        assert hist["lr"][e] == ref["lr"][e] == float(logged["lr"])
    z = np.load(os.path.join(d1, "d_vector_gru.npz"))
    assert str(z["kind"]) == "conv_gru" and str(z["recurrent_activation"]) == "hard_sigmoid" and int(z["reset_after"]) == 0
    dv._MODELS.pop("gru")
    loaded = dv.load_model("gru", d1)
    assert isinstance(loaded, dv.ConvGruNet) and loaded.output_dim == TOY["embedding"] and loaded.recurrent_activation == "hard_sigmoid"
    tr = model.trainer_
    assert np.array_equal(loaded.K, tr.read("conv_K")) and np.array_equal(loaded.bc, tr.read("conv_b"))
    for i in range(TOY["n_gru"]):
        for j, k in enumerate(("W", "U", "b")):
            assert np.array_equal(loaded.grus[i][j], tr.read("gru%d_%s" % (i, k)))
    assert np.array_equal(loaded.Wd, tr.read("dense_W")) and np.array_equal(loaded.bd, tr.read("dense_b"))
    dv._MODELS.pop("gru")
    with pytest.raises(NotImplementedError):
        model.inference_gru(Xt, Yt, Xv, Yv, epochs=1, reset_after=True, model_dir=d1, **TOY)
    # at a larger lr the network learns: the oracle first, on the CPU
    fast, _ = TO.fit(Xt, yt, Xv, yv, C, TOY_FAST_EPOCHS, TOY_FAST_BATCH, TOY_FAST_LR, TOY_SEED, **TOY)
    assert fast["loss"][-1] < 0.5 * fast["loss"][0], "precondition: more epochs"
    d2 = str(tmp_path / "fast")
    model = dv.nn_model(n_class=C)
    hist = model.inference_gru(Xt, Yt, Xv, Yv, epochs=TOY_FAST_EPOCHS, batch_size=TOY_FAST_BATCH, lr=TOY_FAST_LR, seed=TOY_SEED, model_dir=d2, **TOY)
    print("[measured] lr %g: loss %s (oracle %s)" % (TOY_FAST_LR, ["%.4f" % v for v in hist["loss"]], ["%.4f" % v for v in fast["loss"]]))
    assert hist["loss"][-1] < 0.5 * hist["loss"][0]
    # enroll two toy speakers and evaluate a held-out chunk of each with the registered 'gru'
    who = dv.nn_model(n_class=C)
    for s, name in ((0, "anna"), (1, "ben")):
        who.enroll(Xt[yt == s], name, model_name="gru")
    for s, name in ((0, "anna"), (1, "ben")):
        assert who.eval(Xv[yv == s][0], model_name="gru") == name
    dv._MODELS.pop("gru", None)
