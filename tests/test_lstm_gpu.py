"""GPU tests of the LSTM d-vector network (run with -m gpu on an MI355X): the recurrent MFMA kernel through api.LstmForward and
d_vector.LstmNet against the float64 restatement tests/lstm_oracle.py.

Tolerance: the project's feature rule (tests/test_gpu_parity.py assert_feat_close, north star 1e-4):
    max |gpu - ref| <= 1e-4 max(1, max |ref|)
Input condition: an LSTM with large recurrent weights is chaotic and float32 then leaves float64 whatever the kernel does.  Multi-step
cases draw weights at Keras' own initialisation scale x <= 2 and first assert, on the CPU, that the float32 restatement is within 1e-5 of
the float64 one on the very inputs of the case.  Large weights (x 10, saturated gates) are covered at T = 1 and 2 only.
Unpinned: the reference holds no LSTM weights or outputs and Keras is not installed; the restatement is corroborated against
torch.nn.LSTM in tests/test_lstm_host.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_oracle as LO  # noqa: E402

pytestmark = pytest.mark.gpu

FEAT_TOL = 1e-4
PRECOND = 1e-5


def assert_feat_close(got, ref, what=""):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), what + ": non-finite pattern differs"
    g, r = got[fin], ref[fin]
    if r.size == 0:
        return 0.0
    err = float(np.abs(g - r).max())
    print("[measured] %s: max abs err %.3e (ref max %.3e)" % (what, err, np.abs(r).max()))
    assert err <= FEAT_TOL * max(1.0, np.abs(r).max()), "%s: max abs err %.3e (ref max %.3e)" % (what, err, np.abs(r).max())
    return err


@pytest.fixture(scope="module")
def ssp():
    from speech_signal_processing_amd import api, d_vector
    return api, d_vector


def _case(seed, N, T, D, H, scale, in_std=3.0):
    rng = np.random.default_rng(seed)
    W, U, b = LO.keras_init(rng, D, H, scale)
    b = (b + 0.1 * rng.standard_normal(4 * H)).astype(np.float32)
    X = (in_std * rng.standard_normal((N, T, D))).astype(np.float32)
    return W, U, b, X


def _precondition(W, U, b, X, act, ref, what):
    f32 = LO.forward(W, U, b, X, act, dtype=np.float32)
    drift = float(np.abs(f32.astype(np.float64) - ref).max())
    assert drift <= PRECOND, "%s: float32 numpy is %.3e from float64 — the inputs, not the kernel, are out of range" % (what, drift)


@pytest.mark.parametrize("act", LO.ACTIVATIONS)
@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_reference_shape_vs_restatement(ssp, act, scale):
    """(98, 13) -> 128, the reference's network (d_vector.py:271-294); N = 1000 is neither a multiple of 16 nor of 64"""
    api, _ = ssp
    W, U, b, X = _case(11, 1000, 98, 13, 128, scale)
    ref = LO.forward(W, U, b, X, act)
    _precondition(W, U, b, X, act, ref, "reference shape")
    net = api.LstmForward(api.default_context(), W, U, b, act)
    got = net.forward(X)
    assert got.dtype == np.float32 and got.shape == (1000, 128)
    assert_feat_close(got, ref, "lstm 98x13->128 %s x%g" % (act, scale))
    nob = api.LstmForward(api.default_context(), W, U, None, act).forward(X[:50])
    assert_feat_close(nob, LO.forward(W, U, None, X[:50], act), "no bias")


@pytest.mark.parametrize("act", LO.ACTIVATIONS)
@pytest.mark.parametrize("H", [16, 64, 128])
@pytest.mark.parametrize("D", [13, 26, 39])
@pytest.mark.parametrize("T", [1, 2, 298])
def test_shapes_vs_restatement(ssp, T, D, H, act):
    api, _ = ssp
    N = 77 if T == 298 else 203
    W, U, b, X = _case(T * 1000 + D * 10 + H, N, T, D, H, 1.5)
    ref = LO.forward(W, U, b, X, act)
    _precondition(W, U, b, X, act, ref, "T %d D %d H %d" % (T, D, H))
    got = api.LstmForward(api.default_context(), W, U, b, act).forward(X)
    assert_feat_close(got, ref, "lstm T %d D %d H %d %s" % (T, D, H, act))


@pytest.mark.parametrize("act", LO.ACTIVATIONS)
@pytest.mark.parametrize("D,H", [(64, 48), (1, 112), (17, 32), (5, 96), (40, 80)])
def test_padded_shapes_vs_restatement(ssp, D, H, act):
    """units that do not fill the kernel's 1 / 2 / 4 / 8 tiles and inputs that do not fill a group of 16: the padding must stay inert"""
    api, _ = ssp
    W, U, b, X = _case(D * 7 + H, 131, 40, D, H, 1.5)
    ref = LO.forward(W, U, b, X, act)
    _precondition(W, U, b, X, act, ref, "D %d H %d" % (D, H))
    assert_feat_close(api.LstmForward(api.default_context(), W, U, b, act).forward(X), ref, "lstm D %d H %d %s" % (D, H, act))


@pytest.mark.parametrize("act", LO.ACTIVATIONS)
@pytest.mark.parametrize("T", [1, 2])
def test_large_weights_saturated_gates(ssp, T, act):
    """scale x 10 at T = 1, 2, where nothing can amplify: pre-activations of tens, gates pinned at 0 and 1, tanh at +-1"""
    api, _ = ssp
    W, U, b, X = _case(900 + T, 333, T, 13, 128, 10.0)
    ref = LO.forward(W, U, b, X, act)
    z = X[:, 0].astype(np.float64) @ W + b
    assert (np.abs(z) > 10).mean() > 0.05                       # saturation is present in the inputs (1 - tanh(10) = 4e-9)
    assert_feat_close(api.LstmForward(api.default_context(), W, U, b, act).forward(X), ref, "lstm x10 T %d %s" % (T, act))


def test_unsupported_shapes_raise(ssp):
    api, _ = ssp
    ctx = api.default_context()
    with pytest.raises(NotImplementedError):
        api.LstmForward(ctx, np.zeros((13, 400), np.float32), np.zeros((100, 400), np.float32), None, "sigmoid")
    with pytest.raises(NotImplementedError):
        api.LstmForward(ctx, np.zeros((65, 64), np.float32), np.zeros((16, 64), np.float32), None, "sigmoid")
    with pytest.raises(ValueError):
        api.LstmForward(ctx, np.zeros((13, 64), np.float32), np.zeros((16, 64), np.float32), None, "tanh")
    net = api.LstmForward(ctx, np.zeros((13, 64), np.float32), np.zeros((16, 64), np.float32), None, "sigmoid")
    with pytest.raises(ValueError):
        net.forward(np.zeros((4, 5, 12), np.float32))
    with pytest.raises(ValueError):
        net.forward(np.zeros((20, 13), np.float32))             # 2-D without segments
    assert net.forward(np.zeros((0, 5, 13), np.float32)).shape == (0, 16)


@pytest.mark.parametrize("act", LO.ACTIVATIONS)
def test_ragged_batch_bit_equal_to_sequences_alone(ssp, act):
    """lengths 0 ... 300 shuffled in one call: every sequence's bits equal the sequence run alone; the host-pointer route equals the
    device-pointer route; segments that do not start at row 0 address the same rows"""
    import torch
    api, _ = ssp
    ctx = api.default_context()
    rng = np.random.default_rng(77)
    W, U, b = LO.keras_init(rng, 13, 128, 1.5)
    lengths = rng.permutation(301)
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    feats = (3 * rng.standard_normal((off[-1], 13))).astype(np.float32)
    net = api.LstmForward(ctx, W, U, b, act)
    seg = api.Segments(ctx, off)
    got = net.forward(feats, seg)
    assert got.shape == (301, 128) and not got[lengths == 0].any()
    ref = LO.forward_ragged(W, U, b, feats, off, act)
    _precond = LO.forward_ragged(W, U, b, feats, off, act, dtype=np.float32)
    assert np.abs(_precond - ref).max() <= PRECOND
    assert_feat_close(got, ref, "ragged %s" % act)
    dev = net.forward(torch.from_numpy(feats).cuda(), seg)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)                     # device route == host route, bit for bit
    for s in range(301):
        alone = net.forward(feats[off[s]:off[s + 1]][None]) if lengths[s] else np.zeros((1, 128), np.float32)
        assert np.array_equal(alone[0], got[s]), "sequence %d (length %d) depends on its batch" % (s, lengths[s])
    shifted = net.forward(np.concatenate((np.full((5, 13), np.nan, np.float32), feats)), api.Segments(ctx, off + 5))
    assert np.array_equal(shifted, got)
    # a NaN sequence poisons itself only
    bad = feats.copy()
    s_bad = int(np.argmax(lengths == 150))
    bad[off[s_bad] + 3, 2] = np.nan
    gb = net.forward(bad, seg)
    assert np.isnan(gb[s_bad]).any() and np.array_equal(np.delete(gb, s_bad, 0), np.delete(got, s_bad, 0))


def _speaker_chunks(rng, S, per, T=98, D=13):
    lab = np.repeat(np.arange(S), per)
    protos = 2.0 * rng.standard_normal((S, 1, D))
    X = (protos[lab] + 1.5 * rng.standard_normal((S * per, T, D))).astype(np.float32)
    p = rng.permutation(S * per)
    return X[p], lab[p]


@pytest.mark.parametrize("act", LO.ACTIVATIONS)
def test_enroll_eval_test_with_lstm_by_name(ssp, tmp_path, act):
    """nn_model.test / enroll / eval (d_vector.py:296-361) with an LstmNet registered under 'lstm', then saved as d_vector_lstm.npz and
    loaded again by the default model name; decisions equal the restatement's"""
    api, d_vector = ssp
    rng = np.random.default_rng(21)
    W, U, b = LO.keras_init(rng, 13, 128, 1.5)
    S, per = 4, 30
    X, lab = _speaker_chunks(rng, S, per)
    Y = np.eye(S)[lab]
    emb = LO.forward(W, U, b, X, act)
    avg = np.stack([emb[::2][lab[::2] == s].mean(0) for s in range(S)])

    def cosd(a, c):
        return 1 - (a @ c.T) / (np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(c, axis=1)[None])
    dist = cosd(emb[1::2], avg)
    srt = np.sort(dist, axis=1)
    assert (srt[:, 1] - srt[:, 0]).min() > 1e-3                    # no near-tie: the arg-min is decided far outside the tolerance
    ref_pred = dist.argmin(1)
    ref_acc = (ref_pred == lab[1::2]).mean()
    assert ref_acc > 0.5

    net = d_vector.LstmNet(W, U, b, recurrent_activation=act)
    assert net.input_dim == 13 and net.output_dim == 128
    assert_feat_close(net.predict(X), emb, "LstmNet.predict 3-D")
    assert np.array_equal(net.predict(X.reshape(len(X), -1)), net.predict(X))           # (N, T * D), as load_data(reshape=True) gives
    old_dir = d_vector.MODEL_DIR
    try:
        for round_ in ("registered", "reloaded"):
            if round_ == "registered":
                d_vector.register_model('lstm', net)
            else:
                d_vector.save_model(net, 'lstm', model_dir=str(tmp_path))
                d_vector._MODELS.pop('lstm', None)
                d_vector.MODEL_DIR = str(tmp_path)
            m = d_vector.nn_model(store=str(tmp_path / ("d_vector_%s.pkl" % round_)))
            acc = m.test(X[::2], Y[::2], X[1::2], Y[1::2], model_name='lstm')
            assert acc == ref_acc, (round_, acc, ref_acc)
            np.testing.assert_allclose(m.centroids_, avg, atol=1e-4)
            for s in range(S):
                m.enroll(X[::2][lab[::2] == s], 'spk%d' % s)                              # default model_name = 'lstm'
            enrolled = np.stack([emb[::2][lab[::2] == s].mean(0) for s in range(S)])
            d_en = cosd(emb[1::2], enrolled)
            for i in range(0, len(d_en), 7):
                want = 'spk%d' % d_en[i].argmin() if d_en[i].min() < 1 else None
                assert m.eval(X[1::2][i:i + 1]) == want, (round_, i)                    # (1, T, D) -> reshape(1, -1) inside eval
            loaded = d_vector.load_model('lstm')
            assert isinstance(loaded, d_vector.LstmNet) and loaded.recurrent_activation == act
            assert np.array_equal(loaded.predict(X[:20]), net.predict(X[:20]))
    finally:
        d_vector.MODEL_DIR = old_dir
        d_vector._MODELS.pop('lstm', None)


def test_npz_round_trip_of_both_kinds(ssp, tmp_path):
    """a file without `kind` stays a DenseNet (also under the name 'lstm'); an LstmNet's file says kind = 'lstm' and its activation"""
    api, d_vector = ssp
    rng = np.random.default_rng(2)
    layers = [((rng.standard_normal((40, 32)) / 6).astype(np.float32), rng.standard_normal(32).astype(np.float32) * 0.1, 'relu'),
              ((rng.standard_normal((32, 16)) / 5).astype(np.float32), None, 'linear')]
    dense = d_vector.DenseNet(layers)
    W, U, b = LO.keras_init(rng, 26, 64)
    X = rng.standard_normal((9, 40)).astype(np.float32)
    S = rng.standard_normal((9, 12, 26)).astype(np.float32)
    try:
        d_vector.save_model(dense, 'lstm', model_dir=str(tmp_path))
        assert "kind" not in np.load(str(tmp_path / "d_vector_lstm.npz")).files
        back = d_vector.load_model('lstm', model_dir=str(tmp_path))
        assert isinstance(back, d_vector.DenseNet) and np.array_equal(back.predict(X), dense.predict(X))
        d_vector._MODELS.pop('lstm', None)
        for act, bias in (("hard_sigmoid", b), ("sigmoid", None)):
            net = d_vector.LstmNet(W, U, bias, recurrent_activation=act)
            d_vector.save_model(net, 'rec_' + act, model_dir=str(tmp_path))
            z = np.load(str(tmp_path / ("d_vector_rec_%s.npz" % act)))
            assert str(z["kind"]) == "lstm" and str(z["recurrent_activation"]) == act
            back = d_vector.load_model('rec_' + act, model_dir=str(tmp_path))
            assert isinstance(back, d_vector.LstmNet) and back.recurrent_activation == act and (back.b is None) == (bias is None)
            assert np.array_equal(back.predict(S), net.predict(S))
    finally:
        for k in ('lstm', 'rec_hard_sigmoid', 'rec_sigmoid'):
            d_vector._MODELS.pop(k, None)


def test_from_keras_duck_types_the_layer(ssp):
    api, d_vector = ssp
    W, U, b = LO.keras_init(np.random.default_rng(4), 13, 32)

    def hard_sigmoid(x):
        return x

    class Layer:
        recurrent_activation = staticmethod(hard_sigmoid)

        def get_weights(self):
            return [W, U, b]
    net = d_vector.LstmNet.from_keras(Layer())
    X = np.random.default_rng(5).standard_normal((5, 9, 13)).astype(np.float32)
    assert net.recurrent_activation == "hard_sigmoid"
    assert_feat_close(net.predict(X), LO.forward(W, U, b, X, "hard_sigmoid"), "from_keras")


def test_resident_path_equals_host_hopped_path(ssp):
    """MFCC -> LSTM -> identify with every array staying on the device equals the same three steps through host arrays, bit for bit"""
    import torch
    from conftest import synth_audio
    api, d_vector = ssp
    from speech_signal_processing_amd import frontend
    sr, n_chunks = 16000, 70
    plan = api.MfccPlan(api.default_context(), frontend.preset_sidekit(fs=sr))
    plan.set_reproducible(True)
    chunks = [synth_audio(u, sr, sr) for u in range(n_chunks)]
    seg = api.Segments.from_lengths(plan.ctx, [sr] * n_chunks)
    fseg = plan.frame_segments(seg)
    assert int(fseg.offsets[1]) == 98 and plan.d_out == 13
    flat = np.concatenate(chunks)
    rng = np.random.default_rng(8)
    W, U, b = LO.keras_init(rng, 13, 128)
    W = (W / 30).astype(np.float32)                                  # (raw cepstra are tens to hundreds: keep the gates in range)
    net = d_vector.LstmNet(W, U, b, recurrent_activation="sigmoid")
    feats_h = plan.run(flat, seg, fseg)
    emb_h = net.predict_ragged(feats_h, fseg)
    cents = np.stack([emb_h[s::10].mean(0) for s in range(10)]).astype(np.float32)
    ctx = api.default_context()
    pred_h = np.asarray(api.cosine_identify(ctx, emb_h, cents, minval=False)["argmin"])
    feats_d = plan.run(torch.from_numpy(flat).cuda(), seg, fseg)
    emb_d = net.predict_ragged(feats_d, fseg)
    assert emb_d.is_cuda and emb_d.shape == (n_chunks, 128)
    pred_d = api.cosine_identify(ctx, emb_d, torch.from_numpy(cents).cuda(), minval=False)["argmin"].cpu().numpy()
    assert np.array_equal(feats_d.cpu().numpy(), np.asarray(feats_h))
    assert np.array_equal(emb_d.cpu().numpy(), emb_h) and np.array_equal(pred_d, pred_h)
    assert np.isfinite(emb_h).all() and np.ptp(emb_h, axis=0).max() > 1e-3
    # the (N, 98, 13) view of the same rows is the same computation
    assert np.array_equal(net.predict(np.asarray(feats_h).reshape(n_chunks, 98, 13)), emb_h)
    X3 = np.asarray(feats_h).reshape(n_chunks, 98, 13)
    ref = LO.forward(W, U, b, X3, "sigmoid")
    _precondition(W, U, b, X3, "sigmoid", ref, "MFCC -> LSTM")
    assert_feat_close(emb_h, ref, "MFCC -> LSTM")
