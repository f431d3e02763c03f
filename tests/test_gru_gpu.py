"""GPU tests of the conv + GRU d-vector network (run with -m gpu on an MI355X): the convolution, the per-step MFMA recurrence through
api.GruForward, and d_vector.ConvGruNet against the float64 restatement tests/gru_oracle.py.

Tolerance: the project's feature rule (tests/test_gpu_parity.py assert_feat_close, north star 1e-4):
    max |gpu - ref| <= 1e-4 max(1, max |ref|)
Input condition: a recurrent network with large recurrent weights is chaotic and float32 then leaves float64 whatever the kernel does.
Multi-step cases draw weights at Keras' own initialisation scale x <= 2 and first assert, on the CPU, that the float32 restatement is
within 1e-5 of the float64 one on the very inputs of the case.  Large weights (x 10, saturated gates) are covered at T <= 2 only.
Unpinned: the reference holds no GRU weights or outputs and Keras is not installed; the restatement is corroborated against
torch.nn.GRU and torch's conv2d in tests/test_gru_host.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_oracle as GO  # noqa: E402

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


def _precondition(f32, ref, what):
    drift = float(np.abs(np.asarray(f32, np.float64) - ref).max())
    print("[precondition] %s: float32 restatement %.3e from float64" % (what, drift))
    assert drift <= PRECOND, "%s: float32 numpy is %.3e from float64 — the inputs, not the kernel, are out of range" % (what, drift)


# ---- one GRU layer ------------------------------------------------------------------------------------------------------------------

LAYER_SHAPES = [(1, 7, 16, 1), (2, 448, 48, 37), (5, 449, 1008, 37), (9, 100, 1024, 203), (21, 13, 80, 131)]   # (T, d_in, H, N)


@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
@pytest.mark.parametrize("T,d_in,H,N", LAYER_SHAPES)
def test_gru_layer_sequence_and_mean_vs_restatement(ssp, T, d_in, H, N, act, reset_after):
    """state and input widths that do not fill a tile (16, 48, 80, 1008; 7, 449), batches that do not fill one (1, 37, 131, 203), more than
    one workgroup along both axes (1024 units, 203 chunks), and the zero-state-only step (T = 1)"""
    api, _ = ssp
    rng = np.random.default_rng(T * 100000 + d_in * 100 + H + 7 * reset_after)
    W, U, b = GO.gru_init(rng, d_in, H, reset_after, 1.5)
    X = (3 * rng.standard_normal((N, T, d_in))).astype(np.float32)
    ref = GO.gru(W, U, b, X, act, reset_after)
    what = "gru T %d d_in %d H %d N %d %s reset_after %d" % (T, d_in, H, N, act, reset_after)
    if T > 1:
        _precondition(GO.gru(W, U, b, X, act, reset_after, dtype=np.float32), ref, what)
    net = api.GruForward(api.default_context(), W, U, b, act, reset_after)
    seq = net.forward(X)
    assert seq.dtype == np.float32 and seq.shape == (N, T, H)
    assert_feat_close(seq, ref, what + " sequence")
    mean = net.forward(X, mean=True)
    assert mean.dtype == np.float32 and mean.shape == (N, H)
    assert_feat_close(mean, GO.time_mean(ref), what + " mean")


@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
def test_gru_layer_without_bias(ssp, act, reset_after):
    api, _ = ssp
    rng = np.random.default_rng(5)
    W, U, _ = GO.gru_init(rng, 100, 80, reset_after, 1.5, bias=False)
    X = (3 * rng.standard_normal((37, 9, 100))).astype(np.float32)
    ref = GO.gru(W, U, None, X, act, reset_after)
    _precondition(GO.gru(W, U, None, X, act, reset_after, dtype=np.float32), ref, "no bias")
    assert_feat_close(api.GruForward(api.default_context(), W, U, None, act, reset_after).forward(X), ref, "gru no bias %s %d" % (act, reset_after))


@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
@pytest.mark.parametrize("T", [1, 2])
def test_gru_layer_large_weights_saturated_gates(ssp, T, act, reset_after):
    """scale x 10 at T = 1, 2, where nothing can amplify: pre-activations of tens, gates pinned at 0 and 1, tanh at +-1"""
    api, _ = ssp
    rng = np.random.default_rng(900 + T)
    W, U, b = GO.gru_init(rng, 448, 48, reset_after, 10.0)
    X = (3 * rng.standard_normal((37, T, 448))).astype(np.float32)
    ref = GO.gru(W, U, b, X, act, reset_after)
    assert np.abs(ref).max() > 0.999                                # saturated
    assert_feat_close(api.GruForward(api.default_context(), W, U, b, act, reset_after).forward(X), ref, "gru x10 T %d %s %d" % (T, act, reset_after))


# ---- the convolution ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [64, 16, 1])
def test_convolution_vs_restatement(ssp, F):
    """the host test's grid: (98, 13), (97, 14), (1, 1), (5, 3) x kernels 5, 3, 1 x strides (2, 2), (1, 1), (2, 1)"""
    api, _ = ssp
    ctx = api.default_context()
    rng = np.random.default_rng(F)
    worst = 0.0
    for T, D in ((98, 13), (97, 14), (1, 1), (5, 3)):
        X = (3 * rng.standard_normal((3, T, D))).astype(np.float32)
        for k in (5, 3, 1):
            K = GO.glorot(rng, (k, k, 1, F), k * k, k * k * F)
            bc = (0.1 * rng.standard_normal(F)).astype(np.float32)
            for strides in ((2, 2), (1, 1), (2, 1)):
                ref = GO.conv2d_same(X, K, bc, strides)
                got = api.conv2d_same(ctx, X, K, bc, strides)
                assert got.dtype == np.float32
                assert got.shape == ref.shape, (T, D, k, strides)
                err = float(np.abs(got - ref).max())
                worst = max(worst, err)
                assert err <= FEAT_TOL * max(1.0, np.abs(ref).max()), (T, D, k, strides, err)
    print("[measured] conv F %d: max abs err %.3e" % (F, worst))
    nob = api.conv2d_same(ctx, X, K, None, (2, 1))
    assert np.abs(nob - GO.conv2d_same(X, K, None, (2, 1))).max() <= FEAT_TOL


def test_l2_normalize_vs_restatement(ssp):
    api, _ = ssp
    rng = np.random.default_rng(2)
    y = rng.standard_normal((131, 512)).astype(np.float32)
    y[3] = 0.0
    y[4] *= 1e-10
    got = api.l2_normalize(api.default_context(), y)
    assert_feat_close(got, GO.l2_normalize(y.astype(np.float64)), "l2_normalize")
    assert not got[3].any()
    odd = rng.standard_normal((5, 33)).astype(np.float32)
    assert_feat_close(api.l2_normalize(api.default_context(), odd), GO.l2_normalize(odd.astype(np.float64)), "l2_normalize d 33")


# ---- the network --------------------------------------------------------------------------------------------------------------------

def _net_case(T, D, F, H, E, N, reset_after, seed, scale):
    rng = np.random.default_rng(seed)
    conv, grus, dense = GO.network_init(rng, T, D, F, H, E, 3, reset_after, scale=scale)
    X = (3 * rng.standard_normal((N, T, D))).astype(np.float32)
    return conv, grus, dense, X


@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
def test_reference_network_vs_restatement(ssp, act, reset_after):
    """(98, 13) -> Conv2D(64, 5x5, stride 2) -> 3 x GRU(1024) -> mean -> Dense(512) -> L2 (d_vector.py:213-269), N = 37"""
    _, d_vector = ssp
    conv, grus, dense, X = _net_case(98, 13, 64, 1024, 512, 37, reset_after, 31, 1.5)
    emb, mean = GO.network(conv, grus, dense, X, act, reset_after)
    e32, m32 = GO.network(conv, grus, dense, X, act, reset_after, dtype=np.float32)
    _precondition(m32, mean, "reference network mean")
    _precondition(e32, emb, "reference network embedding")
    net = d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after)
    parts = {}
    got = net.predict(X, parts=parts)
    assert got.dtype == np.float32 and got.shape == (37, 512) and net.output_dim == 512
    assert_feat_close(parts["mean"], mean, "conv+gru 98x13 %s reset_after %d: mean of the last GRU" % (act, reset_after))
    assert_feat_close(got, emb, "conv+gru 98x13 %s reset_after %d: embedding" % (act, reset_after))
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= 1e-5


@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
def test_small_network_vs_restatement(ssp, act, reset_after):
    """16 filters, H = 48 (three unit tiles: the padding tile of an odd count), E = 32, (21, 14) input: what the big one's full tiles hide"""
    _, d_vector = ssp
    conv, grus, dense, X = _net_case(21, 14, 16, 48, 32, 131, reset_after, 41, 2.0)
    emb, mean = GO.network(conv, grus, dense, X, act, reset_after)
    e32, m32 = GO.network(conv, grus, dense, X, act, reset_after, dtype=np.float32)
    _precondition(m32, mean, "small network mean")
    _precondition(e32, emb, "small network embedding")
    net = d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after)
    parts = {}
    got = net.predict(X, parts=parts)
    assert_feat_close(parts["mean"], mean, "small conv+gru %s %d: mean" % (act, reset_after))
    assert_feat_close(got, emb, "small conv+gru %s %d: embedding" % (act, reset_after))


# ---- bit equality -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
def test_network_bits_do_not_depend_on_batch_or_slab(ssp, act, reset_after):
    """N = 203 in one call against the same chunks one at a time (a sample of them), in calls of 50, and with the workspace forced low
    enough for four slabs; the torch route equals the numpy route; a NaN chunk poisons only itself"""
    import torch
    _, d_vector = ssp
    conv, grus, dense, X = _net_case(21, 14, 16, 48, 32, 203, reset_after, 51, 1.5)
    net = d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after)
    whole = net.predict(X)
    assert net.last_slab == 203
    assert np.isfinite(whole).all()
    for i in (0, 1, 49, 63, 64, 127, 202):
        assert np.array_equal(net.predict(X[i:i + 1]), whole[i:i + 1]), i
    assert np.array_equal(np.concatenate([net.predict(X[i:i + 50]) for i in range(0, 203, 50)]), whole)
    _, per, _ = net._slab(21, 14)
    low = d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after, workspace_bytes=per * 60)
    assert np.array_equal(low.predict(X), whole)
    assert low.last_slab == 60                                     # 60 + 60 + 60 + 23
    dev = net.predict(torch.from_numpy(X).cuda())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), whole)
    bad = X.copy()
    bad[70, 3, 2] = np.nan
    pois = net.predict(bad)
    assert np.isnan(pois[70]).all()
    keep = np.arange(203) != 70
    assert np.array_equal(pois[keep], whole[keep])


@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
def test_layer_bits_do_not_depend_on_slab_or_route(ssp, act, reset_after):
    """api.GruForward alone: the library's own slabs (workspace cap forced to 50 chunks) and the host route (staged input, sequence copied
    back) against the device route (sequence written in place)"""
    import torch
    api, _ = ssp
    rng = np.random.default_rng(61)
    T, d_in, H, N = 9, 100, 80, 203
    W, U, b = GO.gru_init(rng, d_in, H, reset_after, 1.5)
    X = (3 * rng.standard_normal((N, T, d_in))).astype(np.float32)
    net = api.GruForward(api.Context.for_torch(), W, U, b, act, reset_after)
    host = net.forward(X)
    assert net.last_slab == N
    dev = net.forward(torch.from_numpy(X).cuda())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    per_chunk_host = 4 * (T * 3 * H + T * H + (0 if reset_after else 2 * H))
    net.set_workspace(per_chunk_host * 50)
    assert np.array_equal(net.forward(X), host) and net.last_slab == 50
    assert np.array_equal(net.forward(X, mean=True), net.set_workspace(1 << 30).forward(X, mean=True))
    assert np.array_equal(net.forward(torch.from_numpy(X).cuda(), mean=True).cpu().numpy(), net.forward(X, mean=True))
    assert np.array_equal(net.forward(X[100:101]), host[100:101])


# ---- model handling -----------------------------------------------------------------------------------------------------------------

def _speaker_chunks(rng, S, per, T, D):
    """chunks of S synthetic speakers: a speaker's own (T, D) pattern plus noise"""
    pat = 3 * rng.standard_normal((S, T, D))
    lab = np.repeat(np.arange(S), per)
    X = pat[lab] + 0.7 * rng.standard_normal((S * per, T, D))
    p = rng.permutation(S * per)
    return X[p].astype(np.float32), lab[p]


@functools.lru_cache(maxsize=None)
def _model_case(act, reset_after):
    rng = np.random.default_rng(71)
    T, D, S, per = 21, 14, 4, 16
    conv, grus, dense = GO.network_init(rng, T, D, 16, 48, 32, 2, reset_after, scale=1.5)
    X, lab = _speaker_chunks(rng, S, per, T, D)
    emb, _ = GO.network(conv, grus, dense, X, act, reset_after)
    return conv, grus, dense, X, lab, emb


@pytest.mark.parametrize("act,reset_after", GO.VARIANTS)
def test_enroll_eval_test_with_conv_gru_by_name(ssp, tmp_path, act, reset_after):
    """nn_model.test / enroll / eval (d_vector.py:296-361) with a ConvGruNet registered under 'gru', then saved as d_vector_gru.npz and
    loaded again by name; decisions equal the restatement's"""
    _, d_vector = ssp
    conv, grus, dense, X, lab, emb = _model_case(act, reset_after)
    S, T, D = 4, 21, 14
    Y = np.eye(S)[lab]
    avg = np.stack([emb[::2][lab[::2] == s].mean(0) for s in range(S)])

    def cosd(a, c):
        return 1 - (a @ c.T) / (np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(c, axis=1)[None])
    dist = cosd(emb[1::2], avg)
    srt = np.sort(dist, axis=1)
    assert (srt[:, 1] - srt[:, 0]).min() > 1e-3                    # no near-tie: the arg-min is decided far outside the tolerance
    assert np.abs(srt[:, 0] - 1).min() > 1e-3                      # ... and so is eval's `distance < 1`
    ref_acc = (dist.argmin(1) == lab[1::2]).mean()

    net = d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after, input_shape=(T, D))
    base = net.predict(X)
    assert_feat_close(base, emb, "ConvGruNet.predict 3-D")
    assert np.array_equal(net.predict(X[..., None]), base)                              # (N, T, D, 1), what d_vector.py:389 hands over
    assert np.array_equal(net.predict(X.reshape(len(X), -1)), base)                     # (N, T * D), eval's reshape(1, -1)
    old_dir = d_vector.MODEL_DIR
    try:
        for round_ in ("registered", "reloaded"):
            if round_ == "registered":
                d_vector.register_model('gru', net)
            else:
                d_vector.save_model(net, 'gru', model_dir=str(tmp_path))
                d_vector._MODELS.pop('gru', None)
                d_vector.MODEL_DIR = str(tmp_path)
                z = np.load(str(tmp_path / "d_vector_gru.npz"))
                assert str(z["kind"]) == "conv_gru" and str(z["recurrent_activation"]) == act and int(z["reset_after"]) == int(reset_after)
                assert tuple(z["strides"]) == (2, 2)
            m = d_vector.nn_model(store=str(tmp_path / ("d_vector_%s.pkl" % round_)))
            acc = m.test(X[::2], Y[::2], X[1::2], Y[1::2], model_name='gru')
            assert acc == ref_acc, (round_, acc, ref_acc)
            np.testing.assert_allclose(m.centroids_, avg, atol=1e-4)
            for s in range(S):
                m.enroll(X[::2][lab[::2] == s], 'spk%d' % s, model_name='gru')
            for i in range(0, len(dist), 5):
                want = 'spk%d' % dist[i].argmin() if dist[i].min() < 1 else None
                assert m.eval(X[1::2][i:i + 1], model_name='gru') == want, (round_, i)
            loaded = d_vector.load_model('gru')
            assert isinstance(loaded, d_vector.ConvGruNet)
            assert loaded.recurrent_activation == act and loaded.reset_after == reset_after and loaded.input_shape == (T, D)
            assert np.array_equal(loaded.predict(X[:20]), base[:20])
    finally:
        d_vector.MODEL_DIR = old_dir
        d_vector._MODELS.pop('gru', None)


def test_existing_model_kinds_still_load(ssp, tmp_path):
    _, d_vector = ssp
    rng = np.random.default_rng(3)
    dense = d_vector.DenseNet([(rng.standard_normal((20, 16)).astype(np.float32), None, 'relu')])
    import lstm_oracle as LO
    W, U, b = LO.keras_init(rng, 13, 16)
    lstm = d_vector.LstmNet(W, U, b, recurrent_activation="sigmoid")
    try:
        d_vector.save_model(dense, 'k_dense', model_dir=str(tmp_path))
        d_vector.save_model(lstm, 'k_lstm', model_dir=str(tmp_path))
        assert isinstance(d_vector.load_model('k_dense', model_dir=str(tmp_path)), d_vector.DenseNet)
        assert isinstance(d_vector.load_model('k_lstm', model_dir=str(tmp_path)), d_vector.LstmNet)
    finally:
        d_vector._MODELS.pop('k_dense', None)
        d_vector._MODELS.pop('k_lstm', None)


def test_from_keras_duck_types_the_model(ssp):
    _, d_vector = ssp
    conv, grus, dense, X, _, emb = _model_case("sigmoid", True)

    class Layer:
        def __init__(self, weights, **kw):
            self._w = weights
            self.__dict__.update(kw)

        def get_weights(self):
            return list(self._w)

    class Model:
        layers = [Layer([conv[0], conv[1]], strides=(2, 2)), Layer([]), Layer(grus[0]), Layer(grus[1]), Layer([]), Layer(dense), Layer([])]

    net = d_vector.ConvGruNet.from_keras(Model(), recurrent_activation="sigmoid", reset_after=True)
    assert_feat_close(net.predict(X[:9]), emb[:9], "from_keras")
    with pytest.raises(TypeError):
        d_vector.ConvGruNet.from_keras(Model())
    with pytest.raises(ValueError):
        d_vector.ConvGruNet.from_keras(type("M", (), {"layers": [Layer(grus[0])]})(), recurrent_activation="sigmoid", reset_after=True)


def test_unsupported_shapes_raise_and_empty_batch(ssp):
    api, d_vector = ssp
    ctx = api.default_context()
    for H in (24, 1040):
        with pytest.raises(NotImplementedError):
            api.GruForward(ctx, np.zeros((7, 3 * H), np.float32), np.zeros((H, 3 * H), np.float32), None, "sigmoid", True)
    with pytest.raises(NotImplementedError):
        api.GruForward(ctx, np.zeros((4097, 48), np.float32), np.zeros((16, 48), np.float32), None, "sigmoid", True)
    with pytest.raises(ValueError):
        api.GruForward(ctx, np.zeros((7, 48), np.float32), np.zeros((16, 48), np.float32), np.zeros(48, np.float32), "sigmoid", True)   # bias (2, 3H)
    with pytest.raises(NotImplementedError):
        api.conv2d_same(ctx, np.zeros((1, 9, 9), np.float32), np.zeros((8, 8, 1, 4), np.float32))
    with pytest.raises(NotImplementedError):
        api.conv2d_same(ctx, np.zeros((1, 9, 9), np.float32), np.zeros((3, 3, 1, 257), np.float32))
    conv, grus, dense, X, _, _ = _model_case("sigmoid", True)
    net = d_vector.ConvGruNet(conv, grus, dense, recurrent_activation="sigmoid", reset_after=True)
    with pytest.raises(ValueError):
        net.predict(np.zeros((2, 21, 40), np.float32))             # 20 x 16 features per step, the first GRU takes 7 x 16
    with pytest.raises(ValueError):
        net.predict(np.zeros((2, 21 * 14), np.float32))            # flattened rows without input_shape
    out = net.predict(np.zeros((0, 21, 14), np.float32))
    assert out.shape == (0, 32) and out.dtype == np.float32
    g = api.GruForward(ctx, *grus[1], "sigmoid", True)
    assert g.forward(np.zeros((0, 5, 48), np.float32)).shape == (0, 5, 48)
    with pytest.raises(ValueError):
        g.forward(np.zeros((3, 0, 48), np.float32))                # T >= 1
