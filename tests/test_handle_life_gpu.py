"""Birth and death of every handle class of the C ABI (csrc/handle.hpp): test_handles_may_outlive_their_context of test_gpu_parity.py
widened from five classes to all fourteen, at the smallest shapes the creates accept, and a create / close loop on one context.  The
failure paths of a create cannot be reached from here: tests/native/handle_life.cpp drives them on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSES = ["Segments", "MfccPlan", "GmmScorer", "GmmFullScorer", "MapScorer", "IvectorExtractor", "PldaScorer", "DnnForward", "LstmForward",
           "GruForward", "XVectorForward", "DnnTrainer", "LstmTrainer", "GruTrainer"]
K, D, M = 2, 4, 2             # mixtures, feature width, models
H, T, NC, B = 16, 2, 2, 2     # recurrent units, time steps, classes, batch


@pytest.fixture(scope="module")
def ssp():
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import api
    return pkg, api


def _tables(pkg):
    """the smallest MFCC dialect: a 64-point FFT over 8-sample windows, four positive filters, two cepstra"""
    from speech_signal_processing_amd import frontend as F
    rng = np.random.default_rng(1)
    cfg = F.MfccConfig(sample_rate=8000, win_len=8, hop=4, n_fft=64, n_filt=4, n_ceps=2, floor_mode=F.FLOOR_ADD_EPS, eps=1e-8)
    return F.MfccTables(cfg, np.hanning(10)[1:-1].astype(np.float32), rng.uniform(0.1, 1.0, (4, 33)).astype(np.float32),
                        F.dct2_ortho(4, 0, 2).astype(np.float32))


def _gmm(api, ctx, rng):
    return api.GmmScorer(ctx, np.stack([rng.dirichlet(np.ones(K))] * M), rng.standard_normal((M, K, D)), rng.uniform(0.5, 2, (M, K, D)), has_ubm=True)


def _makers(pkg, api):
    """class name -> make(ctx) -> (handle, call); call() runs one cheap entry point on the handle and returns its arrays"""
    rng = np.random.default_rng(0)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    feats, frames = f32(4, D), [3, 1]
    X3, X2, labels = f32(B, T, D), f32(B, D), np.array([0, 1], dtype=np.int32)
    W, U, Wg, Ug = 0.3 * f32(D, 4 * H), 0.3 * f32(H, 4 * H), 0.3 * f32(D, 3 * H), 0.3 * f32(H, 3 * H)
    w, mu, cv = rng.dirichlet(np.ones(K)), rng.standard_normal((K, D)), rng.uniform(0.5, 2, (K, D))
    chol = np.stack([np.eye(D) + 0.1 * np.triu(rng.standard_normal((D, D)), 1) for _ in range(M * K)]).reshape(M, K, D, D)

    def with_frames(make, call):   # a scorer over feats laid out by `frames`
        def go(ctx):
            h = make(ctx)

            def run():
                fseg = api.Segments.from_lengths(ctx, frames)
                out = call(h, fseg)
                fseg.close()
                return out
            return h, run
        return go

    def mfcc(ctx):
        plan = api.MfccPlan(ctx, _tables(pkg))

        def run():
            seg = api.Segments.from_lengths(ctx, [16, 8])
            fseg = plan.frame_segments(seg)
            out = plan.run(f32(24), seg, fseg)
            assert out.shape == (3 + 1, 2)
            fseg.close(), seg.close()
            return [out]
        return plan, run

    return {
        "Segments": lambda ctx: (lambda s: (s, lambda: [s.offsets.astype(np.float64)]))(api.Segments.from_lengths(ctx, [16, 8])),
        "MfccPlan": mfcc,
        "GmmScorer": with_frames(lambda ctx: _gmm(api, ctx, np.random.default_rng(7)), lambda h, fs: [h.score(feats, fs)["scores"]]),
        "GmmFullScorer": with_frames(lambda ctx: api.GmmFullScorer(ctx, np.stack([w] * M), np.stack([mu] * M), chol, has_ubm=True),
                                     lambda h, fs: [h.score(feats, fs)["scores"]]),
        "MapScorer": with_frames(lambda ctx: api.MapScorer(ctx, w, mu, cv, np.stack([mu + 0.1, mu - 0.1])),
                                 lambda h, fs: [h.score(feats, fs, top_c=1)["diff"]]),
        "IvectorExtractor": lambda ctx: (lambda h: (h, lambda: [h.extract(np.ones((1, K)), 0.1 * rng.standard_normal((1, K, D)))]))(
            api.IvectorExtractor(ctx, mu, cv, 0.1 * rng.standard_normal((K, D, 2)))),
        "PldaScorer": lambda ctx: (lambda h: (h, lambda: [h.score(X2, llr=True)["llr"]]))(
            api.PldaScorer(ctx, rng.uniform(0.5, 2, D), rng.standard_normal((2, D)), [1, 2])),
        "DnnForward": lambda ctx: (lambda h: (h, lambda: [h.forward(X2)]))(api.DnnForward(ctx, [(f32(2, D), None, True)])),
        "LstmForward": lambda ctx: (lambda h: (h, lambda: [h.forward(X3)]))(api.LstmForward(ctx, W, U, None, "sigmoid")),
        "GruForward": lambda ctx: (lambda h: (h, lambda: [h.forward(X3)]))(api.GruForward(ctx, Wg, Ug, None, "sigmoid", False)),
        "XVectorForward": lambda ctx: (lambda h: (h, lambda: [h.forward(feats, frames)]))(api.XVectorForward(ctx, [{"W": f32(2, 1, D)}])),
        "DnnTrainer": lambda ctx: (lambda h: (h, lambda: [np.array(h.evaluate(X2, labels), dtype=np.float64)]))(
            api.DnnTrainer(ctx, [(f32(D, NC), None, False, 0.0)], max_batch=B)),
        "LstmTrainer": lambda ctx: (lambda h: (h, lambda: [np.array(h.evaluate(X3, labels), dtype=np.float64)]))(
            api.LstmTrainer(ctx, W, U, None, f32(H, NC), None, T=T, recurrent_activation="sigmoid", max_batch=B)),
        "GruTrainer": lambda ctx: (lambda h: (h, lambda: [np.array(h.evaluate(X3, labels), dtype=np.float64)]))(
            api.GruTrainer(ctx, (np.ones((1, 1, 1, 1), np.float32), None, (1, 1)), [(Wg, Ug, None)], (f32(H, 2), None), (f32(2, NC), None), T=T, D=D,
                           recurrent_activation="sigmoid", reset_after=False, max_batch=B)),
    }


def test_every_handle_class_may_outlive_its_context(ssp):
    """Finalizers run in any order: each of the fourteen handle classes is created on a context that owns its stream, does one cheap
    call, and is closed AFTER the context, twice.  Nothing raises, and every result from before the close is finite."""
    pkg, api = ssp
    makers = _makers(pkg, api)
    assert sorted(makers) == sorted(CLASSES)
    ctx = api.Context(0)
    handles = []
    for name in CLASSES:
        h, call = makers[name](ctx)
        assert type(h).__name__ == name
        for a in call():
            a = np.asarray(a.cpu() if hasattr(a, "cpu") else a)
            assert a.size > 0 and np.isfinite(a).all(), name
        handles.append(h)
    ctx.close()                  # the context goes first ...
    for h in handles:            # ... then everything that was created on it ...
        h.close()
    for h in handles:            # ... and a second close is a no-op
        h.close()
    ctx.close()


def test_create_and_close_fifty_times_leaves_the_context_as_it_was(ssp):
    """Each class is created and closed 50 times on one context; a GmmScorer made afterwards on that context scores the first case's
    frames to the bits it gave before the loop."""
    pkg, api = ssp
    makers = _makers(pkg, api)
    ctx = api.Context(0)
    feats = np.random.default_rng(0).standard_normal((4, D)).astype(np.float32)

    def score():
        sc, fseg = _gmm(api, ctx, np.random.default_rng(7)), api.Segments.from_lengths(ctx, [3, 1])
        out = np.array(sc.score(feats, fseg)["scores"])
        sc.close(), fseg.close()
        return out

    before = score()
    assert np.isfinite(before).all()
    for name in CLASSES:
        for _ in range(50):
            makers[name](ctx)[0].close()
    assert np.array_equal(score(), before)
    ctx.close()
