"""GPU tests of the x-vector block (run with -m gpu on an MI355X): ssp_tdnn_forward, ssp_stats_pool and ssp_xvector_forward against the
float64 restatement tests/xvector_oracle.py, the bit equalities the header promises (batch, slab, window, host / device), the
non-finite rules, the error codes, and xvector.Extractor as the ``embed`` of diarize.Diarizer.run.  Small shapes at the kernel's edges:
the frame-layer kernel works on tiles of 128 rows x 128 units with k-chunks of 32 inside one tap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xvector_oracle as XO          # noqa: E402
import test_xvector_host as XH       # noqa: E402  (network_case: the inputs the CPU precondition was checked on)

pytestmark = pytest.mark.gpu

FEAT_TOL = 1e-4
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def env():
    import torch
    from speech_signal_processing_amd import api
    return torch, api, api.default_context()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def feat_close(got, ref, what):
    """the project's feature rule: max |got - ref| <= 1e-4 max(1, max |ref|), same non-finite pattern"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), what + ": non-finite pattern differs"
    err = float(np.abs(got[fin] - ref[fin]).max())
    print("[measured] %s: max abs err %.3e (ref max %.3e)" % (what, err, np.abs(ref[fin]).max()))
    assert err <= FEAT_TOL * max(1.0, np.abs(ref[fin]).max()), what


# ============================================================================================================ one frame layer
UNITS = {16: (True, False), 100: (False, True), 512: (True, True), 1500: (False, False)}   # units -> (relu, scale / offset); 1500: no bias


@pytest.mark.parametrize("d_in", [1, 13, 39, 40, 512])
@pytest.mark.parametrize("taps,dil", [(1, 1), (3, 2), (3, 3), (5, 1)])
def test_single_layer_against_the_restatement(env, taps, dil, d_in):
    """|z - ref| <= 1.01 (K + 1) 2^-23 (sum |x| |w| + |b|), K = taps d_in, times |scale| plus 2^-23 |y| with scale / offset, on a ragged
    batch: an empty sequence, R - 1, R and R + 1 frames, and 127, 128 and 129 output rows (the tile's edges)"""
    _, api, ctx = env
    R = (taps - 1) * dil + 1
    counts = [R + 126, 0, R - 1, R, R + 128, R + 1, R + 127]
    rng = np.random.RandomState(1000 * taps + 100 * dil + d_in)
    X = rng.randn(sum(counts), d_in).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(counts)])
    for units, (relu, affine) in UNITS.items():
        fl, _ = XO.random_layers(rng, d_in, [(units, taps, dil, relu)], affine=affine)
        L = fl[0]
        if units == 1500:
            L["b"] = None
        Y, lens = api.tdnn_forward(ctx, X, counts, L["W"], L["b"], dilation=dil, relu=relu, scale=L.get("scale"), offset=L.get("offset"))
        assert Y.shape == (sum(counts), units) and lens.tolist() == [max(0, n - R + 1) for n in counts]
        worst = 0.0
        for i, n in enumerate(counts):
            x = X[off[i]:off[i + 1]]
            ref, bound = XO.layer(x, L), XO.layer_bound(x, L)
            got = Y[off[i]:off[i] + ref.shape[0]].astype(np.float64)
            if ref.size:
                worst = max(worst, float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
                assert (np.abs(got - ref) <= bound).all(), (units, i)
        print("[measured] layer taps=%d dil=%d d_in=%d units=%d: worst error / bound %.3f" % (taps, dil, d_in, units, worst))


# ===================================================================================================================== pooling
@pytest.mark.parametrize("dim", [1, 100, 1500])
def test_pooling(env, dim):
    """windows of 1, 2 and 77 rows (and none); a constant column gives exactly sqrt(var_floor); error <= 1e-4 max(1, max |ref|)"""
    _, api, ctx = env
    rng = np.random.RandomState(dim)
    counts = [90, 0, 5]
    X = (rng.randn(sum(counts), dim) * 3 + 1).astype(np.float32)
    X[:, 0] = np.float32(0.37)
    wins = np.array([[0, 0, 1], [0, 3, 5], [0, 10, 87], [0, 13, 90], [0, 7, 7], [2, 0, 5], [2, 4, 5]], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    for vf in (1e-10, 0.25):
        got = api.stats_pool(ctx, X, counts, wins, var_floor=vf)
        ref = np.stack([XO.pool(X[off[q] + a:off[q] + b], vf) for q, a, b in wins])
        feat_close(got, ref, "pool dim=%d floor=%g" % (dim, vf))
        assert np.isnan(got[4]).all()
        ok = [0, 1, 2, 3, 5, 6]
        assert (got[ok, dim] == np.float32(np.sqrt(np.float64(vf)))).all() and (got[ok, 0] == np.float32(0.37)).all()
    whole = api.stats_pool(ctx, X, counts)
    assert whole.shape == (3, 2 * dim) and np.isnan(whole[1]).all()
    feat_close(whole[[0, 2]], np.stack([XO.pool(X[:90]), XO.pool(X[90:])]), "pool dim=%d whole sequences" % dim)
    import torch
    dev = api.stats_pool(ctx, torch.from_numpy(X).cuda(), counts, wins)
    assert np.array_equal(bits(dev), bits(api.stats_pool(ctx, X, counts, wins)))


# ================================================================================================================= the network
@pytest.mark.parametrize("widths,n", [((64, 64, 64, 64, 100), 40), ((512, 512, 512, 512, 1500), 20)])
def test_network_against_the_restatement(env, widths, n):
    net, feats, counts = cached(("case", widths), lambda: XH.network_case(widths, n))
    ref = XO.network(feats, counts, net.frame_layers, net.segment_layers, net.var_floor)
    f32 = XO.network(feats, counts, net.frame_layers, net.segment_layers, net.var_floor, dtype=np.float32)
    drift = np.abs(f32.astype(np.float64) - ref).max() / max(1.0, np.abs(ref).max())
    print("[measured] float32 restatement drift: %.3g" % drift)
    assert drift <= 1e-5, "precondition: the float32 restatement leaves float64 on this case's inputs"
    got = net.embed(feats, counts)
    assert got.shape == (n, net.embed_width) and got.dtype == np.float32
    feat_close(got, ref, "network widths %s" % (widths,))
    assert np.array_equal(bits(net.predict([feats[:40], feats[40:40 + counts[1]]])), bits(got[:2]))


def _small():
    def make():
        from speech_signal_processing_amd import xvector
        rng = np.random.RandomState(77)
        net = xvector.XVectorNet.snyder(13, rng, widths=(48, 48, 48, 48, 72), embed=40)
        counts = [150, 14, 0, 15, 143, 16, 271, 40]     # below, at and above the receptive field; more than one tile of 128 rows
        feats = rng.randn(sum(counts), 13).astype(np.float32)
        return net, feats, counts, net.embed(feats, counts)
    return cached("small", make)


def test_bits_do_not_depend_on_the_batch(env):
    net, feats, counts, base = _small()
    off = np.concatenate([[0], np.cumsum(counts)])
    assert np.isnan(base[[1, 2]]).all() and np.isfinite(base[[0, 3, 4, 5, 6, 7]]).all()
    for i, n in enumerate(counts):
        alone = net.embed(feats[off[i]:off[i + 1]], [n])
        assert np.array_equal(bits(alone[0]), bits(base[i])), i


def test_bits_do_not_depend_on_the_slab(env):
    net, feats, counts, base = _small()
    fwd = net.forward_object()
    assert np.array_equal(bits(net.embed(feats, counts)), bits(base)) and fwd.last_slab == len(counts)
    try:
        fwd.set_workspace(1)     # every slab holds one sequence (one sequence always runs)
        capped = net.embed(feats, counts)
        assert fwd.last_slab == 1
        mid = net.set_workspace(2 * 4 * 72 * 300).embed(feats, counts)      # 300 rows: slabs of several whole sequences
        assert 1 < fwd.last_slab < len(counts)
    finally:
        fwd.set_workspace(2 << 30)
    assert np.array_equal(bits(capped), bits(base)) and np.array_equal(bits(mid), bits(base))


WINS = np.array([[0, 0, 150], [0, 0, 40], [0, 20, 60], [0, 40, 80], [0, 100, 150], [0, 50, 60], [3, 0, 15], [4, 1, 143], [4, 64, 128],
                 [6, 0, 100], [6, 50, 150], [6, 100, 200], [6, 150, 250], [6, 200, 271], [6, 120, 135], [7, 40, 40]], dtype=np.int64)


def test_windows_have_the_bits_of_stand_alone_extraction(env):
    net, feats, counts, base = _small()
    off = np.concatenate([[0], np.cumsum(counts)])
    got = net.embed(feats, counts, WINS)
    assert got.shape == (len(WINS), net.embed_width)
    chunks = [feats[off[q] + a:off[q] + b] for q, a, b in WINS]
    alone = net.embed(np.concatenate(chunks), [c.shape[0] for c in chunks])
    assert np.array_equal(bits(got), bits(alone))
    assert np.array_equal(bits(got[0]), bits(base[0])) and np.isnan(got[[5, 15]]).all() and np.isfinite(np.delete(got, [5, 15], axis=0)).all()
    ref = XO.network(feats, counts, net.frame_layers, net.segment_layers, net.var_floor, windows=WINS.tolist())
    feat_close(got, ref, "windowed network")
    fwd = net.forward_object()
    try:
        fwd.set_workspace(1)
        assert np.array_equal(bits(net.embed(feats, counts, WINS)), bits(got))     # windows of a slab's sequences: a run of the table
    finally:
        fwd.set_workspace(2 << 30)


def test_host_and_device_pointers_give_the_same_bits(env):
    torch, api, ctx = env
    net, feats, counts, base = _small()
    dev = net.embed(torch.from_numpy(feats).cuda(), counts)
    assert dev.is_cuda and np.array_equal(bits(dev), bits(base))
    devw = net.embed(torch.from_numpy(feats).cuda(), counts, WINS)
    assert np.array_equal(bits(devw), bits(net.embed(feats, counts, WINS)))
    L = net.frame_layers[1]
    X = np.random.RandomState(3).randn(200, 48).astype(np.float32)
    Yh, _ = api.tdnn_forward(ctx, X, [120, 80], L["W"], L["b"], dilation=L["dilation"], relu=True, scale=L["scale"], offset=L["offset"])
    t = lambda a: torch.from_numpy(a).cuda()    # noqa: E731
    Yd, _ = api.tdnn_forward(ctx, t(X), [120, 80], t(L["W"]), t(L["b"]), dilation=L["dilation"], relu=True, scale=t(L["scale"]), offset=t(L["offset"]))
    span = 2 * L["dilation"]
    for a, b in ((0, 120 - span), (120, 200 - span)):     # (the rows behind a sequence's valid ones are unspecified)
        assert np.array_equal(bits(Yd[a:b]), bits(Yh[a:b]))


# ============================================================================================================ non-finite input
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_reaches_exactly_the_rows_that_cover_it(env, bad):
    net, feats, counts, base = _small()
    off = np.concatenate([[0], np.cumsum(counts)])
    clean = net.embed(feats, counts, WINS)
    dirty = feats.copy()
    dirty[off[6] + 130, 5] = bad       # sequence 6, frame 130: inside windows [50, 150), [100, 200) and [120, 135) only
    got = net.embed(dirty, counts, WINS)
    ref = XO.network(dirty, counts, net.frame_layers, net.segment_layers, net.var_floor, windows=WINS.tolist())
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and np.array_equal(np.isnan(got), np.isnan(ref))
    hit = [10, 11, 14]
    assert np.isnan(got[hit]).all()
    keep = [w for w in range(len(WINS)) if w not in hit]
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    whole = net.embed(dirty, counts)
    assert np.isnan(whole[6]).all() and np.array_equal(bits(np.delete(whole, 6, axis=0)), bits(np.delete(base, 6, axis=0)))


# ================================================================================================================= error codes
def test_error_codes(env):
    _, api, ctx = env
    net, feats, counts, _ = _small()
    with pytest.raises(ValueError):
        net.embed(feats, counts, [[1, 0, 10], [0, 0, 20]])       # sequences must be non-decreasing
    with pytest.raises(ValueError):
        net.embed(feats, counts, [[0, 0, 151]])                  # past the end of its sequence
    with pytest.raises(ValueError):
        net.embed(feats, counts, [[0, 30, 20]])                  # first > end
    with pytest.raises(ValueError):
        net.embed(feats, counts, [[len(counts), 0, 0]])          # no such sequence
    with pytest.raises(ValueError):
        api.stats_pool(ctx, feats, counts, [[0, 0, 151]])
    X = np.zeros((40, 4), np.float32)
    with pytest.raises(NotImplementedError):
        api.tdnn_forward(ctx, X, [40], np.zeros((8, 17, 4), np.float32))                     # more than 16 taps
    with pytest.raises(NotImplementedError):
        api.tdnn_forward(ctx, X, [40], np.zeros((8, 3, 4), np.float32), dilation=513)        # (taps - 1) dilation above 1024
    with pytest.raises(NotImplementedError):
        api.tdnn_forward(ctx, np.zeros((2, 8193), np.float32), [2], np.zeros((8, 1, 8193), np.float32))
    with pytest.raises(NotImplementedError):
        api.XVectorForward(ctx, [{"W": np.zeros((8193, 1, 4), np.float32)}])
    with pytest.raises(ValueError):
        api.tdnn_forward(ctx, X, [40], np.zeros((8, 3, 4), np.float32), dilation=0)


# ================================================================================================ Extractor inside Diarizer.run
@pytest.mark.parametrize("norm", [None, "sliding"])
def test_extractor_is_an_embed_for_diarizer_run(env, norm):
    """the embed_windows route (features and frame layers once per recording) against the per-chunk route: the same labels; with
    norm=None the same BITS — every window starts on a multiple of the feature hop, so a chunk's frames are its recording's.  With
    norm='sliding' the two routes take the mean over different extents (the recording, the chunk) and their embeddings differ by a
    third of their length in float64 already (tests/test_xvector_host.py restates both routes and checks the labels' margin on this
    case): there the labels are compared, and each route's embeddings are held to its own restatement inside the margin that
    precondition proved harmless to the labels."""
    torch, api, ctx = env
    from speech_signal_processing_amd import VAD, diarize, frontend, xvector
    tables = frontend.preset_sidekit(fs=8000, nwin=0.032, shift=0.016, nlogfilt=24, nceps=13, maxfreq=4000.0)
    assert tables.cfg.win_len == 256 and tables.cfg.hop == 128      # the VAD's frame step: speech segments start on feature frames
    net = cached("diar-net", XH.diar_net)
    ex = xvector.Extractor(net, 8000, tables=tables, norm=norm, window=300)
    sigs = XO.diar_signals()
    d = diarize.Diarizer("cosine", threshold=0.0, ctx=ctx)
    via_windows = d.run(sigs, ex, win=3072, hop=1536, min_len=2560, n_speakers=[2, 2])
    via_chunks = d.run(sigs, lambda chunks: ex(chunks), win=3072, hop=1536, min_len=2560, n_speakers=[2, 2])
    assert len(via_windows) == 2 and all(np.array_equal(a, b) for a, b in zip(via_windows, via_chunks))
    assert all(set(a.tolist()) == {-1, 0, 1} for a in via_windows)
    masks = VAD.detect_batch(sigs)
    wins = [diarize.windows(VAD.speech_segments(m, len(x)), 3072, 1536, 2560) for m, x in zip(masks, sigs)]
    assert all(w.shape[0] >= 2 and (w[:, 0] % 128 == 0).all() for w in wins), [w.tolist() for w in wins]
    e_win = ex.embed_windows(sigs, wins).cpu().numpy()
    e_chunk = ex([x[a:b] for x, w in zip(sigs, wins) for a, b in w]).cpu().numpy()
    assert e_win.shape == e_chunk.shape == (sum(w.shape[0] for w in wins), 24) and np.isfinite(e_win).all() and np.isfinite(e_chunk).all()
    print("[measured] extractor norm=%s: max |windows - chunks| = %.3e (max |embedding| %.3e)" % (norm, np.abs(e_win - e_chunk).max(), np.abs(e_chunk).max()))
    if norm is None:
        assert np.array_equal(bits(e_win), bits(e_chunk))
    ref, counts = XO.extractor_routes(sigs, net, 300 if norm else None)
    assert counts == [w.shape[0] for w in wins]
    unit = lambda e: e / np.linalg.norm(e, axis=1, keepdims=True)      # noqa: E731
    for name, e in (("windows", e_win), ("chunks", e_chunk)):      # each route against its own restatement, inside the margin the host
        err = float(np.abs(unit(e.astype(np.float64)) - ref[name][0]).max())     # precondition proved harmless to the labels (1e-3)
        print("[measured] extractor norm=%s, route %s: unit embeddings within %.3e of the restatement" % (norm, name, err))
        assert err <= 1e-3, (norm, name, err)
    off = np.concatenate([[0], np.cumsum(counts)])
    for i, (g, w) in enumerate(zip(via_windows, wins)):
        assert np.array_equal(g, diarize.frame_labels(w, ref["windows"][1][off[i]:off[i + 1]], len(g), 128))
