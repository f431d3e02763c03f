"""Host tests of the x-vector block (no GPU): the restatement tests/xvector_oracle.py against torch.nn.functional.conv1d (dilation,
float64) and torch's population variance, windowed pooling against stand-alone extraction inside the restatement, fold_batchnorm
against torch's batch_norm in eval mode, the float32-against-float64 precondition of the GPU network cases, the bindings and the
Python surface."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xvector_oracle as XO   # noqa: E402

ENTRY_POINTS = {"ssp_tdnn_forward": 16, "ssp_stats_pool": 10, "ssp_xvector_create": 20, "ssp_xvector_destroy": 1, "ssp_xvector_info": 4,
                "ssp_xvector_set_workspace": 2, "ssp_xvector_last_slab": 2, "ssp_xvector_forward": 8}


def _torch_layer(x, L):
    import torch
    import torch.nn.functional as F
    W = torch.from_numpy(np.asarray(L["W"], dtype=np.float64))
    if W.ndim == 2:
        W = W[:, None, :]
    b = None if L.get("b") is None else torch.from_numpy(np.asarray(L["b"], dtype=np.float64))
    taps = W.shape[1]
    dil = int(L.get("dilation", 1))
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).T[None]          # (1, d_in, T)
    if xt.shape[2] < (taps - 1) * dil + 1:
        return np.zeros((0, W.shape[0]))
    z = F.conv1d(xt, W.permute(0, 2, 1).contiguous(), b, dilation=dil)[0].T    # (To, units)
    if L.get("relu"):
        z = torch.relu(z)
    if L.get("scale") is not None:
        z = z * torch.from_numpy(np.asarray(L["scale"], dtype=np.float64))
    if L.get("offset") is not None:
        z = z + torch.from_numpy(np.asarray(L["offset"], dtype=np.float64))
    return z.numpy()


@pytest.mark.parametrize("taps,dil", [(1, 1), (3, 2), (3, 3), (5, 1)])
def test_layer_equals_torch_conv1d(taps, dil):
    rng = np.random.RandomState(10 * taps + dil)
    for d_in, units, T in ((1, 16, 40), (13, 100, 31), (40, 7, (taps - 1) * dil + 1), (5, 3, (taps - 1) * dil)):
        fl, _ = XO.random_layers(rng, d_in, [(units, taps, dil, True)])
        x = rng.randn(T, d_in).astype(np.float32)
        got, ref = XO.layer(x, fl[0]), _torch_layer(x, fl[0])
        assert got.shape == ref.shape == (max(0, T - (taps - 1) * dil), units)
        assert got.size == 0 or np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_network_equals_torch():
    import torch
    rng = np.random.RandomState(5)
    spec = [(u, t, d, True) for u, (t, d) in zip((24, 24, 24, 24, 40), XO.SNYDER)]
    fl, sl = XO.random_layers(rng, 13, spec, segment=[(32, True), (20, False)])
    assert XO.receptive_field(fl) == 15
    counts = [40, 15, 14, 0, 33]
    feats = rng.randn(sum(counts), 13).astype(np.float32)
    got = XO.network(feats, counts, fl, sl, var_floor=1e-10)
    off = np.concatenate([[0], np.cumsum(counts)])
    for i, n in enumerate(counts):
        if n < 15:
            assert np.isnan(got[i]).all()
            continue
        h = feats[off[i]:off[i + 1]]
        for L in fl:
            h = _torch_layer(h, L)
        ht = torch.from_numpy(h)
        mean, var = ht.mean(0), ht.var(0, unbiased=False)
        p = torch.cat([mean, torch.sqrt(torch.clamp(var, min=1e-10))]).numpy()
        assert np.abs(XO.pool(h, 1e-10) - p).max() <= 1e-6 * max(1.0, np.abs(p).max())    # (the restatement rounds to float32 once)
        p64 = XO.pool(h, 1e-10).astype(np.float64)[None, :]
        for L in sl:
            p64 = _torch_layer(p64, L)
        assert np.abs(got[i] - p64[0]).max() <= 1e-12 * max(1.0, np.abs(p64).max())


def test_pooling_equals_torch_population_variance_and_floors_a_constant_column():
    import torch
    rng = np.random.RandomState(6)
    for n, C in ((1, 1), (2, 100), (77, 1500)):
        x = rng.randn(n, C).astype(np.float32) * 3 + 1
        x[:, 0] = 0.37
        p = XO.pool(x, 1e-10)
        xt = torch.from_numpy(x.astype(np.float64))
        ref = torch.cat([xt.mean(0), torch.sqrt(torch.clamp(xt.var(0, unbiased=False), min=1e-10))]).numpy()
        assert np.abs(p.astype(np.float64) - ref.astype(np.float32)).max() <= 1e-12 + 2.0 ** -23 * np.abs(ref).max()
        assert p[C] == np.float32(np.sqrt(np.float64(1e-10))) and p[0] == np.float32(0.37)
    assert np.isnan(XO.pool(np.zeros((0, 4), np.float32))).all()


def test_windowed_pooling_equals_stand_alone_extraction_exactly(monkeypatch):
    monkeypatch.setattr(XO, "ROWWISE", True)    # (a row's bits must not hang on the BLAS's choice of summation order by matrix shape)
    rng = np.random.RandomState(7)
    spec = [(u, t, d, True) for u, (t, d) in zip((16, 16, 16, 16, 24), XO.SNYDER)]
    fl, sl = XO.random_layers(rng, 13, spec, segment=[(12, False)])
    counts = [120, 60]
    feats = rng.randn(sum(counts), 13).astype(np.float32)
    wins = [(0, 0, 40), (0, 20, 60), (0, 40, 80), (0, 100, 120), (0, 50, 60), (1, 0, 60), (1, 45, 60), (1, 46, 60)]   # overlapping, a short one
    for dtype in (np.float64, np.float32):
        got = XO.network(feats, counts, fl, sl, windows=wins, dtype=dtype)
        off = [0, 120]
        for w, (q, a, b) in enumerate(wins):
            alone = XO.embed(feats[off[q] + a:off[q] + b], fl, sl, dtype=dtype)
            assert np.array_equal(got[w], alone, equal_nan=True), (dtype, w)
        assert np.isnan(got[4]).all() and np.isnan(got[7]).all() and np.isfinite(got[6]).all()


def test_fold_batchnorm_equals_torch_eval_batch_norm():
    import torch
    import torch.nn.functional as F
    from speech_signal_processing_amd import xvector
    rng = np.random.RandomState(8)
    C = 37
    mean, var = rng.randn(C), rng.uniform(0.1, 3.0, C)
    gamma, beta = rng.uniform(0.5, 2.0, C), rng.randn(C)
    x = rng.randn(50, C)
    for g, b in ((gamma, beta), (None, None)):
        scale, offset = xvector.fold_batchnorm(mean, var, g, b, eps=1e-3)
        assert scale.dtype == offset.dtype == np.float32
        ref = F.batch_norm(torch.from_numpy(x), torch.from_numpy(mean), torch.from_numpy(var), None if g is None else torch.from_numpy(g),
                           None if b is None else torch.from_numpy(b), training=False, eps=1e-3).numpy()
        got = x * scale.astype(np.float64) + offset.astype(np.float64)
        assert np.abs(got - ref).max() <= 4 * 2.0 ** -24 * (np.abs(ref).max() + np.abs(x * scale).max())    # (scale and offset are float32)
    with pytest.raises(ValueError):
        xvector.fold_batchnorm(mean, var[:-1])


@pytest.mark.parametrize("widths,n", [((64, 64, 64, 64, 100), 40), ((512, 512, 512, 512, 1500), 20)])
def test_float32_restatement_stays_within_1e_5_of_float64_on_the_gpu_cases(widths, n):
    """the CPU precondition of the GPU network tests, on their own inputs (tests/test_xvector_gpu.py builds the same case)"""
    from speech_signal_processing_amd import xvector
    net, feats, counts = network_case(widths, n)
    ref = XO.network(feats, counts, net.frame_layers, net.segment_layers, net.var_floor)
    f32 = XO.network(feats, counts, net.frame_layers, net.segment_layers, net.var_floor, dtype=np.float32)
    drift = np.abs(f32.astype(np.float64) - ref).max() / max(1.0, np.abs(ref).max())
    print("[measured] float32 drift at widths %s: %.3g" % (widths, drift))
    assert drift <= 1e-5
    assert isinstance(net, xvector.XVectorNet)


def network_case(widths, n):
    """the network cases of the GPU tests: the Snyder topology with Glorot kernels and scales in [0.5, 2], unit-variance inputs"""
    from speech_signal_processing_amd import xvector
    rng = np.random.RandomState(sum(widths))
    net = xvector.XVectorNet.snyder(39, rng, widths=widths, embed=64 if widths[0] < 512 else 512)
    counts = [40] * n if widths[0] < 512 else [40 + (i % 3) for i in range(n)]
    feats = rng.randn(sum(counts), 39).astype(np.float32)
    return net, feats, counts


def diar_net():
    """the network of the Extractor-in-Diarizer.run tests"""
    from speech_signal_processing_amd import xvector
    return xvector.XVectorNet.snyder(13, np.random.RandomState(12), widths=(32, 32, 32, 32, 48), embed=24)


@pytest.mark.parametrize("window", [None, 300])
def test_extractor_routes_give_the_same_labels_in_float64_with_a_margin(window):
    """the CPU precondition of the GPU test of xvector.Extractor inside Diarizer.run: restated in float64 on the host, the windowed route and
    the per-chunk route put the same windows together (the two voices), and a perturbation of 1e-3 of the unit-length embeddings — a
    thousand times the float32 network's error — changes no label.  With the sliding normalisation the two routes' embeddings differ
    by a third of their length (the mean is taken over the recording or over the chunk): only the labels can agree."""
    import diarize_oracle as DO
    out, counts = XO.extractor_routes(XO.diar_signals(), diar_net(), window)
    assert counts == [10, 9]
    (Ew, lw), (Ec, lc) = out["windows"], out["chunks"]
    assert np.array_equal(lw, lc) and lw.tolist() == [0] * 5 + [1] * 5 + [0] * 4 + [1] * 5
    diff = float(np.abs(Ew - Ec).max())
    print("[measured] window %s: largest difference between the routes' unit embeddings %.3g" % (window, diff))
    assert (diff == 0.0) if window is None else (diff > 0.05)
    rng = np.random.RandomState(0)
    for E, lab in (out["windows"], out["chunks"]):
        for _ in range(20):
            En = E + rng.randn(*E.shape) * 1e-3
            En /= np.linalg.norm(En, axis=1, keepdims=True)
            S = DO.pairwise(En.astype(np.float32), DO.offsets(counts)).astype(np.float32)
            assert np.array_equal(DO.ahc_batch(S, counts, "average", 0.0, n_speakers=[2, 2])["labels"], lab)


def _n_params(header, name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, "%s is not declared in include/ssp.h" % name
    return len(m.group(1).split(","))


def test_header_declarations_are_bound():
    from speech_signal_processing_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    for name, n_args in ENTRY_POINTS.items():
        assert _n_params(header, name) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "xvector.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "xvector.hip"))
    block = header[header.index("x-vector extractor forward"):]
    for word in ("EXTENSION", "UNPINNED", "tests/xvector_oracle.py", "SSP_ERR_UNSUPPORTED", "var_floor", "receptive field", "pool_win"):
        assert word in block, word
    assert "#define SSP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()      # (binds every symbol of SIGNATURES: AttributeError if one is not exported)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name
        assert lib.ssp_xvector_destroy(None) == _lib.SSP_OK
        assert lib.ssp_xvector_info(None, None, None, None) == _lib.SSP_ERR_INVALID


def test_python_surface_exists_and_fails_loudly_without_gpu():
    import torch
    from speech_signal_processing_amd import _lib, api, xvector
    for name in ("XVectorForward", "tdnn_forward", "stats_pool"):
        assert hasattr(api, name), name
    for name in ("XVectorNet", "fold_batchnorm", "Extractor"):
        assert hasattr(xvector, name), name
    rng = np.random.RandomState(0)
    net = xvector.XVectorNet.snyder(13, rng, widths=(16, 16, 16, 16, 24), embed=8)
    assert net.receptive_field == 15 and net.pooled_width == 48 and net.embed_width == 8 and net.d_in == 13
    for name in ("embed", "predict", "save", "load", "snyder"):
        assert callable(getattr(net, name)), name
    ex = xvector.Extractor(net, 16000, norm="sliding")
    assert callable(ex) and callable(ex.embed_windows)
    # windows in samples -> frames of the recording (25 ms / 10 ms at 16 kHz: win_len 400, hop 160)
    tab = ex.frame_windows([np.array([[0, 24000], [12000, 36000]]), np.array([[160, 400]])])
    assert tab.tolist() == [[0, 0, 148], [0, 75, 223], [1, 1, 1]]
    with pytest.raises(ValueError):
        xvector.Extractor(net, 16000, norm="cmvn")
    with pytest.raises(ValueError):
        xvector.Extractor(net, 8000, tables=ex.tables)
    with pytest.raises(ValueError):
        xvector.XVectorNet([{"W": np.zeros((4, 13), np.float32)}])
    with pytest.raises(ValueError):
        xvector.XVectorNet([{"W": np.zeros((4, 3, 13), np.float32)}], [{"W": np.zeros((4, 9), np.float32)}])
    with pytest.raises(ValueError):
        xvector.XVectorNet([{"W": np.zeros((4, 3, 13), np.float32), "stride": 2}])
    if torch.cuda.is_available():
        return
    with pytest.raises((_lib.SspError, RuntimeError, ImportError)):   # (the library's context: nothing computes on the CPU)
        net.embed(np.zeros((40, 13), np.float32), [40])
    with pytest.raises((_lib.SspError, RuntimeError, ImportError)):
        ex([np.zeros(16000, np.float32)])


def test_save_load_round_trip(tmp_path):
    from speech_signal_processing_amd import xvector
    rng = np.random.RandomState(1)
    net = xvector.XVectorNet.snyder(13, rng, widths=(16, 16, 16, 16, 24), embed=8, var_floor=1e-6)
    net.frame_layers[1]["scale"] = None
    path = str(tmp_path / "net.npz")
    net.save(path)
    back = xvector.XVectorNet.load(path)
    assert back.var_floor == net.var_floor and back.receptive_field == 15 and back.embed_width == 8
    for a, b in zip(net.frame_layers + net.segment_layers, back.frame_layers + back.segment_layers):
        assert set(a) == set(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert b[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
    with np.load(path, allow_pickle=False) as z:    # weights and settings only
        assert all(z[k].dtype.kind in "fi" for k in z.files)


def test_product_never_imports_the_test_oracle():
    pkg = os.path.join(ROOT, "speech_signal_processing_amd")
    for name in ("xvector.py", "api.py", "diarize.py"):
        assert not re.search(r"^\s*(import|from)\s+\S*xvector_oracle", open(os.path.join(pkg, name)).read(), flags=re.M), name
