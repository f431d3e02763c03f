"""GPU tests of sliding-window normalisation, feature warping and frame selection (ssp_featnorm_sliding, ssp_select_frames; run with
-m gpu on an MI355X) against the float64 restatement and the bands of tests/featnorm_oracle.py.  Lengths sit around the kernel's tile
(L = _lib.FEATNORM_TILE) and around the window; every oracle result is computed once and shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featnorm_oracle as FO   # noqa: E402
from conftest import synth_audio  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


@pytest.fixture(scope="module")
def env():
    from speech_signal_processing_amd import api, _lib
    return api, _lib, api.default_context()


def lengths_for(W, L):
    """0 in the middle of the batch, 1, 2, the window's and the tile's neighbours, more than two and three tiles"""
    return [1, 2, W - 1, W, 0, W + 1, L - 1, L, L + 1, 2 * L + 1, 3 * L + 5]


def data(lens, D, seed):
    """columns with spreads 0.5 .. 2 around offsets of up to twice the spread"""
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    return (rng.standard_normal((n, D)) * rng.uniform(0.5, 2.0, D) + rng.uniform(-2.0, 2.0, D) * rng.uniform(0.5, 2.0, D)).astype(np.float32)


def offsets_of(lens, start=0):
    return np.concatenate([[start], start + np.cumsum(lens)]).astype(np.int64)


def want_for(key, x, off, W, mode):
    if key not in _WANT:
        _WANT[key] = FO.sliding_batch(x, off, W, mode)
    return _WANT[key]


def run_and_check(env, x, lens, W, mode, key, what):
    api, _, ctx = env
    seg = api.Segments.from_lengths(ctx, lens)
    got = api.featnorm_sliding(ctx, x, seg, window=W, mode=mode)
    want, band = want_for(key, x, seg.offsets, W, mode)
    FO.check(got, want, band, what)
    return got


# every window at dim 13; every dim at an even and an odd window.  13 and 39 are not whole numbers of the kernel's 8-column groups, 12 is 1.5
CASES = [(W, 13) for W in (3, 4, 300, 301)] + [(W, D) for W in (4, 301) for D in (1, 39, 12)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "w%d-d%d" % c)
def test_lengths_around_window_and_tile(env, case, mode):
    W, D = case
    lens = lengths_for(W, env[1].FEATNORM_TILE)
    run_and_check(env, data(lens, D, 100 + W), lens, W, mode, ("len", W, D, mode), "lengths w%d d%d mode %d" % (W, D, mode))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_window_larger_than_every_utterance(env, mode):
    """window 1000 over utterances of at most 3 L + 5 = 773 frames: every window is the whole utterance, every table row but the last"""
    L = env[1].FEATNORM_TILE
    lens = [1, 2, 0, L - 1, L, L + 1, 2 * L + 1, 3 * L + 5]
    assert max(lens) < 1000
    run_and_check(env, data(lens, 13, 5), lens, 1000, mode, ("large", mode), "window 1000 mode %d" % mode)


@pytest.mark.parametrize("mode", [1, 2])
def test_largest_window_inside_longer_utterances(env, mode):
    """window 1024 (the largest LDS image, the longest table row) inside utterances of 1024, 1025 and 1300 frames"""
    lens = [1024, 0, 1025, 1300]
    run_and_check(env, data(lens, 3, 6), lens, 1024, mode, ("w1024", mode), "window 1024 mode %d" % mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_offset_column(env, mode):
    """a column whose offset is 100 times its spread: a / s = 100, the edge of what the band covers"""
    lens = [700, 301]
    x = data(lens, 3, 8)
    rng = np.random.default_rng(9)
    x[:, 1] = (100.0 + rng.standard_normal(x.shape[0])).astype(np.float32)
    x[:, 2] = (-25.0 + 0.25 * rng.standard_normal(x.shape[0])).astype(np.float32)
    run_and_check(env, x, lens, 300, mode, ("offset", mode), "offset column mode %d" % mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_constant_column(env, mode):
    """deviation 0: the divisor is 1, the output 0 in modes 0 and 1 and phi^-1(n / 2n) = 0 in mode 2"""
    lens = [5, 300, 530]
    x = data(lens, 3, 10)
    x[:, 1] = np.float32(3.25)
    x[5:305, 2] = np.float32(-0.1)      # constant through one whole utterance only
    got = run_and_check(env, x, lens, 300, mode, ("const", mode), "constant column mode %d" % mode)
    assert (got[:, 1] == 0).all() and (got[5:305, 2] == 0).all()


@pytest.mark.parametrize("W", [4, 301])
def test_ties_get_the_mid_rank(env, W):
    lens = [2, 600, 257]
    x = data(lens, 4, 11)
    x[:, 0] = np.round(x[:, 0] * 2) / 2
    x[:, 3] = np.round(x[:, 3])
    x[10:40, 3] = -0.0                    # -0 ties with +0
    x[40:60, 3] = 0.0
    run_and_check(env, x, lens, W, 2, ("ties", W), "ties w%d" % W)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("W", [4, 300])
def test_nan_entries_are_left_out_and_stay_nan(env, W, mode):
    L = env[1].FEATNORM_TILE
    lens = [3, 2 * L + 40, L, 7]
    x = data(lens, 9, 12)
    rng = np.random.default_rng(13)
    x[rng.random(x.shape) < 0.05] = np.nan          # scattered entries
    x[3 + 100: 3 + 104] = np.nan                    # whole rows: with window 4 a window of nothing but NaN
    x[3 + 2 * L + 40 + 17] = np.nan
    x[-7:, 2] = np.nan                              # a column of one utterance with no entry at all
    got = run_and_check(env, x, lens, W, mode, ("nan", W, mode), "NaN entries w%d mode %d" % (W, mode))
    assert np.array_equal(np.isnan(got), np.isnan(x))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("W", [4, 300])
def test_infinities_stay_inside_the_windows_that_hold_them(env, W, mode):
    L = env[1].FEATNORM_TILE
    lens = [3 * L, 2 * L + 9]
    x = data(lens, 5, 14)
    x[L + 3, 1] = np.inf
    x[3 * L + L + 100, 1] = -np.inf
    x[200, 3] = np.inf                   # both kinds 40 frames apart in one column: windows with one, the other, or both
    x[240, 3] = -np.inf
    got = run_and_check(env, x, lens, W, mode, ("inf", W, mode), "infinities w%d mode %d" % (W, mode))
    off = offsets_of(lens)
    for u in range(2):
        T = lens[u]
        lo, hi = FO.window_bounds(T, W)
        for c in (1, 3):
            pos = np.flatnonzero(np.isinf(x[off[u]:off[u + 1], c]))
            reach = np.zeros(T, dtype=bool)
            for p in pos:
                reach |= (lo <= p) & (p < hi)
            assert np.isfinite(got[off[u]:off[u + 1], c][~reach]).all(), (u, c)
    assert np.isfinite(got[:, [0, 2, 4]]).all()


@pytest.mark.parametrize("mode", [1, 2])
def test_segment_table_that_starts_past_row_zero(env, mode):
    """rows in front of the table are neither read (they hold NaN) nor written (the output keeps its poison there)"""
    import torch
    api, _lib, ctx = env
    lens = [300, 0, 41]
    start = 37
    body = data(lens, 13, 15)
    x = np.concatenate([np.full((start, 13), np.nan, dtype=np.float32), body])
    seg = api.Segments(ctx, offsets_of(lens, start))
    want, band = want_for(("shift", mode), x, seg.offsets, 300, mode)
    dx = torch.from_numpy(x).cuda()
    out = torch.full_like(dx, -77.0)
    _lib.check(ctx._lib.ssp_featnorm_sliding(ctx._h, dx.data_ptr(), seg._h, 13, 300, mode, out.data_ptr(), _lib.DEVICE, None))
    ctx.sync()
    got = out.cpu().numpy()
    assert (got[:start] == -77.0).all()
    FO.check(got[start:], want, band, "shifted table mode %d" % mode)
    host = np.full_like(x, -77.0)
    _lib.check(ctx._lib.ssp_featnorm_sliding(ctx._h, x.ctypes.data, seg._h, 13, 300, mode, host.ctypes.data, _lib.HOST, None))
    assert np.array_equal(host.view(np.uint32), got.view(np.uint32))
    same = FO.sliding_batch(body, offsets_of(lens), 300, mode)[0]
    assert np.array_equal(np.isnan(same), np.isnan(want)) and np.array_equal(same[~np.isnan(same)], want[~np.isnan(want)])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_host_and_device_paths_agree_bit_for_bit(env, mode):
    import torch
    api, _, ctx = env
    lens = [513, 0, 77, 300]
    x = data(lens, 13, 16)
    x[5, 2] = np.nan
    seg = api.Segments.from_lengths(ctx, lens)
    host = api.featnorm_sliding(ctx, x, seg, window=300, mode=mode)
    dev = api.featnorm_sliding(ctx, torch.from_numpy(x).cuda(), seg, window=300, mode=mode)
    assert isinstance(host, np.ndarray) and dev.is_cuda
    assert np.array_equal(host.view(np.uint32), dev.cpu().numpy().view(np.uint32))
    again = api.featnorm_sliding(ctx, x, seg, window=300, mode=mode)
    assert np.array_equal(host.view(np.uint32), again.view(np.uint32))          # the same bits every call


# ------------------------------------------------------------------------------------------------------------------------ selection
def select_case(lens, D, seed, kind):
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    bits = rng.integers(0, 2 ** 32, size=(n, D), dtype=np.uint64).astype(np.uint32)     # every bit pattern: NaN payloads, infinities, denormals
    x = bits.view(np.float32)
    if kind == "none":
        mask = np.zeros(n, dtype=np.uint8)
    elif kind == "all":
        mask = np.full(n, 255, dtype=np.uint8)
    else:
        mask = (rng.random(n) < 0.6).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)   # any non-zero byte keeps
    return x, mask


@pytest.mark.parametrize("kind", ["mixed", "none", "all"])
@pytest.mark.parametrize("D", [1, 39])
def test_select_frames_equals_boolean_indexing(env, D, kind):
    """raw calls on poisoned outputs, host and device: the kept rows bit for bit, the counts, and the poison behind them"""
    import torch
    api, _lib, ctx = env
    lens = [5, 0, 255, 256, 257, 1, 64 * 256 + 3, 700]        # (the long one: every slice of the copy kernel walks more than one chunk)
    x, mask = select_case(lens, D, 20 + D, kind)
    seg = api.Segments.from_lengths(ctx, lens)
    kept, counts = FO.select(x, seg.offsets, mask)
    n = x.shape[0]
    poison = np.uint32(0xA5A5A5A5)
    for where in (_lib.DEVICE, _lib.HOST):
        cnt = np.full(len(lens), -7, dtype=np.int64)
        if where == _lib.DEVICE:
            dx, dm = torch.from_numpy(x.view(np.int32)).cuda(), torch.from_numpy(mask).cuda()
            out = torch.from_numpy(np.full((n, D), poison, dtype=np.uint32).view(np.int32)).cuda()
            ptrs = (dx.data_ptr(), dm.data_ptr(), out.data_ptr())
        else:
            out = np.full((n, D), poison, dtype=np.uint32)
            ptrs = (x.ctypes.data, mask.ctypes.data, out.ctypes.data)
        _lib.check(ctx._lib.ssp_select_frames(ctx._h, ptrs[0], seg._h, D, ptrs[1], ptrs[2], cnt.ctypes.data_as(C.POINTER(C.c_int64)), where, None))
        got = out.cpu().numpy().view(np.uint32) if where == _lib.DEVICE else out
        assert np.array_equal(cnt, counts), (where, cnt, counts)
        assert np.array_equal(got[:kept.shape[0]], kept), where
        assert (got[kept.shape[0]:] == poison).all(), where


def test_select_frames_api_and_shifted_table(env):
    import torch
    api, _, ctx = env
    lens = [300, 0, 41, 513]
    start = 11
    x, mask = select_case([start] + lens, 13, 31, "mixed")
    seg = api.Segments(ctx, offsets_of(lens, start))
    kept, counts = FO.select(x, seg.offsets, mask)
    for dev in (False, True):
        a, m = (torch.from_numpy(x.view(np.int32)).cuda().view(torch.float32), torch.from_numpy(mask).cuda()) if dev else (x, mask)
        rows, kseg, cnt = api.select_frames(ctx, a, seg, m)
        rows = rows.cpu().numpy() if dev else rows
        assert np.array_equal(rows.view(np.uint32), kept) and np.array_equal(cnt, counts)
        assert np.array_equal(kseg.offsets, np.concatenate([[0], np.cumsum(counts)]))


# ------------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(env):
    import torch
    api, _lib, ctx = env
    x = torch.zeros((10, 3), device="cuda")
    out = torch.zeros_like(x)
    seg = api.Segments.from_lengths(ctx, [10])
    cnt = np.zeros(1, dtype=np.int64)
    cp = cnt.ctypes.data_as(C.POINTER(C.c_int64))
    m = torch.ones(10, dtype=torch.uint8, device="cuda")

    def sliding(window=300, mode=1, dim=3, o=out):
        return ctx._lib.ssp_featnorm_sliding(ctx._h, x.data_ptr(), seg._h, dim, window, mode, o.data_ptr(), _lib.DEVICE, None)
    assert sliding() == _lib.SSP_OK
    for kw in ({"mode": 3}, {"mode": -1}, {"window": 0}, {"window": 1025}, {"dim": 0}, {"dim": 4097}, {"o": x}):
        assert sliding(**kw) == _lib.SSP_ERR_INVALID, kw
    assert ctx._lib.ssp_featnorm_sliding(ctx._h, x.data_ptr(), seg._h, 3, 300, 1, out.data_ptr(), 2, None) == _lib.SSP_ERR_INVALID
    assert ctx._lib.ssp_featnorm_sliding(ctx._h, x.data_ptr(), None, 3, 300, 1, out.data_ptr(), _lib.DEVICE, None) == _lib.SSP_ERR_INVALID
    assert ctx._lib.ssp_select_frames(ctx._h, x.data_ptr(), seg._h, 3, m.data_ptr(), out.data_ptr(), cp, _lib.DEVICE, None) == _lib.SSP_OK
    assert ctx._lib.ssp_select_frames(ctx._h, x.data_ptr(), seg._h, 3, m.data_ptr(), x.data_ptr(), cp, _lib.DEVICE, None) == _lib.SSP_ERR_INVALID
    assert ctx._lib.ssp_select_frames(ctx._h, x.data_ptr(), seg._h, 3, m.data_ptr(), out.data_ptr(), None, _lib.DEVICE, None) == _lib.SSP_ERR_INVALID
    assert ctx._lib.ssp_select_frames(ctx._h, x.data_ptr(), seg._h, 0, m.data_ptr(), out.data_ptr(), cp, _lib.DEVICE, None) == _lib.SSP_ERR_INVALID
    with pytest.raises(ValueError):
        api.featnorm_sliding(ctx, x, seg, window=1025)
    with pytest.raises(ValueError):
        api.select_frames(ctx, x, seg, np.ones(10, dtype=np.uint8))          # arrays of two kinds
    ctx.sync()


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_featnorm_module_on_single_arrays_and_lists(env):
    from speech_signal_processing_amd import featnorm, sidekit_features as SF
    lens = [310, 40, 0]
    x = data(lens, 13, 40)
    off = offsets_of(lens)
    parts = [x[off[i]:off[i + 1]] for i in range(3)]
    for fn, kw, mode in [(featnorm.cmvn_sliding, {}, 1), (featnorm.cmvn_sliding, {"norm_vars": False}, 0), (featnorm.feature_warp, {}, 2)]:
        got = fn(parts, window=300, **kw)
        assert isinstance(got, list) and [g.shape for g in got] == [p.shape for p in parts] and all(g.dtype == np.float32 for g in got)
        want, band = want_for(("module", mode), x, off, 300, mode)
        FO.check(np.concatenate(got), want, band, "featnorm module mode %d" % mode)
        one = fn(parts[0].astype(np.float64), window=300, **kw)
        assert one.dtype == np.float64 and np.array_equal(one, got[0].astype(np.float64))
    assert np.array_equal(SF.cep_sliding_norm(parts[0], win=301, reduce=True), featnorm.cmvn_sliding(parts[0], window=301))
    assert np.array_equal(SF.cep_sliding_norm(parts[0], win=301), featnorm.cmvn_sliding(parts[0], window=301, norm_vars=False))
    assert np.array_equal(SF.stg(parts[0], win=301), featnorm.feature_warp(parts[0], window=301))
    masks = [(np.arange(n) % 3 != 0).astype(np.uint8) for n in lens]
    sel = featnorm.select_frames(parts, masks)
    assert all(np.array_equal(s, p[m != 0]) for s, p, m in zip(sel, parts, masks))
    assert np.array_equal(featnorm.select_frames(parts[1], masks[1]), parts[1][masks[1] != 0])


@pytest.mark.parametrize("order", [1, 2])
def test_extract_feature_with_sliding_normalisation(env, order):
    """norm='sliding' | 'warp' equals the composed calls; norm='utterance' is the call without the keyword, bit for bit"""
    import torch
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import GMM_UBM as G
    api, _, _ = env
    sigs = [synth_audio(u, n, 16000) for u, n in enumerate([16000, 4000, 52000])]
    y = [0, 1, 0]
    base, _ = G.extract_feature(sigs, y, delta_order=order)
    named, _ = G.extract_feature(sigs, y, delta_order=order, norm='utterance', window=123)
    assert all(np.array_equal(a, b) for a, b in zip(base, named))
    ctx = api.default_context()
    plan = api.MfccPlan(ctx, pkg.preset_sidekit(fs=16000, delta_order=order, cmvn=0))
    flat, lens = api.flatten_signals(sigs)
    seg = api.Segments.from_lengths(ctx, lens)
    fseg = plan.frame_segments(seg)
    raw = plan.run(torch.from_numpy(np.ascontiguousarray(flat)).cuda(), seg, fseg)
    for norm, mode in (("sliding", 1), ("warp", 2)):
        got, yy = G.extract_feature(sigs, y, delta_order=order, norm=norm, window=200)
        want = api.featnorm_sliding(ctx, raw, fseg, window=200, mode=mode).cpu().numpy().astype(np.float64)
        assert yy is y and [g.shape for g in got] == [(int(fseg.offsets[i + 1] - fseg.offsets[i]), 13 * (order + 1)) for i in range(3)]
        assert all(g.dtype == np.float64 for g in got) and np.array_equal(np.concatenate(got), want)
        o64, b64 = FO.sliding_batch(raw.cpu().numpy(), fseg.offsets, 200, mode)
        FO.check(np.concatenate(got), o64, b64, "extract_feature %s order %d" % (norm, order))
    train, feats, _ = G.extract_feature(sigs, y, is_train=True, delta_order=order, norm='warp')
    assert sorted(train) == [0, 1] and train[0].shape[0] == feats[0].shape[0] + feats[2].shape[0]
    with pytest.raises(ValueError):
        G.extract_feature(sigs, y, norm='window')
