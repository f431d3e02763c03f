"""Host checks of the sliding-normalisation block (no GPU): the float64 oracle against a frame-by-frame brute force, the warping table
of ssp_featnorm_table against scipy's ndtri, the host helper frames_in_segments, and the no-fall-back rule."""
import os
import re
import sys

import numpy as np
import pytest
from scipy.special import ndtri

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featnorm_oracle as FO   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_rule_holds_min_w_t_frames_and_contains_t():
    for T in range(1, 20):
        for W in range(1, 12):
            lo, hi = FO.window_bounds(T, W)
            t = np.arange(T)
            assert ((hi - lo) == min(W, T)).all(), (T, W)
            assert (lo >= 0).all() and (hi <= T).all() and (lo <= t).all() and (t < hi).all(), (T, W)
            if T >= W:   # away from the ends the window is centred
                mid = (t - W // 2 >= 0) & (t - W // 2 + W <= T)
                assert (lo[mid] == t[mid] - W // 2).all(), (T, W)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_equals_the_brute_force_loop(mode):
    rng = np.random.default_rng(7)
    for T, W in [(1, 1), (1, 5), (2, 3), (7, 3), (7, 4), (9, 9), (9, 11), (19, 6), (19, 7)]:
        x = rng.standard_normal((T, 3)).astype(np.float32)
        x[:, 1] = np.round(x[:, 1] * 2) / 2          # ties
        if T > 4:
            x[2, 0] = np.nan
            x[T - 1, 2] = np.nan
        want, band = FO.sliding(x, W, mode)
        brute = FO.sliding_brute(x, W, mode)
        assert (FO.kind(want) == FO.kind(brute)).all(), (T, W)
        fin = np.isfinite(brute)
        assert np.abs(want[fin] - brute[fin]).max(initial=0.0) <= 1e-12, (T, W)
        assert (band[fin] >= 0).all()


def test_oracle_keeps_an_infinity_inside_the_windows_that_hold_it():
    x = np.arange(40, dtype=np.float32).reshape(40, 1) % 7
    x[10, 0] = np.inf
    for mode in (0, 1, 2):
        want, _ = FO.sliding(x, 5, mode)
        lo, hi = FO.window_bounds(40, 5)
        holds = (lo <= 10) & (10 < hi)
        assert np.isfinite(want[~holds]).all(), mode
        if mode == 0:
            assert (want[holds & (np.arange(40) != 10), 0] == -np.inf).all() and np.isnan(want[10, 0])
        elif mode == 1:
            assert np.isnan(want[holds]).all()
        else:
            assert np.isfinite(want[holds]).all()   # an infinity ranks like any value


@pytest.fixture(scope="module")
def lib():
    from speech_signal_processing_amd import _lib
    return _lib


@pytest.mark.parametrize("W", [1, 2, 3, 300, 301, 1024])
def test_warping_table_against_ndtri(lib, W):
    from speech_signal_processing_amd import api
    tab = api.featnorm_table(W)
    assert tab.dtype == np.float32 and tab.shape == (W * W,)
    want = FO.table(W)
    err = np.abs(tab.astype(np.float64) - want)
    print("[measured] table %d: max err / |want| %.3e" % (W, float((err / np.maximum(np.abs(want), 1e-300))[want != 0].max(initial=0.0))))
    assert (err <= 2.0 ** -23 * np.abs(want)).all()
    for n in {n for n in (1, 2, 3, W // 2 + 1, W) if n <= W}:
        row = tab[(n - 1) ** 2: n * n]
        assert row.shape == (2 * n - 1,)
        assert row[n - 1] == 0.0 and not np.signbit(row[n - 1])
        assert np.array_equal(row, -row[::-1]), n          # antisymmetric, exactly
        assert (np.diff(row) > 0).all(), n


def test_warping_table_rejects_bad_windows(lib):
    from speech_signal_processing_amd import api
    buf = np.zeros(4, dtype=np.float32)
    for w in (0, -1, 1025):
        assert lib.load().ssp_featnorm_table(w, buf.ctypes.data) == lib.SSP_ERR_INVALID
        with pytest.raises(ValueError):
            api.featnorm_table(w)
    assert lib.load().ssp_featnorm_table(2, None) == lib.SSP_ERR_INVALID


def test_tile_constant_is_the_same_in_header_binding_and_kernel(lib):
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    src = open(os.path.join(ROOT, "speech_signal_processing_amd", "csrc", "featnorm.hip")).read()
    assert int(re.search(r"#define SSP_FEATNORM_TILE (\d+)", header).group(1)) == lib.FEATNORM_TILE
    assert re.search(r"constexpr int FN_TILE = SSP_FEATNORM_TILE;", src)
    assert lib.FEATNORM_MAX_WINDOW == int(re.search(r"constexpr int FN_MAX_WINDOW = (\d+);", src).group(1)) == 1024


def test_frames_in_segments_on_hand_made_ranges():
    from speech_signal_processing_amd import featnorm
    # centres of frames 0 .. 5 at win 400, hop 160: 200, 360, 520, 680, 840, 1000
    m = featnorm.frames_in_segments([(0, 361), (680, 840)], 6)
    assert m.dtype == np.uint8 and m.tolist() == [1, 1, 0, 1, 0, 0]
    assert featnorm.frames_in_segments([], 4).tolist() == [0, 0, 0, 0]
    assert featnorm.frames_in_segments([(0, 10 ** 9)], 3).tolist() == [1, 1, 1]
    assert featnorm.frames_in_segments([(5, 25)], 4, win=10, hop=10).tolist() == [1, 1, 0, 0]   # centres 5, 15, 25, 35; end exclusive
    assert featnorm.frames_in_segments([(0, 5)], 0).shape == (0,)
    for segs, n, win, hop in [([(100, 900), (1500, 1700)], 12, 400, 160), ([(0, 128), (256, 300)], 9, 256, 128)]:
        assert np.array_equal(featnorm.frames_in_segments(segs, n, win, hop), FO.frames_in_segments(segs, n, win, hop))


def test_sidekit_names_refuse_the_causal_window():
    from speech_signal_processing_amd import sidekit_features as SF
    with pytest.raises(NotImplementedError):
        SF.cep_sliding_norm(np.zeros((4, 2), dtype=np.float32), center=False)


def test_no_fall_back_without_a_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speech_signal_processing_amd import featnorm
    x = np.zeros((10, 3), dtype=np.float32)
    with pytest.raises(lib.SspError):
        featnorm.cmvn_sliding(x)
    with pytest.raises(lib.SspError):
        featnorm.feature_warp([x, x])
    with pytest.raises(lib.SspError):
        featnorm.select_frames(x, np.ones(10, dtype=np.uint8))
