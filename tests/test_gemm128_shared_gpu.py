"""dense_kernel (csrc/dense.hip) and tdnn_kernel (csrc/xvector.hip) are one GEMM block (csrc/gemm128.hpp) behind two operand walks: a frame
layer of ONE tap, dilation 1, without scale and offset is a dense layer, and ssp_tdnn_forward must then return the bits of
ssp_dense_forward through the tiled kernel — one k-ordered chain of 32-column slabs per output in both.

Shapes (d_in -> units, N), the smallest at which the slab walk can go wrong: 257 -> 130, N = 129 (nine slabs, an odd count, units off
the multiple of 4, a second workgroup of one row); 321 -> 257, N = 300 (eleven slabs, three unit blocks); and with SSP_DENSE_NO_REG
(read per call: d_in <= 256 goes to dense_kernel too) 33 -> 5, N = 1 (two slabs, every look-ahead load out of range) and 64 -> 128,
N = 128 (one full tile exactly).  Bias and ReLU on and off.  One sample carries a NaN, one a -inf: the comparison is of bit patterns, NaN
payloads included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ((257, 130, 129, False), (321, 257, 300, False), (33, 5, 1, True), (64, 128, 128, True))


@pytest.fixture(scope="module")
def api():
    from speech_signal_processing_amd import api
    return api


def _inputs(d_in, units, n):
    rng = np.random.default_rng(1000 * d_in + units)
    X = rng.standard_normal((n, d_in)).astype(np.float32)
    W = (rng.standard_normal((units, d_in)) / np.sqrt(d_in)).astype(np.float32)
    b = rng.standard_normal(units).astype(np.float32)
    X[n // 2, d_in - 1] = np.float32("nan")
    X[n - 1, 0] = -np.float32("inf")
    return X, W, b


@pytest.mark.parametrize("d_in,units,n,no_reg", SHAPES, ids=lambda v: str(v))
def test_one_tap_frame_layer_is_the_dense_layer(api, monkeypatch, d_in, units, n, no_reg):
    ctx = api.default_context()
    X, W, b = _inputs(d_in, units, n)
    if no_reg:
        monkeypatch.setenv("SSP_DENSE_NO_REG", "1")
    else:
        monkeypatch.delenv("SSP_DENSE_NO_REG", raising=False)
    for bias in (None, b):
        for relu in (False, True):
            dense = api.dense_forward(ctx, X, W, bias, relu=relu)
            tdnn, lens = api.tdnn_forward(ctx, X, [n], W.reshape(units, 1, d_in), bias, dilation=1, relu=relu)
            what = (d_in, units, n, "bias" if bias is not None else "no bias", "relu" if relu else "linear")
            assert list(lens) == [n], what
            assert dense.shape == tdnn.shape == (n, units) and dense.dtype == tdnn.dtype == np.float32, what
            assert np.isnan(dense[n // 2]).all() and not np.isnan(dense[:n // 2]).any(), what  # (the NaN sample, and only it and the -inf one)
            differ = np.argwhere(dense.view(np.uint32) != tdnn.view(np.uint32))
            assert differ.size == 0, (what, "%d elements differ, the first at (sample, unit)" % len(differ), differ[:4].tolist())
