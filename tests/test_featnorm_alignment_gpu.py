"""The two device-pointer entry points of the sliding-normalisation block on arrays that are NOT 16-byte aligned, in the pattern of
tests/test_snorm_alignment_gpu.py (tests/test_gpu_alignment.py's guarded views, bit-equality rule and guard checks): ssp_featnorm_sliding
and ssp_select_frames with every device input and output 4 bytes past a 16-byte line (the mask 1 byte), bit-equal to the aligned call,
guards untouched, and for one skew per case also checked against the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featnorm_oracle as FO         # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)

pytestmark = pytest.mark.gpu
env = GA.env

LENS = [300, 0, 41, 513]
SLIDING_SKEWS = [{"feats": 4}, {"out": 4}, {"feats": 4, "out": 4}, {"feats": 12, "out": 8}]


def feats_case(D, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((sum(LENS), D)) * 1.5 + 0.5).astype(np.float32)
    x[7, 0] = np.nan
    return x


@pytest.mark.parametrize("skews", SLIDING_SKEWS, ids=GA.ids(SLIDING_SKEWS))
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("D", [13, 39])
def test_featnorm_sliding_input_and_output_skewed(env, D, mode, skews):
    _, api, _lib, ctx = env
    x = feats_case(D, 50 + D)
    seg = GA.cached(("featnorm seg",), lambda: api.Segments.from_lengths(ctx, LENS))

    def run(sk):
        a = GA.Arrays(sk)
        f = a.inp("feats", x)
        out = a.out("out", x.shape)
        _lib.check(ctx._lib.ssp_featnorm_sliding(ctx._h, GA.p(f), seg._h, D, 300, mode, GA.p(out), GA.DEVICE, None))
        return a.finish()
    what = "featnorm sliding d%d mode %d %s" % (D, mode, skews)
    got = GA.run_case(("featnorm sliding", D, mode), run, skews, what)
    if skews == {"feats": 4}:
        want, band = FO.sliding_batch(x, seg.offsets, 300, mode)
        FO.check(got["out"], want, band, what)


SELECT_SKEWS = [{"feats": 4, "mask": 1}, {"out": 4}, {"feats": 4, "mask": 1, "out": 4}, {"feats": 8, "mask": 3, "out": 12}]


@pytest.mark.parametrize("skews", SELECT_SKEWS, ids=GA.ids(SELECT_SKEWS))
@pytest.mark.parametrize("D", [13, 39])
def test_select_frames_every_array_skewed(env, D, skews):
    """the rows behind the kept ones keep the 0xA5 bytes the guarded view starts with; the counts are a host array"""
    _, api, _lib, ctx = env
    x = feats_case(D, 60 + D)
    mask = (np.random.default_rng(61).random(x.shape[0]) < 0.55).astype(np.uint8)
    seg = GA.cached(("featnorm seg",), lambda: api.Segments.from_lengths(ctx, LENS))

    def run(sk):
        a = GA.Arrays(sk)
        f = a.inp("feats", x)
        m = a.inp("mask", mask, "uint8")
        out = a.out("out", x.shape)
        cnt = np.zeros(len(LENS), dtype=np.int64)
        _lib.check(ctx._lib.ssp_select_frames(ctx._h, GA.p(f), seg._h, D, GA.p(m), GA.p(out), cnt.ctypes.data_as(C.POINTER(C.c_int64)),
                                              GA.DEVICE, None))
        return a.finish({"counts": cnt})
    what = "select frames d%d %s" % (D, skews)
    got = GA.run_case(("featnorm select", D), run, skews, what)
    if skews == SELECT_SKEWS[0]:
        kept, counts = FO.select(x, seg.offsets, mask)
        bits = got["out"].view(np.uint32)
        assert np.array_equal(got["counts"], counts), what
        assert np.array_equal(bits[:kept.shape[0]], kept) and (bits[kept.shape[0]:] == 0xA5A5A5A5).all(), what
