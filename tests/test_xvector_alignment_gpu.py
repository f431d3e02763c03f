"""The three device-pointer entry points of the x-vector block on arrays that are NOT 16-byte aligned, in the pattern of
tests/test_diarize_alignment_gpu.py (tests/test_gpu_alignment.py holds the guarded views, the bit-equality rule and the guard checks):
ssp_tdnn_forward, ssp_stats_pool and ssp_xvector_forward with every array at 4-, 8- and 12-byte offsets, bit-equal to the aligned call,
guards untouched, and for one skew per case also checked against the restatement.  The frame-layer kernel picks 16-byte or scalar
stores from Y's address and reads its operands through buffer loads of 16 bytes at 4-byte aligned addresses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xvector_oracle as XO          # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)

pytestmark = pytest.mark.gpu
env = GA.env

COUNTS = (131, 0, 9, 140)
TDNN_SKEWS = [{"X": 4}, {"X": 12, "W": 4}, {"Y": 4}, {"Y": 8, "bias": 4, "scale": 8, "offset": 12}, {"X": 8, "W": 12, "Y": 12}]


def _seg(api, ctx):
    return GA.cached("xv-seg", lambda: api.Segments.from_lengths(ctx, COUNTS))


def _layer(d_in, units):
    def make():
        rng = np.random.RandomState(d_in + units)
        fl, _ = XO.random_layers(rng, d_in, [(units, 3, 2, True)])
        return fl[0], rng.randn(sum(COUNTS), d_in).astype(np.float32)
    return GA.cached(("xv-layer", d_in, units), make)


@pytest.mark.parametrize("skews", TDNN_SKEWS, ids=GA.ids(TDNN_SKEWS))
@pytest.mark.parametrize("d_in,units", [(13, 100), (40, 130)])
def test_tdnn_forward_every_array_skewed(env, d_in, units, skews):
    _, api, _lib, ctx = env
    seg = _seg(api, ctx)
    L, X = _layer(d_in, units)

    def run(sk):
        a = GA.Arrays(sk)
        x, w = a.inp("X", X), a.inp("W", L["W"])
        b, s, o = a.inp("bias", L["b"]), a.inp("scale", L["scale"]), a.inp("offset", L["offset"])
        y = a.out("Y", (sum(COUNTS), units))
        _lib.check(ctx._lib.ssp_tdnn_forward(ctx._h, GA.p(x), seg._h, d_in, GA.p(w), GA.p(b), 3, 2, units, 1, GA.p(s), GA.p(o), GA.p(y), None,
                                             GA.DEVICE, None))
        return a.finish()
    what = "tdnn d_in=%d units=%d %s" % (d_in, units, skews)
    got = GA.run_case(("xv-tdnn", d_in, units), run, skews, what)
    if skews == {"X": 4}:
        off = np.concatenate([[0], np.cumsum(COUNTS)])
        for i in range(len(COUNTS)):
            x = X[off[i]:off[i + 1]]
            ref = XO.layer(x, L)
            assert (np.abs(got["Y"][off[i]:off[i] + ref.shape[0]] - ref) <= XO.layer_bound(x, L)).all(), what


POOL_SKEWS = [{"X": 4}, {"X": 12}, {"out": 4}, {"X": 8, "out": 12}]
POOL_WINS = np.array([[0, 0, 131], [0, 5, 6], [2, 0, 9], [2, 9, 9], [3, 63, 140]], dtype=np.int64)


@pytest.mark.parametrize("skews", POOL_SKEWS, ids=GA.ids(POOL_SKEWS))
@pytest.mark.parametrize("dim", [7, 300])
def test_stats_pool_input_and_output_skewed(env, dim, skews):
    _, api, _lib, ctx = env
    seg = _seg(api, ctx)
    X = GA.cached(("xv-poolX", dim), lambda: np.random.RandomState(dim).randn(sum(COUNTS), dim).astype(np.float32))

    def run(sk):
        a = GA.Arrays(sk)
        x, out = a.inp("X", X), a.out("out", (len(POOL_WINS), 2 * dim))
        _lib.check(ctx._lib.ssp_stats_pool(ctx._h, GA.p(x), seg._h, dim, POOL_WINS.ctypes.data_as(C.POINTER(C.c_int64)), len(POOL_WINS), 1e-10,
                                           GA.p(out), GA.DEVICE, None))
        return a.finish()
    what = "stats pool dim=%d %s" % (dim, skews)
    got = GA.run_case(("xv-pool", dim), run, skews, what)
    if skews == {"X": 4}:
        off = np.concatenate([[0], np.cumsum(COUNTS)])
        ref = np.stack([XO.pool(X[off[q] + a:off[q] + b]) for q, a, b in POOL_WINS])
        GA.assert_feat_close(got["out"], ref, what)


NET_SKEWS = [{"feats": 4}, {"feats": 12}, {"emb": 4}, {"feats": 8, "emb": 12}]
NET_WINS = np.array([[0, 0, 131], [0, 30, 90], [2, 0, 9], [3, 0, 140], [3, 70, 140]], dtype=np.int64)


def _net(api, ctx):
    def make():
        rng = np.random.RandomState(21)
        spec = [(u, t, d, True) for u, (t, d) in zip((40, 40, 40, 40, 52), XO.SNYDER)]
        fl, sl = XO.random_layers(rng, 13, spec, segment=[(300, True), (30, False)])      # (a segment layer of d_in > 256 and one below)
        return fl, sl, api.XVectorForward(ctx, fl, sl), rng.randn(sum(COUNTS), 13).astype(np.float32)
    return GA.cached("xv-net", make)


@pytest.mark.parametrize("skews", NET_SKEWS, ids=GA.ids(NET_SKEWS))
@pytest.mark.parametrize("windows", [False, True])
def test_xvector_forward_input_and_output_skewed(env, windows, skews):
    _, api, _lib, ctx = env
    seg = _seg(api, ctx)
    fl, sl, fwd, feats = _net(api, ctx)
    n_out = len(NET_WINS) if windows else len(COUNTS)

    def run(sk):
        a = GA.Arrays(sk)
        x, out = a.inp("feats", feats), a.out("emb", (n_out, 30))
        _lib.check(ctx._lib.ssp_xvector_forward(fwd._h, GA.p(x), seg._h, NET_WINS.ctypes.data_as(C.POINTER(C.c_int64)) if windows else None,
                                                len(NET_WINS) if windows else 0, GA.p(out), GA.DEVICE, None))
        return a.finish()
    what = "xvector forward windows=%s %s" % (windows, skews)
    got = GA.run_case(("xv-fwd", windows), run, skews, what)
    if skews == {"feats": 4}:
        ref = XO.network(feats, COUNTS, fl, sl, windows=NET_WINS.tolist() if windows else None)
        GA.assert_feat_close(got["emb"], ref, what)
