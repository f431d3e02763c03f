"""The three device-pointer entry points of the score-normalisation block on arrays that are NOT 16-byte aligned, in the pattern of
tests/test_gpu_alignment.py (whose guarded views, bit-equality rule and guard checks these cases use): ssp_topn_stats, ssp_snorm_apply and
ssp_det_counts with every device input and output at 4- and 12-byte offsets, bit-equal to the aligned call, guards untouched, and for one
skew per case also checked against the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snorm_oracle as SN            # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)

pytestmark = pytest.mark.gpu
env = GA.env

TOPN_SKEWS = [{"scores": 4}, {"scores": 12}, {"scores": 4, "mean": 4, "std": 12, "kth": 4}, {"scores": 8, "mean": 12, "std": 4, "kth": 12}]
# rows of 260 bytes in registers; rows of 16388 bytes read again per pass; columns at a stride of 280 bytes
TOPN_CASES = [(5, 65, 7, 1), (5, 4097, 300, 1), (200, 70, 40, 0)]


@pytest.mark.parametrize("skews", TOPN_SKEWS, ids=GA.ids(TOPN_SKEWS))
@pytest.mark.parametrize("case", TOPN_CASES, ids=lambda c: "%dx%d-top%d-axis%d" % c)
def test_topn_stats_scores_and_outputs_skewed(env, case, skews):
    _, api, _lib, ctx = env
    rows, cols, n, axis = case
    X = SN.topn_case(rows, cols) if axis == 1 else np.ascontiguousarray(SN.topn_case(cols, rows).T)
    lines = rows if axis == 1 else cols
    names = ("mean", "std", "kth")

    def run(sk):
        a = GA.Arrays(sk)
        x = a.inp("scores", X)
        if a.skewed_outputs(names) or not sk:
            outs = [a.out(k, (lines,)) for k in names]
            _lib.check(ctx._lib.ssp_topn_stats(ctx._h, GA.p(x), rows, cols, cols, axis, n, *[GA.p(o) for o in outs], GA.DEVICE, None))
            return a.finish()
        for k in names:
            a.skew(k)
        r = api.topn_stats(ctx, x, n, axis=axis)
        return a.finish({k: r[k] for k in names})
    what = "topn %s %s" % (case, skews)
    got = GA.run_case(("topn", case), run, skews, what)
    if skews == {"scores": 4}:
        want = SN.topn_stats(X, n, axis=axis)
        bound = SN.stat_bound(X if axis == 1 else X.T)
        assert np.array_equal(got["kth"], want["kth"]), what
        assert (np.abs(got["mean"] - want["mean"]) <= bound).all() and (np.abs(got["std"] - want["std"]) <= bound).all(), what


APPLY_SKEWS = [{"scores": 4}, {"scores": 12, "rm": 4, "rs": 12, "cm": 4, "cs": 12}, {"out": 4, "argmax": 12, "max": 4},
               {"scores": 8, "out": 12, "argmax": 4, "max": 12, "cm": 8}]


@pytest.mark.parametrize("skews", APPLY_SKEWS, ids=GA.ids(APPLY_SKEWS))
@pytest.mark.parametrize("shape", [(5, 33), (300, 70)], ids=lambda s: "%dx%d" % s)
def test_snorm_apply_every_array_skewed(env, shape, skews):
    _, api, _lib, ctx = env
    N, S = shape
    g = SN.apply_case(N, S)

    def run(sk):
        a = GA.Arrays(sk)
        x = a.inp("scores", g["x"])
        st = [a.inp(k, g[k]) for k in ("rm", "rs", "cm", "cs")]
        out, am, mx = a.out("out", (N, S)), a.out("argmax", (N,), "int32"), a.out("max", (N,))
        _lib.check(ctx._lib.ssp_snorm_apply(ctx._h, GA.p(x), N, S, S, *[GA.p(s) for s in st], 1e-6, GA.p(out), S, GA.p(am), GA.p(mx),
                                            GA.DEVICE, None))
        return a.finish()
    what = "apply %s %s" % (shape, skews)
    got = GA.run_case(("apply", shape), run, skews, what)
    if skews == {"scores": 4}:
        want = SN.apply_f32(g["x"], g["rm"], g["rs"], g["cm"], g["cs"], 1e-6)
        wam, wmx = SN.decide(want)
        assert np.array_equal(got["out"], want) and np.array_equal(got["argmax"], wam) and np.array_equal(got["max"], wmx), what


DET_SKEWS = [{"scores": 4}, {"scores": 12, "target": 4}, {"scores": 8, "target": 12}]


@pytest.mark.parametrize("skews", DET_SKEWS, ids=GA.ids(DET_SKEWS))
@pytest.mark.parametrize("shape", [(300, 70, 1024), (5, 33, 4096)], ids=lambda s: "N%d-S%d-M%d" % s)
def test_det_counts_scores_and_targets_skewed(env, shape, skews):
    """ssp_det_counts on skewed device scores and targets; its outputs are host arrays"""
    _, api, _, ctx = env
    x, tgt, th = SN.det_case(*shape)
    names = ("tar_hist", "non_hist", "nan_count", "range")

    def run(sk):
        a = GA.Arrays(sk)
        r = api.det_counts(ctx, a.inp("scores", x), a.inp("target", tgt, "int32"), th)
        return a.finish({k: r[k] for k in names})
    got = GA.run_case(("det", shape), run, skews, "det %s %s" % (shape, skews))
    if skews == {"scores": 4}:
        want = SN.det_counts(x, tgt, th)
        assert all(np.array_equal(got[k], want[k]) for k in names)
