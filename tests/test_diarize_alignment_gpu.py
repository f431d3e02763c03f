"""The two device-pointer entry points of the diarization block on arrays that are NOT 16-byte aligned, in the pattern of
tests/test_snorm_alignment_gpu.py (tests/test_gpu_alignment.py holds the guarded views, the bit-equality rule and the guard checks):
ssp_pairwise_scores and ssp_ahc_cluster with X, the scores and every output at 4-, 8- and 12-byte offsets, bit-equal to the aligned call,
guards untouched, and for one skew per case also checked against the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diarize_oracle as DO          # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)

pytestmark = pytest.mark.gpu
env = GA.env

COUNTS = (33, 1, 65, DO.N_LDS + 1)
PAIR_SKEWS = [{"X": 4}, {"X": 12}, {"out": 4}, {"X": 8, "out": 12}]


def _seg(api, ctx):
    return GA.cached("diar-seg", lambda: api.Segments.from_lengths(ctx, COUNTS))


def _X(q):
    def make():
        rng = np.random.RandomState(77 + q)
        X = rng.randn(sum(COUNTS), q).astype(np.float32)
        return X / np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
    return GA.cached(("diar-X", q), make)


@pytest.mark.parametrize("skews", PAIR_SKEWS, ids=GA.ids(PAIR_SKEWS))
@pytest.mark.parametrize("q", [7, 130])
def test_pairwise_scores_input_and_output_skewed(env, q, skews):
    _, api, _lib, ctx = env
    X, seg = _X(q), _seg(api, ctx)
    total = int(DO.sq_offsets(COUNTS)[-1])

    def run(sk):
        a = GA.Arrays(sk)
        x, out = a.inp("X", X), a.out("out", (total,))
        _lib.check(ctx._lib.ssp_pairwise_scores(ctx._h, GA.p(x), seg._h, q, None, None, 0.0, GA.p(out), GA.DEVICE, None))
        return a.finish()
    what = "pairwise q=%d %s" % (q, skews)
    got = GA.run_case(("diar-pair", q), run, skews, what)
    if skews == {"X": 4}:
        ref = DO.pairwise(X, DO.offsets(COUNTS))
        for G, R in zip(DO.blocks(got["out"], COUNTS), DO.blocks(ref, COUNTS)):
            assert np.abs(G - R).max() <= DO.parity_bound(R) and np.array_equal(G, G.T), what


AHC_SKEWS = [{"scores": 4}, {"scores": 12}, {"labels": 4, "n_clusters": 12, "merge_pair": 4, "merge_score": 12},
             {"scores": 8, "labels": 12, "n_clusters": 4, "merge_pair": 12, "merge_score": 8}]


@pytest.mark.parametrize("skews", AHC_SKEWS, ids=GA.ids(AHC_SKEWS))
@pytest.mark.parametrize("linkage", [0, 1])
def test_ahc_cluster_every_array_skewed(env, linkage, skews):
    _, api, _lib, ctx = env
    seg = _seg(api, ctx)
    S = GA.cached("diar-S", lambda: DO.pairwise(np.concatenate([DO.cluster_case(n, 4, 32, 0.5, 100 + n)[0] for n in COUNTS]),
                                                  DO.offsets(COUNTS)).astype(np.float32))
    total = sum(COUNTS)

    def run(sk):
        a = GA.Arrays(sk)
        s = a.inp("scores", S)
        lab, cnt = a.out("labels", (total,), "int32"), a.out("n_clusters", (len(COUNTS),), "int32")
        mp, ms = a.out("merge_pair", (total, 2), "int32"), a.out("merge_score", (total,))
        _lib.check(ctx._lib.ssp_ahc_cluster(ctx._h, GA.p(s), seg._h, linkage, 0.5, 1, None, GA.p(lab), GA.p(cnt), GA.p(mp), GA.p(ms),
                                            GA.DEVICE, None))
        return a.finish()
    what = "ahc linkage=%d %s" % (linkage, skews)
    got = GA.run_case(("diar-ahc", linkage), run, skews, what)
    if skews == {"scores": 4}:
        want = DO.ahc_batch(S, COUNTS, DO.LINKAGES[linkage], 0.5)
        assert all(np.array_equal(got[k], want[k], equal_nan=(k == "merge_score")) for k in want), what
