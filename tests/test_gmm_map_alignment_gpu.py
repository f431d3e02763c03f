"""The two device-pointer entry points of the MAP / top-C feature on arrays that are NOT 16-byte aligned, in the pattern of
tests/test_gpu_alignment.py (whose guarded views, bit-equality rule and guard checks these cases use): api.gmm_em_stats_shared and
api.MapScorer.score / ssp_gmm_map_score with the features — and, through the C-ABI, every output — at a 4-byte offset, bit-equal to the
aligned call, guards untouched, and for the 4-byte feature skew also within the oracle's tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_oracle as MO              # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)
from test_gmm_map_gpu import ATOL, RTOL, make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
env = GA.env

LENS = [1, 70, 300]
MAP_SKEWS = [{"feats": 4}, {"feats": 12}, {"feats": 4, "diff": 4, "ubm": 8, "argmax": 12, "idx": 4}, {"diff": 12, "ubm": 4, "argmax": 4, "idx": 8}]


@pytest.mark.parametrize("skews", MAP_SKEWS, ids=GA.ids(MAP_SKEWS))
@pytest.mark.parametrize("D", [39, 40])
def test_map_score_features_and_outputs_skewed(env, D, skews):
    """K = 70 (two chunks), 5 speakers, C = 5, utterances of 1 / 70 / 300 frames; D = 40: rows of 160 bytes, where the base alone decides
    whether a row is 16-byte aligned"""
    _, api, _lib, ctx = env
    K, S, Ck = 70, 5, 5

    def make():
        g = make_inputs(K, D, S, 400 + D, lens=LENS)
        g["sc"] = api.MapScorer(ctx, g["w"], g["mu"], g["cv"], g["sm"])
        g["seg"] = api.Segments.from_lengths(ctx, LENS)
        return g
    g = GA.cached(("map", D), make)
    sc, seg = g["sc"], g["seg"]
    F, U = seg.total, seg.n
    names = ("diff", "ubm", "argmax", "idx")

    def run(sk):
        a = GA.Arrays(sk)
        x = a.inp("feats", g["X"])
        if a.skewed_outputs(names) or not sk:
            df, ub = a.out("diff", (U, S)), a.out("ubm", (U,))
            am, ix = a.out("argmax", (U,), "int32"), a.out("idx", (F, Ck), "int32")
            _lib.check(ctx._lib.ssp_gmm_map_score(sc._h, GA.p(x), seg._h, Ck, GA.p(df), GA.p(ub), GA.p(am), GA.p(ix), GA.DEVICE, None))
            return a.finish()
        for n in names:
            a.skew(n)
        r = sc.score(x, seg, top_c=Ck, ubm=True, idx=True)
        return a.finish({n: r[n] for n in names})
    what = "map score D %d %s" % (D, skews)
    got = GA.run_case(("map", D), run, skews, what)
    assert np.isfinite(got["diff"]).all() and np.isfinite(got["ubm"]).all() and (got["idx"] >= 0).all(), what
    if skews.get("feats") == 4:
        ref = MO.topc_scores(g["w"], g["mu"], g["cv"], g["sm"], g["X"], g["off"], Ck, idx=got["idx"])
        assert (np.abs(got["diff"] - ref["diff"]) <= ATOL + RTOL * np.abs(ref["diff"])).all(), what
        assert (np.abs(got["ubm"] - ref["ubm"]) <= ATOL + RTOL * np.abs(ref["ubm"])).all(), what


@pytest.mark.parametrize("skew", GA.F32)
def test_em_stats_shared_device_frames_skewed(env, skew):
    """ssp_gmm_em_stats_shared on a skewed device X (K = 16, D = 39, three overlapping ranges of 500 frames); its outputs are host arrays"""
    _, api, _, ctx = env
    g = GA.cached("map shared", lambda: make_inputs(16, 39, 1, 61, lens=[500]))
    off, cnt = np.array([0, 100, 37]), np.array([500, 400, 203])

    def run(sk):
        a = GA.Arrays(sk)
        st = api.gmm_em_stats_shared(ctx, g["w"], g["mu"], g["cv"], a.inp("X", g["X"]), off, cnt)
        return a.finish({"nk": st["nk"], "sx": st["sx"], "sxx": st["sxx"], "ll": st["loglik_sum"]})
    got = GA.run_case("map shared", run, {"X": skew}, "em stats shared X skewed %d" % skew)
    assert all(np.isfinite(v).all() for v in got.values())
    if skew == 4:
        for m in range(3):   # (tests/test_gpu_parity.py test_gmm_em_stats_shapes' rules)
            nk, sx, sxx = MO.stats(g["w"], g["mu"], g["cv"], g["X"][off[m]:off[m] + cnt[m]])
            assert np.allclose(got["nk"][m], nk, rtol=1e-4, atol=1e-4 * nk.max())
            assert np.allclose(got["sx"][m], sx, rtol=1e-4, atol=1e-4 * np.abs(sx).max())
            assert np.allclose(got["sxx"][m], sxx, rtol=1e-4, atol=1e-4 * np.abs(sxx).max())
