"""The two device-pointer entry points of the full-covariance GMM feature on arrays that are NOT 16-byte aligned, in the pattern of
tests/test_gmm_map_alignment_gpu.py (tests/test_gpu_alignment.py holds the guarded views, the bit-equality rule and the guard checks):
api.gmm_full_em_stats with the features, and api.GmmFullScorer.score / ssp_gmm_full_score with the features and every device output, at
4- and 12-byte skews, D = 39 and D = 40 (rows of 160 bytes: the base alone decides whether a row is 16-byte aligned) — bit-equal to the
aligned call, guards untouched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_full_cases as FC          # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)

pytestmark = pytest.mark.gpu
env = GA.env

LENS = [1, 70, 300]
SCORE_SKEWS = [{"feats": 4}, {"feats": 12}, {"feats": 4, "loglik": 4, "scores": 12, "argmax": 4}, {"loglik": 12, "scores": 4, "argmax": 12}]


@pytest.mark.parametrize("skews", SCORE_SKEWS, ids=GA.ids(SCORE_SKEWS))
@pytest.mark.parametrize("loglik", [True, False])
@pytest.mark.parametrize("D", [39, 40])
def test_full_score_features_and_outputs_skewed(env, D, loglik, skews):
    """3 models with a UBM, K = 5, utterances of 1 / 70 / 300 frames, with and without loglik_out"""
    _, api, _lib, ctx = env

    def make():
        c = FC.scorer_case(3, True, K=5, D=D, lens=LENS)
        return dict(c=c, sc=api.GmmFullScorer(ctx, c["w"], c["mus"], c["Us"], has_ubm=True), seg=api.Segments.from_lengths(ctx, LENS))
    g = GA.cached(("full", D), make)
    c, sc, seg = g["c"], g["sc"], g["seg"]
    skews = {k: v for k, v in skews.items() if loglik or k != "loglik"}
    F, U, M = seg.total, seg.n, sc.n_models
    names = ("loglik", "scores", "argmax") if loglik else ("scores", "argmax")

    def run(sk):
        a = GA.Arrays(sk)
        x = a.inp("feats", c["X"])
        if a.skewed_outputs(names) or not sk:
            ll = a.out("loglik", (M, F)) if loglik else None
            s_, am = a.out("scores", (U, M)), a.out("argmax", (U,), "int32")
            _lib.check(ctx._lib.ssp_gmm_full_score(sc._h, GA.p(x), seg._h, GA.p(ll), GA.p(s_), GA.p(am), GA.DEVICE, None))
            return a.finish()
        for n in names:
            a.skew(n)
        r = sc.score(x, seg, loglik=loglik)
        return a.finish({n: r[n] for n in names})
    what = "full score D %d loglik %d %s" % (D, loglik, skews)
    got = GA.run_case(("full", D, loglik), run, skews, what)
    assert all(np.isfinite(v).all() for v in got.values()), what
    if skews.get("feats") == 4 and loglik:
        FC.compare_loglik(got["loglik"], c["ref_ll"], c["emu_ll"], what)
        assert np.array_equal(got["argmax"], (c["ref_sc"][:, 1:] - c["ref_sc"][:, :1]).argmax(axis=1)), what


@pytest.mark.parametrize("skew", (4, 12))
@pytest.mark.parametrize("D", [39, 40])
def test_full_em_stats_device_frames_skewed(env, D, skew):
    """ssp_gmm_full_em_stats on a skewed device X (K = 5, 257 frames, a shift); its outputs are host arrays"""
    _, api, _, ctx = env
    c = FC.em_case(5, D, 257, 30.0)

    def run(sk):
        a = GA.Arrays(sk)
        st = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], a.inp("X", c["X"]), shift=c["shift"])
        return a.finish({"nk": st["nk"], "sx": st["sx"], "sxx": st["sxx"], "ll": np.array([st["loglik_sum"]])})
    got = GA.run_case(("full em", D), run, {"X": skew}, "full em stats D %d X skewed %d" % (D, skew))
    if skew == 4:
        import torch
        num_cu = torch.cuda.get_device_properties(0).multi_processor_count
        FC.compare(dict(nk=got["nk"], sx=got["sx"], sxx=got["sxx"], loglik_sum=got["ll"][0]), c["ev"], FC.acc_frames(257, 5, num_cu),
                   "full em stats D %d" % D)
