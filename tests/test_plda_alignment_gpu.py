"""The two device-pointer entry points of the PLDA back end on arrays that are NOT 16-byte aligned, in the pattern of
tests/test_gpu_alignment.py (whose guarded views, bit-equality rule and guard checks these cases use): api.plda_stats / ssp_plda_stats with
the rows and the labels, and api.PldaScorer.score / ssp_plda_score with the test vectors — and, through the C-ABI, every output — at 4-
and 12-byte offsets, bit-equal to the aligned call, guards untouched, and for one skew per case also within the oracle's tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_oracle as PO             # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)

pytestmark = pytest.mark.gpu
env = GA.env

SCORE_SKEWS = [{"T": 4}, {"T": 12}, {"T": 4, "llr": 4, "argmax": 12, "max": 4}, {"llr": 12, "argmax": 4, "max": 12}]
# q = 64: rows of 256 bytes, where the base alone decides whether a row is 16-byte aligned; q = 5: rows of 20 bytes; S = 33 / 70: llr rows
# of 132 / 280 bytes
SCORE_CASES = [(3, 0), (3, 1), (2, 0), (10, 0)]   # (index into PO.SCORER_CASES, flags)


@pytest.mark.parametrize("skews", SCORE_SKEWS, ids=GA.ids(SCORE_SKEWS))
@pytest.mark.parametrize("idx,flags", SCORE_CASES)
def test_score_test_vectors_and_outputs_skewed(env, idx, flags, skews):
    _, api, _lib, ctx = env
    case = PO.SCORER_CASES[idx]
    g = PO.scorer_case(case)
    sc = GA.cached(("plda", idx, flags), lambda: api.PldaScorer(ctx, g["psi"], g["enrol"], g["counts"], flags=flags))
    N, S = g["ref"].shape
    names = ("llr", "argmax", "max")

    def run(sk):
        a = GA.Arrays(sk)
        t = a.inp("T", g["T"])
        if a.skewed_outputs(names) or not sk:
            lr, am, mx = a.out("llr", (N, S)), a.out("argmax", (N,), "int32"), a.out("max", (N,))
            _lib.check(ctx._lib.ssp_plda_score(sc._h, GA.p(t), N, GA.p(lr), GA.p(am), GA.p(mx), GA.DEVICE, None))
            return a.finish()
        for n in names:
            a.skew(n)
        r = sc.score(t, llr=True)
        return a.finish({n: r[n] for n in names})
    what = "plda score %s flags %d %s" % (case, flags, skews)
    got = GA.run_case(("plda", idx, flags), run, skews, what)
    assert np.isfinite(got["llr"]).all() and (got["argmax"] >= 0).all(), what
    if skews == {"T": 4}:
        assert (np.abs(got["llr"] - g["ref"]).max(axis=1) <= PO.llr_bound(g["ref"])).all(), what
        assert np.array_equal(got["argmax"][g["keep"]], g["ref"].argmax(axis=1)[g["keep"]]), what


STATS_SKEWS = [{"X": 4}, {"X": 12}, {"X": 8, "labels": 4}, {"labels": 12}]


@pytest.mark.parametrize("skews", STATS_SKEWS, ids=GA.ids(STATS_SKEWS))
@pytest.mark.parametrize("q,N,S", [(5, 1025, 7), (64, 2500, 40)])
def test_stats_rows_and_labels_skewed(env, q, N, S, skews):
    """ssp_plda_stats on skewed device rows and labels; its outputs are host arrays"""
    _, api, _, ctx = env

    def make():
        rng = np.random.default_rng(q + N)
        lab = rng.integers(0, S, N).astype(np.int32)
        return (rng.standard_normal((N, q)) * 2 + 0.5 + rng.standard_normal((S, q))[lab]).astype(np.float32), lab
    X, lab = GA.cached(("plda stats", q, N), make)

    def run(sk):
        a = GA.Arrays(sk)
        st = api.plda_stats(ctx, a.inp("X", X), a.inp("labels", lab, "int32"), S)
        return a.finish({k: st[k] for k in ("sum", "count", "mean", "sw")})
    got = GA.run_case(("plda stats", q, N), run, skews, "plda stats %s" % skews)
    assert all(np.isfinite(v).all() for v in got.values())
    if skews == {"X": 4}:
        want = PO.class_stats(X, lab, S)
        assert np.array_equal(got["sum"], want["sum"]) and np.array_equal(got["count"], want["count"])
        assert np.abs(got["sw"] - want["sw"]).max() <= 1e-4 * np.abs(want["sw"]).max()
