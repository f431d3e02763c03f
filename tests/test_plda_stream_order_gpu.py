"""Stream ordering of the two device-pointer entry points of the PLDA back end, in the pattern of tests/test_gpu_stream_order.py
(tests/stream_order.py holds the protocol): each call is made while the producer of its inputs is still in flight on a side stream and its
outputs are consumed on that stream the moment it returns, in the three configurations — owned, borrowed-current, borrowed-stale — and must
equal, bit for bit, the same call on inputs at rest.  api.PldaScorer.score returns without a host wait (asserted by the protocol);
api.plda_stats hands its sums back to host arrays (one host wait)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_oracle as PO            # noqa: E402
import stream_order as SO           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


@pytest.mark.parametrize("idx,flags", [(8, 0), (8, 1)], ids=["class-shared", "general"])
def test_plda_score(cfg, idx, flags):
    """q = 256, 70 speakers, 300 test vectors (three workgroups): no host wait"""
    g = PO.scorer_case(PO.SCORER_CASES[idx])
    sc = cfg.cached(("plda", idx, flags), lambda: cfg.api.PldaScorer(cfg.ctx, g["psi"], g["enrol"], g["counts"], flags=flags))

    def call(d, o):
        r = sc.score(d["T"], llr=True)
        return {n: r[n] for n in ("llr", "argmax", "max")}
    base = cfg.race("plda score", {"T": g["T"]}, call)
    if cfg.mode == "owned":
        assert (np.abs(base["llr"] - g["ref"]).max(axis=1) <= PO.llr_bound(g["ref"])).all()
        assert np.array_equal(base["argmax"][g["keep"]], g["ref"].argmax(axis=1)[g["keep"]])


def test_plda_stats(cfg):
    """device rows and labels; the statistics come back to host arrays (one host wait per call).  The labels' poison is a wrong but
    in-range array: poison never indexes memory"""
    rng = np.random.default_rng(23)
    N, q, S = 2500, 64, 7
    lab = rng.integers(0, S, N).astype(np.int32)
    X = (rng.standard_normal((N, q)) + rng.standard_normal((S, q))[lab]).astype(np.float32)
    api, ctx = cfg.api, cfg.ctx

    def call(d, o):
        st = api.plda_stats(ctx, d["X"], d["labels"], S)
        return {k: st[k] for k in ("sum", "count", "mean", "sw")}
    got = cfg.race("plda stats", {"X": X, "labels": lab}, call, poison={"labels": (lab + 1) % S}, waits=True)
    if cfg.mode == "owned":
        want = PO.class_stats(X, lab, S)
        assert np.array_equal(got["sum"], want["sum"]) and np.array_equal(got["count"], want["count"])
        assert np.abs(got["sw"] - want["sw"]).max() <= 1e-4 * np.abs(want["sw"]).max()
