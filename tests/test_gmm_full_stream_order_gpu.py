"""Stream ordering of the two device-pointer entry points of the full-covariance GMM feature, in the pattern of
tests/test_gmm_map_stream_order_gpu.py (tests/stream_order.py holds the protocol): each call is made while the producer of its features is
still in flight on a side stream and its outputs are consumed on that stream the moment it returns, in the three configurations, and must
equal, bit for bit, the same call on inputs at rest.  api.GmmFullScorer.score returns without a host wait (asserted by the protocol);
api.gmm_full_em_stats hands its sums back to host arrays (one host wait)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_full_cases as FC         # noqa: E402
import stream_order as SO           # noqa: E402

pytestmark = pytest.mark.gpu

LENS = [0, 1, 70, 300, 33, 129]


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


@pytest.mark.parametrize("loglik", [True, False])
def test_full_score(cfg, loglik):
    """4 models with a UBM, K = 5, D = 39: no host wait, with and without loglik_out"""
    c = FC.scorer_case(4, True, K=5, D=39, lens=LENS)
    sc, seg = cfg.cached("full", lambda: (cfg.api.GmmFullScorer(cfg.ctx, c["w"], c["mus"], c["Us"], has_ubm=True),
                                          cfg.api.Segments.from_lengths(cfg.ctx, LENS)))
    names = ("loglik", "scores", "argmax") if loglik else ("scores", "argmax")

    def call(d, o):
        r = sc.score(d["feats"], seg, loglik=loglik)
        return {n: r[n] for n in names}
    base = cfg.race("full score loglik %d" % loglik, {"feats": c["X"]}, call)
    if cfg.mode == "owned" and loglik:
        FC.compare_loglik(base["loglik"], c["ref_ll"], c["emu_ll"], "full score")


def test_full_em_stats(cfg):
    """device frames; the sums come back to host arrays (one host wait per call)"""
    c = FC.em_case(5, 39, 257, 30.0)
    api, ctx = cfg.api, cfg.ctx

    def call(d, o):
        st = api.gmm_full_em_stats(ctx, c["w"], c["mu"], c["U"], d["X"], shift=c["shift"])
        return {"nk": st["nk"], "sx": st["sx"], "sxx": st["sxx"], "ll": np.array([st["loglik_sum"]])}
    got = cfg.race("full em stats", {"X": c["X"]}, call, waits=True)
    assert all(np.isfinite(v).all() for v in got.values())
