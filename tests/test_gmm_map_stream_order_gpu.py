"""Stream ordering of the two device-pointer entry points of the MAP / top-C feature, in the pattern of tests/test_gpu_stream_order.py
(tests/stream_order.py holds the protocol): each call is made while the producer of its features is still in flight on a side stream and
its outputs are consumed on that stream the moment it returns, in the three configurations — owned, borrowed-current, borrowed-stale —
and must equal, bit for bit, the same call on inputs at rest.  api.MapScorer.score returns without a host wait (asserted by the
protocol); api.gmm_em_stats_shared hands its sums back to host arrays (one host wait)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_oracle as MO             # noqa: E402
import stream_order as SO           # noqa: E402
from test_gmm_map_gpu import ATOL, RTOL, make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

_DATA = {}


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


def _data():
    if not _DATA:
        rng = np.random.default_rng(17)
        _DATA.update(make_inputs(70, 39, 12, 171, lens=list(rng.integers(5, 60, 300))))
    return _DATA


def test_map_score(cfg):
    """K = 70, D = 39, 12 speakers, C = 5, 300 utterances of 5 .. 59 frames: no host wait"""
    g = _data()
    sc, seg = cfg.cached("map", lambda: (cfg.api.MapScorer(cfg.ctx, g["w"], g["mu"], g["cv"], g["sm"]),
                                         cfg.api.Segments.from_lengths(cfg.ctx, g["lens"])))
    names = ("diff", "ubm", "argmax", "idx")

    def call(d, o):
        r = sc.score(d["feats"], seg, top_c=5, ubm=True, idx=True)
        return {n: r[n] for n in names}
    base = cfg.race("map score", {"feats": g["X"]}, call)
    if cfg.mode == "owned":
        ref = MO.topc_scores(g["w"], g["mu"], g["cv"], g["sm"], g["X"], g["off"], 5, idx=base["idx"])
        assert (np.abs(base["diff"] - ref["diff"]) <= ATOL + RTOL * np.abs(ref["diff"])).all()
        assert (np.abs(base["ubm"] - ref["ubm"]) <= ATOL + RTOL * np.abs(ref["ubm"])).all()


def test_em_stats_shared(cfg):
    """device frames; the sums come back to host arrays (one host wait per call): three overlapping ranges, the batch call's bits"""
    g = _data()
    api, ctx = cfg.api, cfg.ctx
    off, cnt = np.array([0, 100, 37]), np.array([500, 400, 203])

    def shared(d, o):
        st = api.gmm_em_stats_shared(ctx, g["w"], g["mu"], g["cv"], d["X"], off, cnt)
        return {"nk": st["nk"], "sx": st["sx"], "sxx": st["sxx"], "ll": st["loglik_sum"]}
    got = cfg.race("em stats shared", {"X": g["X"]}, shared, waits=True)
    rep = api.gmm_em_stats_batch(ctx, np.stack([g["w"]] * 3), np.stack([g["mu"]] * 3), np.stack([g["cv"]] * 3), g["X"], off, cnt)
    assert all(np.array_equal(got[a], rep[b]) for a, b in (("nk", "nk"), ("sx", "sx"), ("sxx", "sxx"), ("ll", "loglik_sum")))
