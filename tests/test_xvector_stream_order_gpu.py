"""Stream ordering of the three device-pointer entry points of the x-vector block, in the pattern of
tests/test_diarize_stream_order_gpu.py (tests/stream_order.py holds the protocol): each call is made while the producer of its input is
still in flight on a side stream and its outputs are consumed on that stream the moment it returns, in the three configurations — owned,
borrowed-current, borrowed-stale — and must equal, bit for bit, the same call on inputs at rest.  None of api.tdnn_forward,
api.stats_pool and XVectorForward.forward waits on the host once the network's buffers have grown (asserted by the protocol: the
baseline call grows them).  The segment table and the network are made once per configuration: building one uploads and waits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xvector_oracle as XO         # noqa: E402
import stream_order as SO           # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = (131, 0, 9, 140)
WINS = np.array([[0, 0, 131], [0, 30, 90], [2, 0, 9], [3, 0, 140], [3, 70, 140]], dtype=np.int64)


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


def _layers():
    rng = np.random.RandomState(21)
    spec = [(u, t, d, True) for u, (t, d) in zip((40, 40, 40, 40, 52), XO.SNYDER)]
    fl, sl = XO.random_layers(rng, 13, spec, segment=[(300, True), (30, False)])
    return fl, sl, rng.randn(sum(COUNTS), 13).astype(np.float32)


def test_tdnn_forward(cfg):
    fl, _, feats = _layers()
    L = fl[0]
    seg = cfg.cached("seg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, COUNTS))

    def call(d, o):
        Y, _ = cfg.api.tdnn_forward(cfg.ctx, d["X"], seg, d["W"], d["b"], dilation=L["dilation"], relu=True, scale=d["scale"], offset=d["offset"])
        return {"Y": Y}
    base = cfg.race("tdnn forward", {"X": feats, "W": L["W"], "b": L["b"], "scale": L["scale"], "offset": L["offset"]}, call)
    if cfg.mode == "owned":
        off = np.concatenate([[0], np.cumsum(COUNTS)])
        for i in range(len(COUNTS)):
            x = feats[off[i]:off[i + 1]]
            ref = XO.layer(x, L)
            assert (np.abs(base["Y"][off[i]:off[i] + ref.shape[0]] - ref) <= XO.layer_bound(x, L)).all()


def test_stats_pool(cfg):
    X = np.random.RandomState(5).randn(sum(COUNTS), 300).astype(np.float32)
    seg = cfg.cached("seg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, COUNTS))

    def call(d, o):
        return {"out": cfg.api.stats_pool(cfg.ctx, d["X"], seg, WINS)}
    base = cfg.race("stats pool", {"X": X}, call)
    if cfg.mode == "owned":
        off = np.concatenate([[0], np.cumsum(COUNTS)])
        ref = np.stack([XO.pool(X[off[q] + a:off[q] + b]) for q, a, b in WINS])
        assert np.array_equal(np.isnan(base["out"]), np.isnan(ref)) and np.nanmax(np.abs(base["out"] - ref)) <= 1e-4 * max(1.0, np.nanmax(np.abs(ref)))


@pytest.mark.parametrize("windows", [False, True])
def test_xvector_forward(cfg, windows):
    fl, sl, feats = _layers()
    seg = cfg.cached("seg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, COUNTS))
    fwd = cfg.cached("net", lambda: cfg.api.XVectorForward(cfg.ctx, fl, sl))

    def call(d, o):
        return {"emb": fwd.forward(d["feats"], seg, WINS if windows else None)}
    base = cfg.race("xvector forward windows=%s" % windows, {"feats": feats}, call)
    if cfg.mode == "owned":
        ref = XO.network(feats, COUNTS, fl, sl, windows=WINS.tolist() if windows else None)
        assert np.array_equal(np.isnan(base["emb"]), np.isnan(ref))
        assert np.nanmax(np.abs(base["emb"] - ref)) <= 1e-4 * max(1.0, np.nanmax(np.abs(ref)))
