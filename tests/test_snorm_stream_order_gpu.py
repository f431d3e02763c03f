"""Stream ordering of the three device-pointer entry points of the score-normalisation block, in the pattern of
tests/test_gpu_stream_order.py (tests/stream_order.py holds the protocol): each call is made while the producer of its inputs is still in
flight on a side stream and its outputs are consumed on that stream the moment it returns, in the three configurations — owned,
borrowed-current, borrowed-stale — and must equal, bit for bit, the same call on inputs at rest.  api.topn_stats and api.snorm_apply return
without a host wait (asserted by the protocol); api.det_counts hands its counts back to host arrays (one host wait)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snorm_oracle as SN           # noqa: E402
import stream_order as SO           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


@pytest.mark.parametrize("case", [(257, 300, 400, 1), (5, 4097, 300, 1), (200, 70, 40, 0)], ids=lambda c: "%dx%d-top%d-axis%d" % c)
def test_topn_stats(cfg, case):
    """resident rows over 65 workgroups, rows read again per pass, strided columns: no host wait"""
    rows, cols, n, axis = case
    X = SN.topn_case(rows, cols) if axis == 1 else np.ascontiguousarray(SN.topn_case(cols, rows).T)

    def call(d, o):
        r = cfg.api.topn_stats(cfg.ctx, d["scores"], n, axis=axis)
        return {k: r[k] for k in ("mean", "std", "kth")}
    base = cfg.race("topn stats %s" % (case,), {"scores": X}, call)
    if cfg.mode == "owned":
        want = SN.topn_stats(X, n, axis=axis)
        bound = SN.stat_bound(X if axis == 1 else X.T)
        assert np.array_equal(base["kth"], want["kth"])
        assert (np.abs(base["mean"] - want["mean"]) <= bound).all() and (np.abs(base["std"] - want["std"]) <= bound).all()


@pytest.mark.parametrize("inplace", [False, True], ids=["new-matrix", "in-place"])
def test_snorm_apply(cfg, inplace):
    """300 x 70, scores and all four statistics vectors still being produced: no host wait"""
    g = SN.apply_case(300, 70)

    def call(d, o):
        r = cfg.api.snorm_apply(cfg.ctx, d["x"], d["rm"], d["rs"], d["cm"], d["cs"], out=d["x"] if inplace else True)
        return {k: r[k] for k in ("scores", "argmax", "max")}
    base = cfg.race("snorm apply", {k: g[k] for k in ("x", "rm", "rs", "cm", "cs")}, call)
    if cfg.mode == "owned":
        want = SN.apply_f32(g["x"], g["rm"], g["rs"], g["cm"], g["cs"], 1e-6)
        assert np.array_equal(base["scores"], want) and np.array_equal(base["argmax"], SN.decide(want)[0])


def test_det_counts(cfg):
    """device scores and targets; the counts come back to host arrays (one host wait per call).  The targets' poison is a wrong but
    in-range array: poison never indexes memory"""
    x, tgt, th = SN.det_case(300, 70, 1024)
    names = ("tar_hist", "non_hist", "nan_count", "range")

    def call(d, o):
        r = cfg.api.det_counts(cfg.ctx, d["scores"], d["target"], th)
        return {k: r[k] for k in names}
    got = cfg.race("det counts", {"scores": x, "target": tgt}, call, poison={"target": np.where(tgt < 0, 0, (tgt + 1) % 70).astype(np.int32)},
                   waits=True)
    if cfg.mode == "owned":
        want = SN.det_counts(x, tgt, th)
        assert all(np.array_equal(got[k], want[k]) for k in names)
