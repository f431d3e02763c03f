"""Stream ordering of the two device-pointer entry points of the sliding-normalisation block, in the pattern of
tests/test_snorm_stream_order_gpu.py (tests/stream_order.py holds the protocol): each call is made while the producer of its inputs is
still in flight on a side stream and its outputs are consumed on that stream the moment it returns, in the three configurations — owned,
borrowed-current, borrowed-stale — and must equal, bit for bit, the same call on inputs at rest.  api.featnorm_sliding returns without a
host wait (asserted by the protocol; the warping table of its window is on the context after the baseline call); api.select_frames
hands its counts back to a host array (one host wait)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featnorm_oracle as FO        # noqa: E402
import stream_order as SO           # noqa: E402

pytestmark = pytest.mark.gpu

LENS = [300, 0, 41, 513]


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


def feats_case():
    rng = np.random.default_rng(70)
    return (rng.standard_normal((sum(LENS), 39)) * 1.5 + 0.5).astype(np.float32)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_featnorm_sliding(cfg, mode):
    """854 frames x 39 over five column groups and six tiles: no host wait"""
    x = feats_case()
    seg = cfg.cached("featnorm seg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, LENS))

    def call(d, o):
        return {"out": cfg.api.featnorm_sliding(cfg.ctx, d["feats"], seg, window=300, mode=mode)}
    base = cfg.race("featnorm sliding mode %d" % mode, {"feats": x}, call)
    if cfg.mode == "owned":
        want, band = FO.sliding_batch(x, seg.offsets, 300, mode)
        FO.check(base["out"], want, band, "featnorm sliding mode %d (stream order)" % mode)


def test_select_frames(cfg):
    """device rows and mask; the counts come back to a host array (one host wait per call).  The mask's poison is another mask: poison
    never indexes memory"""
    x = feats_case()
    mask = (np.random.default_rng(71).random(x.shape[0]) < 0.55).astype(np.uint8)
    seg = cfg.cached("featnorm seg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, LENS))

    def call(d, o):
        rows, kseg, counts = cfg.api.select_frames(cfg.ctx, d["feats"], seg, d["mask"])
        return {"rows": rows, "counts": counts}
    got = cfg.race("select frames", {"feats": x, "mask": mask}, call, poison={"mask": (1 - mask).astype(np.uint8)}, waits=True)
    if cfg.mode == "owned":
        kept, counts = FO.select(x, seg.offsets, mask)
        assert np.array_equal(got["counts"], counts) and np.array_equal(got["rows"].view(np.uint32), kept)
