"""Stream ordering of the two device-pointer entry points of the diarization block, in the pattern of tests/test_snorm_stream_order_gpu.py
(tests/stream_order.py holds the protocol): each call is made while the producer of its input is still in flight on a side stream and its
outputs are consumed on that stream the moment it returns, in the three configurations — owned, borrowed-current, borrowed-stale — and
must equal, bit for bit, the same call on inputs at rest.  Neither api.pairwise_scores nor api.ahc_cluster waits on the host (asserted by
the protocol).  The recordings' segment table is made once per configuration: building one uploads and waits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diarize_oracle as DO         # noqa: E402
import stream_order as SO           # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = (65, 0, 33, DO.N_LDS + 1)     # LDS-resident and workspace-resident recordings


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


def _case():
    X = np.concatenate([DO.cluster_case(n, 4, 32, 0.5, 100 + n)[0] for n in COUNTS if n])
    rng = np.random.RandomState(2)
    psi = np.sort(rng.gamma(2.0, 2.0, 32))[::-1]
    return X, psi


@pytest.mark.parametrize("form", ["cosine", "plda"])
def test_pairwise_scores(cfg, form):
    X, psi = _case()
    seg = cfg.cached("seg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, COUNTS))
    g = h = None
    c0 = 0.0
    if form == "plda":
        g64, h64, c64 = DO.plda_coeffs(psi)
        g, h, c0 = g64.astype(np.float32), h64.astype(np.float32), float(np.float32(c64))

    def call(d, o):
        return {"scores": cfg.api.pairwise_scores(cfg.ctx, d["X"], seg, g, h, c0)}
    base = cfg.race("pairwise scores %s" % form, {"X": X}, call)
    if cfg.mode == "owned":
        ref = DO.pairwise(X, DO.offsets(COUNTS), g, h, c0)
        for G, R in zip(DO.blocks(base["scores"], COUNTS), DO.blocks(ref, COUNTS)):
            assert G.size == 0 or np.abs(G - R).max() <= DO.parity_bound(R)


@pytest.mark.parametrize("linkage", DO.LINKAGES)
def test_ahc_cluster(cfg, linkage):
    X, _ = _case()
    seg = cfg.cached("seg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, COUNTS))
    S = DO.pairwise(X, DO.offsets(COUNTS)).astype(np.float32)
    names = ("labels", "n_clusters", "merge_pair", "merge_score")

    def call(d, o):
        r = cfg.api.ahc_cluster(cfg.ctx, d["scores"], seg, linkage=linkage, threshold=0.5, merges=True)
        return {k: r[k] for k in names}
    base = cfg.race("ahc %s" % linkage, {"scores": S}, call)
    if cfg.mode == "owned":
        want = DO.ahc_batch(S, COUNTS, linkage, 0.5)
        assert all(np.array_equal(base[k], want[k], equal_nan=(k == "merge_score")) for k in names)
