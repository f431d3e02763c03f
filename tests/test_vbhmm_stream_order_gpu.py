"""Stream ordering of ssp_vbhmm_resegment, in the pattern of tests/test_diarize_stream_order_gpu.py (tests/stream_order.py holds the
protocol): the call is made while the producer of its inputs — the rows, the initial labels and the cluster counts, as when AHC has
just been queued — is still in flight on a side stream and its outputs are consumed on that stream the moment it returns, in the three
configurations, and must equal, bit for bit, the same call on inputs at rest.  api.vb_resegment does not wait on the host (asserted by the
protocol).  The recordings' table is made once per configuration: building one uploads and waits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbhmm_oracle as VO           # noqa: E402
import stream_order as SO           # noqa: E402

pytestmark = pytest.mark.gpu

Q = 32
NAMES = ("labels", "states", "n_speakers", "n_iters", "gamma", "pi", "elbo")


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


def _case(n_states):
    """LDS-resident recordings, one without rows, and one past the residency border of (n_states, Q)"""
    counts = (65, 0, 33, VO.n_lds(n_states, Q) + 1)
    parts = [VO.recording_case(n, Q, 3, 1.0, 60 + n % 97) for n in counts if n]
    X = np.concatenate([p[0] for p in parts])
    init = np.concatenate([p[3] for p in parts])
    ni = np.array([5, 0, 5, 5], dtype=np.int32)
    return counts, X, parts[0][1], init, ni


@pytest.mark.parametrize("n_states", [16, 64])
def test_vb_resegment(cfg, n_states):
    counts, X, phi, init, ni = _case(n_states)
    seg = cfg.cached(("seg", n_states), lambda: cfg.api.Segments.from_lengths(cfg.ctx, counts))
    # wrong but in-range labels and counts as the poison of the integer inputs: a race is a wrong number, nothing more
    poison = {"init_labels": (init + 1) % 5, "n_init": np.array([1, 1, 1, 1], dtype=np.int32)}

    def call(d, o):
        r = cfg.api.vb_resegment(cfg.ctx, d["X"], seg, phi, d["init_labels"], d["n_init"], n_states=n_states, max_iters=3, epsilon=-np.inf)
        return {k: r[k] for k in NAMES}
    base = cfg.race("vb resegment S=%d" % n_states, {"X": X, "init_labels": init, "n_init": ni}, call, poison=poison)
    if cfg.mode == "owned":
        want = VO.resegment_batch(X, counts, phi, init, ni, n_states, max_iters=3, epsilon=-np.inf)
        assert np.array_equal(base["n_iters"], want["n_iters"])
        fin = np.isfinite(want["elbo"])
        assert np.array_equal(np.isfinite(base["elbo"]) | (np.array(counts) == 0)[:, None], fin | (np.array(counts) == 0)[:, None])
        assert (np.abs(base["elbo"][fin] - want["elbo"][fin]) <= 1e-4 * np.abs(want["elbo"][fin])).all()
