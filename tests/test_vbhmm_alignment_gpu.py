"""ssp_vbhmm_resegment on device arrays that are NOT 16-byte aligned, in the pattern of tests/test_diarize_alignment_gpu.py
(tests/test_gpu_alignment.py holds the guarded views, the bit-equality rule and the guard checks): X, the initial labels, the cluster
counts and every output at 4-, 8- and 12-byte offsets, bit-equal to the aligned call, guards untouched, and for one skew also checked
against the restatement.  The float64 ELBO travels as pairs of float32 words (the guarded views know no float64): its natural alignment
allows the 8-byte skew only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbhmm_oracle as VO            # noqa: E402
import test_gpu_alignment as GA      # noqa: E402  (Arrays, run_case, p, DEVICE, the env fixture)

pytestmark = pytest.mark.gpu
env = GA.env

COUNTS = (33, 1, 0, 65)
S, Q, ITERS = 16, 32, 3
SKEWS = [{"X": 4}, {"X": 12, "init_labels": 4, "n_init": 8},
         {"labels": 4, "states": 12, "n_speakers": 4, "n_iters": 8, "elbo": 8, "gamma": 4, "pi": 12, "loglik": 8},
         {"X": 8, "init_labels": 12, "n_init": 4, "labels": 12, "states": 4, "n_speakers": 8, "n_iters": 12, "gamma": 12, "pi": 4, "loglik": 4}]


def _case():
    def make():
        parts = [VO.recording_case(n, Q, 3, 1.0, 40 + n) if n > 3 else None for n in COUNTS]
        phi = parts[0][1]
        rng = np.random.RandomState(9)
        X = np.concatenate([p[0] if p else rng.randn(n, Q).astype(np.float32) for p, n in zip(parts, COUNTS)])
        init = np.concatenate([p[3] if p else np.zeros(n, dtype=np.int32) for p, n in zip(parts, COUNTS)])
        ni = np.array([p[4] if p else 1 for p in parts], dtype=np.int32)
        return X, phi, init, ni
    return GA.cached("vbhmm-case", make)


@pytest.mark.parametrize("skews", SKEWS, ids=GA.ids(SKEWS))
def test_vbhmm_resegment_every_array_skewed(env, skews):
    _, api, _lib, ctx = env
    X, phi, init, ni = _case()
    seg = GA.cached("vbhmm-seg", lambda: api.Segments.from_lengths(ctx, COUNTS))
    total, R = sum(COUNTS), len(COUNTS)

    def run(sk):
        a = GA.Arrays(sk)
        x, lab0, n0 = a.inp("X", X), a.inp("init_labels", init, "int32"), a.inp("n_init", ni, "int32")
        lab, st = a.out("labels", (total,), "int32"), a.out("states", (total,), "int32")
        ns, it = a.out("n_speakers", (R,), "int32"), a.out("n_iters", (R,), "int32")
        el = a.out("elbo", (R, ITERS, 2))
        g, pi, ll = a.out("gamma", (total, S)), a.out("pi", (R, S)), a.out("loglik", (total, S))
        _lib.check(ctx._lib.ssp_vbhmm_resegment(ctx._h, GA.p(x), seg._h, Q, phi.ctypes.data, GA.p(lab0), GA.p(n0), S, 0.99, 0.3, 17.0, 5.0, ITERS,
                                                float("-inf"), GA.p(lab), GA.p(st), GA.p(ns), GA.p(it), GA.p(el), GA.p(g), GA.p(pi), GA.p(ll),
                                                GA.DEVICE, None))
        res = a.finish()
        res["elbo"] = np.ascontiguousarray(res["elbo"]).view(np.float64).reshape(R, ITERS)
        res["loglik"] = np.where(np.arange(S)[None, :] < ni.repeat(COUNTS)[:, None], res["loglik"], 0)   # inert columns: unspecified
        for k in ("n_speakers", "n_iters", "pi", "elbo"):                      # (the recording without rows is not written)
            res[k] = res[k][np.array(COUNTS) > 0]
        return res
    what = "vbhmm %s" % skews
    got = GA.run_case("vbhmm", run, skews, what)
    if skews == {"X": 4}:
        want = VO.resegment_batch(X, COUNTS, phi, init, ni, S, max_iters=ITERS, epsilon=-np.inf)
        live = np.array(COUNTS) > 0
        assert np.array_equal(got["n_iters"], want["n_iters"][live]) and np.array_equal(got["n_speakers"], want["n_speakers"][live]), what
        assert np.abs(got["elbo"] - want["elbo"][live]).max() <= 1e-4 * np.abs(want["elbo"][live]).max(), what
        assert np.abs(got["pi"] - want["pi"][live]).max() <= 1e-4, what
