"""GPU tests of the VB-HMM resegmentation (run with -m gpu on an MI355X) against tests/vbhmm_oracle.py, which tests/test_vbhmm_host.py
corroborates.  One iteration on a ragged batch with spread posteriors (noise 3): loglik within the project's parity bound,
1e-4 max(1, max |ref|) per recording; gamma within 1e-4 of the oracle's forward-backward FED THE DEVICE'S OWN loglik (the same bound, as
gamma <= 1), rows summing to 1 within 1e-5, inert columns exactly 0.  The end-to-end cases have saturated posteriors after every
iteration (asserted on the CPU), so d gamma <= gamma (1 - gamma) d ll carries the 1e-4 through the iterations and labels, states and
speaker counts are EQUAL.  Every check prints measured error over bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbhmm_oracle as VO  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ("gamma", "pi", "elbo", "loglik")
BASE_COUNTS = (0, 1, 2, 63, 64, 65, 200)
ONE_ITER = [(16, 64, True), (1, 1, True), (2, 7, False), (7, 130, True), (64, 130, False), (64, 512, True)]   # (S, q, n_init given)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def env():
    from speech_signal_processing_amd import api, _lib
    return api, _lib, api.default_context()


def _counts(S, q):
    """the ragged batch plus one recording on each side of the residency border of (S, q); the pairs cover alpha in LDS and (64, 512)
    alpha in the workspace"""
    return BASE_COUNTS + (VO.n_lds(S, q), VO.n_lds(S, q) + 1)


def _spread_batch(S, q, with_n_init):
    rng = np.random.RandomState(S * 1000 + q)
    counts = _counts(S, q)
    k = max(1, min(S, 4))
    phi = (4.0 * np.sort(rng.gamma(2.0, 0.5, q))[::-1]).astype(np.float32)
    means = rng.randn(k, q) * np.sqrt(phi)[None, :]
    X = np.concatenate([(means[rng.randint(k, size=n)] + 3.0 * rng.randn(n, q)).astype(np.float32) for n in counts])
    lab = rng.randint(-1, S + 1, size=sum(counts)).astype(np.int32)           # labels outside [0, S) included
    ni = rng.randint(0, S + 2, size=len(counts)).astype(np.int32) if with_n_init else None
    return X, counts, phi, lab, ni


@pytest.mark.parametrize("S,q,with_n_init", ONE_ITER, ids=["S%d-q%d-%s" % (s, q, "ninit" if n else "null") for s, q, n in ONE_ITER])
def test_one_iteration_on_a_ragged_batch(env, S, q, with_n_init):
    api, _lib, ctx = env
    assert VO.alpha_in_lds(S, q) == (not (S == 64 and q == 512))
    X, counts, phi, lab, ni = _spread_batch(S, q, with_n_init)
    got = api.vb_resegment(ctx, X, counts, phi, lab, ni, n_states=S, max_iters=1, want=ALL)
    ref = VO.resegment_batch(X, counts, phi, lab, ni, S, max_iters=1)
    off = np.concatenate([[0], np.cumsum(counts)])
    worst = {"loglik": 0.0, "gamma": 0.0, "rowsum": 0.0}
    spread = 0
    for r, n in enumerate(counts):
        a, b = off[r], off[r + 1]
        if n == 0:
            assert got["n_iters"][r] == 0 and got["n_speakers"][r] == 0
            continue
        Sr = S if ni is None else min(max(int(ni[r]), 1), S)
        R = ref["loglik"][a:b, :Sr]
        ll = got["loglik"][a:b, :Sr].astype(np.float64)
        worst["loglik"] = max(worst["loglik"], np.abs(ll - R).max() / (1e-4 * max(1.0, np.abs(R).max())))
        fed = VO.forward_backward(ll, np.full(Sr, 1.0 / Sr), 0.99)[0]
        g = got["gamma"][a:b]
        worst["gamma"] = max(worst["gamma"], np.abs(g[:, :Sr] - fed).max() / 1e-4)
        worst["rowsum"] = max(worst["rowsum"], np.abs(g.astype(np.float64).sum(axis=1) - 1).max() / 1e-5)
        spread += int((np.minimum(fed, 1 - fed).max(axis=1) > 1e-3).sum())
        assert (g[:, Sr:] == 0).all() and (got["pi"][r, Sr:] == 0).all(), "inert columns of recording %d" % r
        assert got["n_iters"][r] == 1 and np.isfinite(got["elbo"][r, 0])
        assert abs(got["elbo"][r, 0] - ref["elbo"][r, 0]) <= 1e-4 * max(1.0, abs(ref["elbo"][r, 0]))
        assert abs(float(got["pi"][r].sum()) - 1) <= 1e-5
    for k, v in worst.items():
        print("[measured] S=%d q=%d %s: error / bound %.3g" % (S, q, k, v))
    print("[measured] S=%d q=%d rows with an unsaturated posterior: %d of %d" % (S, q, spread, sum(counts)))
    assert S == 1 or spread > 0.02 * sum(counts)          # the posteriors ARE spread: the gamma check is not vacuous
    assert max(worst.values()) <= 1.0, worst


def _e2e(i):
    def make():
        X, phi, truth, init, ni = VO.e2e_case(i)
        return X, phi, truth, init, ni, {mi: VO.resegment(X, phi, init, ni, S=VO.E2E_STATES, max_iters=mi, epsilon=-np.inf) for mi in (2, 10)}
    return cached(("e2e", i), make)


@pytest.mark.parametrize("max_iters", [2, 10])
@pytest.mark.parametrize("case", range(len(VO.E2E_CASES)))
def test_end_to_end_cases(env, case, max_iters):
    api, _lib, ctx = env
    X, phi, truth, init, ni, refs = _e2e(case)
    ref = refs[max_iters]
    got = api.vb_resegment(ctx, X, [X.shape[0]], phi, init, np.array([ni], dtype=np.int32), n_states=VO.E2E_STATES, max_iters=max_iters,
                           epsilon=-np.inf)
    assert np.array_equal(got["labels"], ref["labels"]) and np.array_equal(got["states"], ref["states"])
    assert got["n_speakers"].tolist() == [ref["n_speakers"]] and got["n_iters"].tolist() == [max_iters]
    assert VO.same_partition(got["labels"], truth) and (init != truth).any()
    e_g, e_p = np.abs(got["gamma"] - ref["gamma"]).max() / 1e-4, np.abs(got["pi"][0] - ref["pi"]).max() / 1e-4
    e_e = (np.abs(got["elbo"][0] - ref["elbo"]) / (1e-4 * np.maximum(1.0, np.abs(ref["elbo"])))).max()
    print("[measured] case %d max_iters %d: error / bound gamma %.3g pi %.3g elbo %.3g" % (case, max_iters, e_g, e_p, e_e))
    assert e_g <= 1 and e_p <= 1 and e_e <= 1


def test_early_stop(env):
    api, _lib, ctx = env
    X, counts, phi, init, ni = VO.early_batch()
    ref = cached("early", lambda: VO.resegment_batch(X, counts, phi, init, ni, VO.E2E_STATES, max_iters=10, epsilon=VO.EARLY_EPS))
    got = api.vb_resegment(ctx, X, counts, phi, init, ni, n_states=VO.E2E_STATES, max_iters=10, epsilon=VO.EARLY_EPS)
    assert got["n_iters"].tolist() == ref["n_iters"].tolist() and len(set(ref["n_iters"].tolist())) > 1
    for r, n in enumerate(ref["n_iters"]):
        assert np.isnan(got["elbo"][r, n:]).all() and np.isfinite(got["elbo"][r, :n]).all()
        assert (np.abs(got["elbo"][r, :n] - ref["elbo"][r, :n]) <= 1e-4 * np.maximum(1.0, np.abs(ref["elbo"][r, :n]))).all()
    # the results are those of the last iteration run: the same call cut at each recording's own count
    off = np.concatenate([[0], np.cumsum(counts)])
    for r, n in enumerate(ref["n_iters"]):
        a, b = off[r], off[r + 1]
        cut = api.vb_resegment(ctx, X[a:b], [b - a], phi, init[a:b], ni[r:r + 1], n_states=VO.E2E_STATES, max_iters=int(n), epsilon=-np.inf)
        assert np.array_equal(cut["gamma"], got["gamma"][a:b]) and np.array_equal(cut["pi"][0], got["pi"][r])
        assert np.array_equal(cut["labels"], got["labels"][a:b]) and np.array_equal(cut["states"], got["states"][a:b])


# ---------------------------------------------------------------------------------------------------------------------- contracts
def _contract_batch():
    return cached("contract", lambda: _spread_batch(16, 64, True))


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v) for v in (a[k], b[k]))
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


def test_same_call_same_bits_and_host_route_equals_device_route(env):
    import torch
    api, _lib, ctx = env
    X, counts, phi, lab, ni = _contract_batch()
    kw = dict(n_states=16, max_iters=3, epsilon=-np.inf, want=ALL)
    a = api.vb_resegment(ctx, X, counts, phi, lab, ni, **kw)
    b = api.vb_resegment(ctx, X, counts, phi, lab, ni, **kw)
    _same(a, b)
    d = api.vb_resegment(ctx, torch.from_numpy(X).cuda(), counts, phi, torch.from_numpy(lab).cuda(), torch.from_numpy(ni).cuda(), **kw)
    assert all(v.is_cuda for v in d.values())
    _same(a, d)


def test_a_recording_alone_gives_its_batch_bits(env):
    api, _lib, ctx = env
    X, counts, phi, lab, ni = _contract_batch()
    kw = dict(n_states=16, max_iters=3, epsilon=-np.inf, want=ALL)
    full = api.vb_resegment(ctx, X, counts, phi, lab, ni, **kw)
    off = np.concatenate([[0], np.cumsum(counts)])
    for r in (1, 4, 6, 7, 8):                    # one row, 64 rows, 200 rows and both sides of the residency border
        a, b = off[r], off[r + 1]
        one = api.vb_resegment(ctx, X[a:b], [b - a], phi, lab[a:b], ni[r:r + 1], **kw)
        for k in ("labels", "states", "gamma", "loglik"):
            assert np.array_equal(one[k], full[k][a:b], equal_nan=True), (r, k)
        for k in ("n_speakers", "n_iters", "pi", "elbo"):
            assert np.array_equal(one[k][0], full[k][r], equal_nan=True), (r, k)


def test_chain_from_ahc_runs_on_device_tensors(env):
    """pairwise scores -> AHC -> VB-HMM on torch tensors: the AHC outputs are handed over as they are, nothing is copied to the host
    in between, and the result equals the host route fed the same labels"""
    import torch
    api, _lib, ctx = env
    X, phi, truth, init, ni, _ = _e2e(1)
    from speech_signal_processing_amd import plda
    g, h, c0 = plda.pairwise_coeffs(phi.astype(np.float64))
    seg = api.Segments.from_lengths(ctx, [X.shape[0]])
    dX = torch.from_numpy(X).cuda()
    r = api.ahc_cluster(ctx, api.pairwise_scores(ctx, dX, seg, g=g, h=h, c0=c0), seg, threshold=0.0)
    assert r["labels"].is_cuda and r["n_clusters"].is_cuda
    v = api.vb_resegment(ctx, dX, seg, phi, r["labels"], r["n_clusters"])
    assert all(t.is_cuda for t in v.values()) and v["gamma"].shape == (X.shape[0], 64)
    host = api.vb_resegment(ctx, X, seg, phi, r["labels"].cpu().numpy(), r["n_clusters"].cpu().numpy(), n_states=64)
    _same({k: v[k] for k in ("labels", "states", "n_speakers", "n_iters", "gamma")}, {k: host[k] for k in ("labels", "states", "n_speakers", "n_iters", "gamma")})
    assert VO.same_partition(v["labels"].cpu().numpy(), truth)


def test_a_non_finite_row_poisons_only_its_recording(env):
    api, _lib, ctx = env
    X, counts, phi, lab, ni = _contract_batch()
    kw = dict(n_states=16, max_iters=2, epsilon=-np.inf, want=ALL)
    clean = api.vb_resegment(ctx, X, counts, phi, lab, ni, **kw)
    off = np.concatenate([[0], np.cumsum(counts)])
    bad = X.copy()
    bad[off[5] + 7, 3] = np.nan
    bad[off[3], 0] = -np.inf
    got = api.vb_resegment(ctx, bad, counts, phi, lab, ni, **kw)
    for r, n in enumerate(counts):
        a, b = off[r], off[r + 1]
        if r in (3, 5):
            assert (got["labels"][a:b] == -1).all() and (got["states"][a:b] == -1).all() and got["n_speakers"][r] == -1 and got["n_iters"][r] == 0
            assert np.isnan(got["gamma"][a:b]).all() and np.isnan(got["loglik"][a:b]).all() and np.isnan(got["pi"][r]).all()
            assert np.isnan(got["elbo"][r]).all()
        else:
            for k in ("labels", "states", "gamma", "loglik"):
                assert np.array_equal(got[k][a:b], clean[k][a:b]), (r, k)
            for k in ("n_speakers", "n_iters", "pi", "elbo"):
                assert np.array_equal(got[k][r], clean[k][r], equal_nan=True), (r, k)


def test_error_codes_and_the_context_stays_usable(env):
    api, _lib, ctx = env
    X, phi, truth, init, ni, refs = _e2e(0)
    T, q = X.shape
    seg = api.Segments.from_lengths(ctx, [T])
    lab = np.zeros(T, dtype=np.int32)
    outs = [np.zeros(T, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]

    def call(q_=q, S=4, P=0.9, Fa=0.3, Fb=17.0, sm=5.0, mi=2, eps=1e-4, ph=phi, seg_=seg):
        ph = np.ascontiguousarray(ph, dtype=np.float32)
        return ctx._lib.ssp_vbhmm_resegment(ctx._h, X.ctypes.data, seg_._h, q_, ph.ctypes.data, lab.ctypes.data, None, S, P, Fa, Fb, sm, mi,
                                            eps, outs[0].ctypes.data, None, outs[1].ctypes.data, outs[2].ctypes.data, None, None, None, None,
                                            _lib.HOST, None)
    nan, inf = float("nan"), float("inf")
    neg, bad = phi.copy(), phi.copy()
    neg[1], bad[2] = -1.0, np.inf
    invalid = [dict(q_=0), dict(S=0), dict(mi=0), dict(P=-0.1), dict(P=1.0), dict(P=nan), dict(Fa=0.0), dict(Fa=inf), dict(Fa=nan),
               dict(Fb=-1.0), dict(Fb=inf), dict(sm=-1.0), dict(sm=inf), dict(sm=nan), dict(eps=nan), dict(ph=neg), dict(ph=bad)]
    for kw in invalid:
        assert call(**kw) == _lib.SSP_ERR_INVALID, kw
    long_seg = api.Segments.from_lengths(ctx, [4097])
    for kw in (dict(S=65), dict(q_=1025, ph=np.ones(1025)), dict(mi=101), dict(seg_=long_seg)):
        assert call(**kw) == _lib.SSP_ERR_UNSUPPORTED, kw
    assert call(eps=-inf, mi=5) == _lib.SSP_OK and outs[2][0] == 5                                 # -inf never stops early
    assert call(eps=inf, mi=5) == _lib.SSP_OK and outs[2][0] == 2                                  # +inf stops after the second iteration
    with pytest.raises(ValueError):
        api.vb_resegment(ctx, X, [T], phi, init, loop_prob=1.0)
    with pytest.raises(NotImplementedError):
        api.vb_resegment(ctx, X, [T], phi, init, max_iters=101)
    got = api.vb_resegment(ctx, X, [T], phi, init, np.array([ni], dtype=np.int32), n_states=VO.E2E_STATES, max_iters=2, epsilon=-np.inf)
    assert np.array_equal(got["labels"], refs[2]["labels"])                                        # after the errors the next call works
    empty = api.vb_resegment(ctx, np.zeros((0, q), dtype=np.float32), [0, 0], phi, np.zeros(0, dtype=np.int32), n_states=3)
    assert empty["labels"].shape == (0,) and empty["n_iters"].tolist() == [0, 0] and empty["gamma"].shape == (0, 3)
    none = api.vb_resegment(ctx, np.zeros((0, q), dtype=np.float32), [], phi, np.zeros(0, dtype=np.int32), n_states=3)
    assert none["n_speakers"].shape == (0,)


# ------------------------------------------------------------------------------------------------------------------- the Diarizer
class _Plda:
    """the back end the Diarizer asks for, on an already diagonalised space: project is the identity"""

    def __init__(self, psi):
        self.psi_ = np.asarray(psi, dtype=np.float64)

    def project(self, X):
        return X

    def pairwise_coeffs(self):
        from speech_signal_processing_amd import plda
        return plda.pairwise_coeffs(self.psi_)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_diarizer_with_resegmentation_equals_the_composed_calls(env, kind):
    import torch
    from speech_signal_processing_amd import diarize
    api, _lib, ctx = env
    cases = [_e2e(i) for i in (0, 0)]
    X = np.concatenate([c[0] for c in cases])
    counts = [c[0].shape[0] for c in cases]
    phi = cases[0][1]
    back = _Plda(phi)
    thr = 20.0                                                  # over-split on purpose: the VB pass lets the extra clusters die out
    dz = diarize.Diarizer(back, threshold=thr, ctx=ctx, resegment=True)
    rows = torch.from_numpy(X).cuda() if kind == "torch" else X
    labels, n_spk = dz.cluster(rows, counts)
    g, h, c0 = back.pairwise_coeffs()
    seg = api.Segments.from_lengths(ctx, counts)
    r = api.ahc_cluster(ctx, api.pairwise_scores(ctx, rows, seg, g=g, h=h, c0=c0), seg, threshold=thr)
    v = api.vb_resegment(ctx, rows, seg, phi.astype(np.float32), r["labels"], r["n_clusters"])
    _same({"labels": labels, "n": n_spk}, {"labels": v["labels"], "n": v["n_speakers"]})
    assert (kind == "torch") == bool(getattr(labels, "is_cuda", False))
    plain_labels, plain_n = diarize.Diarizer(back, threshold=thr, ctx=ctx).cluster(rows, counts)
    _same({"labels": plain_labels, "n": plain_n}, {"labels": r["labels"], "n": r["n_clusters"]})
    lab = labels.cpu().numpy() if kind == "torch" else labels
    ahc = plain_labels.cpu().numpy() if kind == "torch" else plain_labels
    T, truth = counts[0], cases[0][2]
    assert VO.same_partition(lab[:T], truth), "the resegmented labels are right"
    assert not VO.same_partition(ahc[:T], truth), "plain AHC's are not (this is what the pass is for)"
