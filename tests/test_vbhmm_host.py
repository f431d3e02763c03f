"""Host tests of the VB-HMM resegmentation block (no GPU).  tests/vbhmm_oracle.py, the yardstick of tests/test_vbhmm_gpu.py, has no outside
pin, so it is corroborated here: (a) forward-backward against brute-force enumeration of all state paths, (b) the M step against the
dense linear-Gaussian posterior of a speaker variable, (c) the structured O(T S) recursion against the dense one, (d) the ELBO never
decreases at Fa = Fb = 1, (e) the label convention, the uniform row and the non-finite rule.  The conditions the GPU tests rest on —
saturated posteriors after every iteration of the end-to-end cases, ELBO deltas clear of the early-stop epsilon — are asserted here too,
and the surface (header, binding, Python names)."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbhmm_oracle as VO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ (a) brute-force paths
def _brute(ll, pi, P):
    """posteriors, ln p(X) and the expected non-loop arrivals per state by enumeration of all S^T paths"""
    T, S = ll.shape
    tr = VO.transition(pi, P)
    post, arrive, total = np.zeros((T, S)), np.zeros(S), 0.0
    for z in itertools.product(range(S), repeat=T):
        p = pi[z[0]] * np.exp(ll[0, z[0]])
        for t in range(1, T):
            p *= tr[z[t - 1], z[t]] * np.exp(ll[t, z[t]])
        total += p
        for t in range(T):
            post[t, z[t]] += p
        arrive[z[0]] += p
        for t in range(1, T):
            j = z[t]
            arrive[j] += p * ((1 - P) * pi[j] / tr[j, j] if z[t - 1] == j else 1.0)
    return post / total, np.log(total), arrive / arrive.sum()


@pytest.mark.parametrize("T,S,P", [(1, 1, 0.5), (1, 3, 0.9), (4, 2, 0.0), (6, 3, 0.99), (5, 3, 0.3), (6, 2, 0.7)])
def test_forward_backward_equals_enumeration_of_all_paths(T, S, P):
    rng = np.random.RandomState(100 * T + S)
    ll = 2.0 * rng.randn(T, S) - 3.0
    pi = rng.dirichlet(np.ones(S))
    gamma, lnp, lfw, lbw, _ = VO.forward_backward(ll, pi, P)
    post, lnp_b, pi_b = _brute(ll, pi, P)
    assert np.abs(gamma - post).max() <= 1e-12 and abs(lnp - lnp_b) <= 1e-12
    assert np.abs(VO.pi_update(gamma, lfw, lbw, ll, lnp, pi, P) - pi_b).max() <= 1e-12
    assert np.abs(gamma.sum(axis=1) - 1).max() <= 1e-12


# ------------------------------------------------------------------------------------------------- (b) the dense linear-Gaussian posterior
def test_m_step_is_the_posterior_of_a_speaker_variable():
    """x_t = V y + e, y ~ N(0, I), e ~ N(0, I), V = diag(sqrt(phi)): with the N rows of a state stacked, A = [V; ...; V], the posterior of
    y is N(A^T (A A^T + I)^-1 x, I - A^T (A A^T + I)^-1 A) — full matrices, no use of the diagonal structure"""
    rng = np.random.RandomState(3)
    q, T, S = 5, 9, 3
    phi = rng.gamma(2.0, 1.0, q)
    X = rng.randn(T, q) * 2
    lab = np.array([0, 0, 1, 2, 2, 2, 0, 1, 2])
    gamma = np.eye(S)[lab]
    N, invL, alpha = VO.m_step(X, phi, gamma, 1.0, 1.0)
    V = np.diag(np.sqrt(phi))
    for s in range(S):
        rows = X[lab == s]
        n = rows.shape[0]
        A = np.concatenate([V] * n, axis=0)
        K = A.T @ np.linalg.inv(A @ A.T + np.eye(n * q))
        mean, cov = K @ rows.reshape(-1), np.eye(q) - K @ A
        assert N[s] == n
        assert np.abs(alpha[s] - mean).max() <= 1e-12
        assert np.abs(np.diag(invL[s]) - cov).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------ (c) structured against dense
@pytest.mark.parametrize("T,S,P,dead", [(40, 5, 0.99, 0), (40, 5, 0.0, 0), (17, 1, 0.9, 0), (60, 7, 0.8, 2), (1, 4, 0.5, 1)])
def test_structured_recursion_equals_the_dense_one(T, S, P, dead):
    """dead: states whose prior is exactly 0 (what an inert or extinct state is inside the recursion)"""
    rng = np.random.RandomState(T + S)
    ll = 5.0 * rng.randn(T, S) - 40.0
    pi = rng.dirichlet(np.ones(S))
    pi[:dead] = 0.0
    pi /= pi.sum()
    g, lnp, lfw, lbw, _ = VO.forward_backward(ll, pi, P)
    new = VO.pi_update(g, lfw, lbw, ll, lnp, pi, P)
    g2, lnp2, new2 = VO.forward_backward_structured(ll, pi, P)
    assert np.abs(g - g2).max() <= 1e-10 and abs(lnp - lnp2) <= 1e-10 * max(1.0, abs(lnp)) and np.abs(new - new2).max() <= 1e-10
    assert (g2[:, :dead] == 0).all() and (new2[:dead] == 0).all()


def test_inert_states_of_the_full_run():
    X, phi, _, init, ni = VO.e2e_case(0)
    a = VO.resegment(X, phi, init, n_init=ni, S=9, max_iters=3, epsilon=-np.inf)
    b = VO.resegment(X, phi, init, n_init=ni, S=ni, max_iters=3, epsilon=-np.inf)
    assert (a["gamma"][:, ni:] == 0).all() and (a["pi"][ni:] == 0).all()
    assert np.array_equal(a["gamma"][:, :ni], b["gamma"]) and np.array_equal(a["elbo"], b["elbo"])
    c = VO.resegment(X, phi, init, n_init=None, S=ni, max_iters=3, epsilon=-np.inf)
    assert np.array_equal(c["gamma"], b["gamma"])
    assert VO.resegment(X, phi, init, n_init=0, S=4, max_iters=1)["n_speakers"] == 1          # clamped to one live state
    assert VO.resegment(X, phi, init, n_init=99, S=4, max_iters=1)["gamma"].shape == (X.shape[0], 4)


# --------------------------------------------------------------------------------------------------------------- (d) the ELBO
@pytest.mark.parametrize("case", range(len(VO.E2E_CASES)))
def test_elbo_never_decreases_at_unit_factors(case):
    X, phi, _, init, ni = VO.e2e_case(case)
    e = VO.resegment(X, phi, init, ni, S=ni, Fa=1.0, Fb=1.0, max_iters=10, epsilon=-np.inf)["elbo"]
    assert np.isfinite(e).all()
    assert (np.diff(e) >= -1e-9 * np.abs(e[1:])).all(), np.diff(e)


# ------------------------------------------------------------------------------------------------------- (e) conventions and rules
def test_labels_rank_states_by_their_first_row_and_ties_go_to_the_lowest_state():
    g = np.array([[0.1, 0.2, 0.7], [0.5, 0.5, 0.0], [0.0, 0.3, 0.7], [0.2, 0.6, 0.2], [0.4, 0.4, 0.2]])
    states, labels, n = VO.states_to_labels(g)
    assert states.tolist() == [2, 0, 2, 1, 0] and labels.tolist() == [0, 1, 0, 2, 1] and n == 3
    assert states.dtype == np.int32 and labels.dtype == np.int32


def test_start_rows():
    g, pi = VO.start([1, -1, 5, 3, 0], S=6, Sr=4, init_smoothing=5.0)
    e = np.exp(5.0)
    assert np.allclose(g[0, :4], np.array([1, e, 1, 1]) / (e + 3), rtol=1e-15) and (g[:, 4:] == 0).all()
    for t in (1, 2):                                   # -1 and 5 lie outside [0, 4): the uniform row
        assert np.array_equal(g[t, :4], np.full(4, 0.25))
    assert np.argmax(g[3]) == 3 and np.argmax(g[4]) == 0
    assert np.abs(g.sum(axis=1) - 1).max() <= 1e-15 and np.array_equal(pi, [0.25] * 4 + [0, 0])
    g0, _ = VO.start([2, 0], S=3, Sr=3, init_smoothing=0.0)
    assert np.allclose(g0, 1.0 / 3)


def test_a_non_finite_row_poisons_its_recording_only():
    X, phi, _, init, ni = VO.e2e_case(0)
    T = X.shape[0]
    X2 = np.concatenate([X, X])
    X2[T + 3, 1] = np.inf
    r = VO.resegment_batch(X2, [T, T], phi, np.concatenate([init, init]), [ni, ni], 8, max_iters=2)
    one = VO.resegment(X, phi, init, ni, 8, max_iters=2)
    assert (r["labels"][T:] == -1).all() and (r["states"][T:] == -1).all() and r["n_speakers"][1] == -1 and r["n_iters"][1] == 0
    assert np.isnan(r["gamma"][T:]).all() and np.isnan(r["pi"][1]).all() and np.isnan(r["elbo"][1]).all()
    assert np.array_equal(r["labels"][:T], one["labels"]) and np.array_equal(r["gamma"][:T], one["gamma"]) and r["n_iters"][0] == 2
    empty = VO.resegment_batch(np.zeros((0, 4)), [0, 0], np.ones(4), np.zeros(0, dtype=np.int32), None, 3)
    assert empty["labels"].shape == (0,) and empty["n_iters"].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------- what the GPU tests rest on, on the CPU
@pytest.mark.parametrize("case", range(len(VO.E2E_CASES)))
def test_end_to_end_cases_recover_every_label_with_saturated_posteriors(case):
    X, phi, truth, init, ni = VO.e2e_case(case)
    T, q, k, _ = VO.E2E_CASES[case]
    assert X.shape == (T, q) and ni == k + 2 and len(set(init.tolist())) == k + 2          # two spurious initial clusters
    wrong = float((init != truth).mean())
    assert 0.12 <= wrong <= 0.25, wrong
    for mi in (2, 10):
        r = VO.resegment(X, phi, init, ni, S=VO.E2E_STATES, max_iters=mi, epsilon=-np.inf, trace=True)
        assert r["n_iters"] == mi and VO.same_partition(r["labels"], truth) and r["n_speakers"] == k
        for g in r["gammas"]:                                                                # after EVERY iteration
            assert float(np.minimum(g, 1 - g).max()) <= 1e-3


def test_early_stop_cases_are_clear_of_epsilon_and_stop_in_different_iterations():
    X, counts, phi, init, ni = VO.early_batch()
    free = VO.resegment_batch(X, counts, phi, init, ni, VO.E2E_STATES, max_iters=10, epsilon=-np.inf)
    for e in free["elbo"]:
        bound = 2e-4 * np.maximum(1.0, np.abs(e)).max()
        assert (np.abs(np.diff(e) - VO.EARLY_EPS) >= bound).all(), (np.diff(e), bound)
    r = VO.resegment_batch(X, counts, phi, init, ni, VO.E2E_STATES, max_iters=10, epsilon=VO.EARLY_EPS)
    assert r["n_iters"].tolist() == [3, 5, 4]
    for k, n in enumerate(r["n_iters"]):
        assert np.isfinite(r["elbo"][k, :n]).all() and np.isnan(r["elbo"][k, n:]).all()
        assert np.array_equal(r["elbo"][k, :n], free["elbo"][k, :n])


def test_residency_borders_follow_the_constants():
    from speech_signal_processing_amd import api
    assert (api.VBHMM_LDS_BYTES, api.VBHMM_ALPHA_LDS_BYTES) == (VO.LDS_BYTES, VO.ALPHA_LDS_BYTES)
    hdr = open(os.path.join(ROOT, "include", "ssp.h")).read()
    assert "#define SSP_VBHMM_LDS_BYTES %d\n" % VO.LDS_BYTES in hdr and "#define SSP_VBHMM_ALPHA_LDS_BYTES %d\n" % VO.ALPHA_LDS_BYTES in hdr
    for S, q in ((1, 1), (16, 64), (16, 256), (17, 130), (64, 130), (64, 255), (64, 256), (64, 512), (33, 1024)):
        assert api.vbhmm_n_lds(S, q) == VO.n_lds(S, q) and api.vbhmm_alpha_in_lds(S, q) == VO.alpha_in_lds(S, q)
        assert api.vbhmm_padded_states(S) == VO.padded(S)
    assert api.vbhmm_alpha_in_lds(64, 255) and not api.vbhmm_alpha_in_lds(64, 256)
    assert api.vbhmm_n_lds(16, 256) >= 800          # the 800-window design point clusters in LDS


# ----------------------------------------------------------------------------------------------------------------------- the surface
def test_header_declaration_is_bound():
    from speech_signal_processing_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "ssp.h")).read()
    m = re.search(r"\bint ssp_vbhmm_resegment\(([^;]*)\);", hdr)
    assert m, "ssp_vbhmm_resegment is not declared in include/ssp.h"
    assert len(m.group(1).split(",")) == 24
    res, args = _lib.SIGNATURES["ssp_vbhmm_resegment"]
    assert len(args) == 24 and hasattr(_lib.load(), "ssp_vbhmm_resegment")
    assert "vbhmm.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vbhmm.hip"))
    assert _lib.ABI_VERSION == 4


def test_python_surface():
    import inspect
    from speech_signal_processing_amd import api, diarize
    names = list(inspect.signature(api.vb_resegment).parameters)
    assert names[:15] == ["ctx", "X", "seg_or_counts", "phi", "init_labels", "n_init", "n_states", "loop_prob", "Fa", "Fb", "init_smoothing",
                          "max_iters", "epsilon", "want", "out"]
    d = {k: v.default for k, v in inspect.signature(api.vb_resegment).parameters.items()}
    assert (d["loop_prob"], d["Fa"], d["Fb"], d["init_smoothing"], d["max_iters"], d["epsilon"]) == (0.99, 0.3, 17.0, 5.0, 10, 1e-4)
    assert d["want"] == ("gamma", "pi", "elbo") and d["n_init"] is None and d["n_states"] is None and d["out"] is None
    v = diarize.VbHmm(np.ones(8), loop_prob=0.9, max_iters=3)
    assert v.params["loop_prob"] == 0.9 and v.params["max_iters"] == 3 and v.phi.dtype == np.float32 and callable(v.resegment)
    with pytest.raises(ValueError):
        diarize.VbHmm(np.array([1.0, -1.0]))
    plain = diarize.Diarizer("cosine", linkage="complete", threshold=0.25, min_clusters=2)
    assert plain.resegment is None and (plain.linkage, plain.threshold, plain.min_clusters) == ("complete", 0.25, 2)
    assert diarize.Diarizer("cosine", resegment=None).resegment is None
    with pytest.raises(ValueError):
        diarize.Diarizer("cosine", resegment=True)             # no phi in the cosine back end
    assert diarize.Diarizer("cosine", resegment=v).resegment is v

    class FakePlda:
        psi_ = np.arange(1.0, 5.0)

        def pairwise_coeffs(self):
            raise AssertionError("not called at construction")
    dz = diarize.Diarizer(FakePlda(), resegment=True)
    assert isinstance(dz.resegment, diarize.VbHmm) and np.array_equal(dz.resegment.phi, np.arange(1.0, 5.0, dtype=np.float32))


def test_fails_loudly_without_a_device():
    """as its neighbours: no CPU fallback"""
    import torch
    if torch.cuda.is_available():
        return
    from speech_signal_processing_amd import _lib, diarize
    X, phi, _, init, ni = VO.e2e_case(0)
    with pytest.raises(_lib.SspError):
        diarize.VbHmm(phi).resegment(X, [X.shape[0]], init, [ni])
