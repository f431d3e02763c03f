"""Golden vectors for full-covariance GMMs: sklearn.mixture.GaussianMixture(covariance_type='full') and nothing else.

    python tests/golden/make_golden_gmm_full.py        (needs scikit-learn; writes tests/golden/gmm_full.npz)

Fit cases (tests/gmm_full_cases.py, FIT_CASES: K = 5, D = 13, n = 3000 and K = 3, D = 39, n = 6000): the frames and the given
weights_init / means_init / precisions_init are drawn from the case's seed, the golden keeps a checksum and the first rows of X and
sklearn's fitted weights_, means_, covariances_, precisions_cholesky_, lower_bound_ and n_iter_ for tol = 0, max_iter in {1, 5} and for
tol = 1e-3.  d_emu: the deviation from sklearn, per parameter block, of the same loop run with the float32 yardstick statistics
(gmm_full_cases.emu32) in place of the kernel — what float32 statistics cost; the GPU fit is held to 8 d_emu + 1e-6 (|value| + 1).
score_samples: two fitted models (max_iter = 5) on a held-out matrix.
E-step / M-step vectors of a small case (K = 4, D = 6, n = 200) for the host file: _estimate_log_prob_resp, _estimate_gaussian_parameters,
_compute_precision_cholesky.
The end-to-end set of tests/test_gmm_full_gpu.py (three speakers that differ in covariance orientation only) is drawn there from a
seed; here sklearn's own accuracies on it are recorded: full models must reach >= 0.95, diag models <= 0.5.
"""
import os
import sys
import warnings

import numpy as np
from sklearn.mixture import GaussianMixture
from sklearn.mixture import _gaussian_mixture as G

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gmm_full_cases as FC  # noqa: E402


def fit(X, w0, mu0, P0, tol, max_iter):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return GaussianMixture(n_components=len(w0), covariance_type="full", tol=tol, max_iter=max_iter, reg_covar=1e-6, weights_init=w0,
                               means_init=mu0, precisions_init=P0).fit(X.astype(np.float64))


def put(out, prefix, g, params=True):
    if params:   # (the symmetric covariances and the triangular factors as their upper triangles: gmm_full_cases.golden_fit unpacks)
        iu = np.triu_indices(g.means_.shape[1])
        out[prefix + "_weights"] = g.weights_
        out[prefix + "_means"] = g.means_
        out[prefix + "_covariances_triu"] = g.covariances_[:, iu[0], iu[1]]
        out[prefix + "_precisions_cholesky_triu"] = g.precisions_cholesky_[:, iu[0], iu[1]]
    out[prefix + "_lower_bound"] = np.float64(g.lower_bound_)
    out[prefix + "_n_iter"] = np.int64(g.n_iter_)


def main():
    out = {}
    fitted = {}
    for name in FC.FIT_CASES:
        X, w0, mu0, P0 = FC.fit_data(name)
        out[name + "_x_sum"] = np.float64(X.astype(np.float64).sum())
        out[name + "_x_head"] = X[:4].copy()
        for it in (1, 5):
            g = fit(X, w0, mu0, P0, 0.0, it)
            put(out, "%s_it%d" % (name, it), g)
            fitted[(name, it)] = g
            e = FC.emu_fit(X, w0, mu0, P0, it)
            dev = FC.fit_deviation(e, FC.golden_fit(out, "%s_it%d" % (name, it)))
            out["%s_it%d_d_emu" % (name, it)] = np.array([dev[b] for b in FC.FIT_BLOCKS])
            out["%s_it%d_d_emu_lower" % (name, it)] = np.float64(abs(e["lower_bound"] - g.lower_bound_))
        put(out, name + "_tol", fit(X, w0, mu0, P0, 1e-3, 100), params=False)
    # score_samples of two fitted models on held-out frames
    for name in FC.FIT_CASES:
        K, D, n, seed = FC.FIT_CASES[name]
        rng = np.random.default_rng(seed + 1000)
        g = fitted[(name, 5)]
        Y = (g.means_[rng.integers(0, K, 96)] + rng.standard_normal((96, D))).astype(np.float32)
        out[name + "_held"] = Y
        out[name + "_score_samples"] = g.score_samples(Y.astype(np.float64))
    # E / M step vectors for the host file
    rng = np.random.default_rng(77)
    w, mu, cov, U = FC.draw_model(rng, 4, 6)
    X = FC.draw_frames(rng, w, mu, cov, 200).astype(np.float64)
    g = GaussianMixture(n_components=4, covariance_type="full")
    g.weights_, g.means_, g.covariances_, g.precisions_cholesky_ = w, mu, cov, G._compute_precision_cholesky(cov, "full")
    log_prob_norm, log_resp = g._estimate_log_prob_resp(X)
    nk, means, covs = G._estimate_gaussian_parameters(X, np.exp(log_resp), 1e-6, "full")
    out.update(step_w=w, step_mu=mu, step_cov=cov, step_X=X.astype(np.float32), step_U=g.precisions_cholesky_, step_lse=log_prob_norm,
               step_log_resp=log_resp, step_nk=nk, step_means=means, step_covs=covs,
               step_U_new=G._compute_precision_cholesky(covs, "full"))
    # the end-to-end set: sklearn alone must satisfy the test's condition
    train, x_test, y_test = FC.orientation_set()
    acc = {}
    for kind in ("full", "diag"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm = [GaussianMixture(4, covariance_type=kind, random_state=0).fit(train[s].astype(np.float64)) for s in sorted(train)]
        pred = np.array([[m.score(x.astype(np.float64)) for m in gm] for x in x_test]).argmax(axis=1)
        acc[kind] = float((pred == np.array(y_test)).mean())
    print("orientation set: sklearn full %.3f, diag %.3f" % (acc["full"], acc["diag"]))
    assert acc["full"] >= 0.95 and acc["diag"] <= 0.5, acc
    out["orient_acc_full"], out["orient_acc_diag"] = np.float64(acc["full"]), np.float64(acc["diag"])
    np.savez_compressed(FC.GOLDEN, **out)
    print("wrote", FC.GOLDEN, os.path.getsize(FC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
