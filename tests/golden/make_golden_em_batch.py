"""Golden vectors for training many speaker GMMs at once (gmm_train.fit_many, ssp_gmm_em_stats_batch): one
sklearn.mixture.GaussianMixture(covariance_type='diag').fit per speaker — the loop the reference trains its speaker models
with (GMM_UBM.py:154-170) — each from explicit initial parameters, so that the EM iterates are deterministic.  The initial
parameters are float32 values (stored as such; every fit reads them as float64).  Run in the build container:

    python tests/golden/make_golden_em_batch.py        ->  tests/golden/gmm_em_batch.npz

Case a: 6 speakers, K = 16, D = 26 (the reference's default shape), ragged frame counts, tol = 1e-3, max_iter = 100 (the
speakers stop after different iteration counts).  Case b: 3 speakers, K = 128, D = 39, max_iter = 3, tol = 0.
"""
import os
import warnings

import numpy as np
from sklearn.mixture import GaussianMixture

HERE = os.path.dirname(os.path.abspath(__file__))
# (tag, K, D, frames per speaker, max_iter, tol, balanced): case b puts every ~8-frame cluster of the data under one component that
# starts at it (balanced labels, means within 0.1 of the centres), so that the fit is well conditioned — no component competes for a
# frame or two, where fp32 statistics no longer resolve its covariance
CASES = [("a", 16, 26, [300, 2500, 700, 1500, 1000, 450], 100, 1e-3, False), ("b", 128, 39, [1000, 900, 1100], 3, 0.0, True)]


def main():
    out = {}
    for tag, K, D, lens, max_iter, tol, balanced in CASES:
        rng = np.random.default_rng(ord(tag) + 101)
        for s, n in enumerate(lens):
            centres = 2.0 * rng.standard_normal((K, D))
            lab = rng.permutation(np.arange(n) % K) if balanced else rng.integers(0, K, n)
            X = centres[lab] + rng.uniform(0.5, 1.5, (K, D))[lab] * rng.standard_normal((n, D))
            X = (np.round(X * 64) / 64).astype(np.float32)  # (multiples of 1/64: the file compresses)
            w0 = rng.dirichlet(5 * np.ones(K)).astype(np.float32)
            w0 = (w0 / w0.sum(dtype=np.float64)).astype(np.float64)
            mu0 = (centres + (0.1 if balanced else rng.uniform(0.2, 2.5)) * rng.standard_normal((K, D))).astype(np.float32)
            cov0 = rng.uniform(0.8, 2.0, (K, D)).astype(np.float32)
            g = GaussianMixture(n_components=K, covariance_type="diag", tol=tol, max_iter=max_iter, reg_covar=1e-6,
                                weights_init=w0, means_init=mu0.astype(np.float64), precisions_init=1.0 / cov0.astype(np.float64))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # ConvergenceWarning of the fixed-iteration case
                g.fit(X.astype(np.float64))
            p = "%s%d_" % (tag, s)
            out.update({p + "X": X, p + "w0": w0, p + "mu0": mu0, p + "cov0": cov0, p + "w": g.weights_, p + "mu": g.means_,
                        p + "cov": g.covariances_, p + "lb": np.array(g.lower_bound_), p + "niter": np.array(g.n_iter_),
                        p + "conv": np.array(g.converged_)})
        out[tag + "_cfg"] = np.array([K, D, len(lens), max_iter, tol])
    np.savez_compressed(os.path.join(HERE, "gmm_em_batch.npz"), **out)
    print("wrote gmm_em_batch.npz", {c[0]: [int(out["%s%d_niter" % (c[0], s)]) for s in range(len(c[3]))] for c in CASES})


if __name__ == "__main__":
    main()
