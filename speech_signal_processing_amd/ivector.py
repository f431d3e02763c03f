"""i-vectors on the GPU: Baum-Welch statistics under a GMM-UBM go in, a fixed-length embedding comes out (Dehak et al. 2011, after
Kenny 2005) — the bridge between the package's GMM-UBM half and its cosine scorer.  An extension and UNPINNED: the reference has no factor
analysis; sidekit, the package it imports its features from, ships this model as FactorAnalyser.total_variability / extract_ivectors.
include/ssp.h (ssp_ivector_*) has the definitions; tests/ivector_oracle.py restates them in float64.

The two halves joined — enrol on i-vectors with the centroid kernel, identify with the cosine scorer:

    from speech_signal_processing_amd import api, d_vector, ivector
    tv = ivector.TotalVariability(rank=64, n_iter=10).fit(ubm, train_feats)          # train_feats: a list of (T_j, D) matrices
    E = tv.transform(enrol_feats, normalize=True)                                    # (U, 64) float32
    cent = api.centroids(api.default_context(), E, enrol_labels, n_speakers)         # ssp_centroids
    who = d_vector.identify(tv.transform(test_feats, normalize=True), cent)          # ssp_cosine_identify

Raw cosine is the weakest way to score i-vectors; the usual chain ends in a PLDA back end (plda.py: LDA, length normalisation, PLDA):

    from speech_signal_processing_amd import plda
    back = plda.Plda(n_iter=10, lda_dim=48).fit(tv.transform(train_feats), train_labels)       # ssp_plda_stats + host EM
    scorer = back.enroll(tv.transform(enrol_feats), enrol_labels, n_speakers)                   # ssp_centroids, ssp_plda_pack
    who = back.identify(scorer, tv.transform(test_feats))                                       # ssp_plda_score
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import api, gmm_train

MAX_RANK = api.IVECTOR_MAX_R


def baum_welch_stats(ubm, Xs, ctx=None):
    """Zeroth- and first-order statistics of every array of ``Xs`` under the fitted diagonal ``ubm``, in ONE ssp_gmm_em_stats_shared call
    -> (nk (U, K), sx (U, K, D)) float64.  ValueError as gmm_train.map_adapt raises it: a non-finite row (the message names the
    utterance and row), mismatched feature widths, an empty array, an unfitted ubm."""
    gmm_train._check_fitted_ubm(ubm)
    w, mu, cv = gmm_train._diag_ubm_arrays(ubm)
    Xs = list(Xs)
    if not Xs:
        return np.empty((0, mu.shape[0])), np.empty((0,) + mu.shape)
    _, _, st = gmm_train._shared_stats(w, mu, cv, Xs, ctx or getattr(ubm, "_ctx", None))
    return st["nk"], st["sx"]


def m_step(A, C):
    """T_k = C_k A_k^-1 in float64, a Cholesky solve per mixture.  A (K, R, R) symmetric, C (K, D, R) -> T (K, D, R).  A mixture no
    utterance reached (A_k = 0) keeps a zero block."""
    T = np.zeros_like(C)
    for k in range(A.shape[0]):
        if not A[k].any():
            continue
        Lk = np.linalg.cholesky(A[k])
        T[k] = np.linalg.solve(Lk.T, np.linalg.solve(Lk, C[k].T)).T
    return T


class TotalVariability:
    """The total-variability (i-vector) model over a fitted diagonal GMM-UBM.

    fit: EM on T from T0 = init_scale * default_rng(seed).standard_normal((K, D, R)); the E-step runs on the device
    (api.IvectorExtractor.estep), the M-step on the host in float64.  No covariance update and no minimum-divergence step.
    ``T_`` (K, D, R) and ``objective_`` (one value per iteration: the objective of the T that iteration started from) are set.
    transform: the i-vectors (U, R) float32 of utterances given as feature matrices (``Xs``) or as statistics (``stats = (nk, sx)``)."""

    def __init__(self, rank, n_iter=10, seed=0, init_scale=0.1, workspace_bytes=None, ctx=None):
        if int(rank) != rank or rank < 1:
            raise ValueError("rank must be an integer >= 1")
        if rank > MAX_RANK:
            raise NotImplementedError("rank=%d exceeds the supported rank (%d)" % (rank, MAX_RANK))
        if int(n_iter) != n_iter or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        self.rank, self.n_iter, self.seed, self.init_scale = int(rank), int(n_iter), seed, float(init_scale)
        self.workspace_bytes = workspace_bytes
        self.ctx = ctx
        self._ext = None

    def _stats(self, Xs, stats):
        if (Xs is None) == (stats is None):
            raise ValueError("give exactly one of Xs (feature matrices) and stats (nk, sx)")
        if stats is not None:
            nk, sx = stats
            return np.asarray(nk, dtype=np.float64), np.asarray(sx, dtype=np.float64)
        ubm = SimpleNamespace(weights_=self.ubm_weights_, means_=self.ubm_means_, covariances_=self.ubm_covariances_)
        return baum_welch_stats(ubm, Xs, ctx=self.ctx)

    def _extractor(self):
        if not hasattr(self, "T_"):
            raise ValueError("This TotalVariability instance is not fitted yet")
        if self._ext is None:
            self.ctx = self.ctx or api.default_context()
            self._ext = api.IvectorExtractor(self.ctx, self.ubm_means_, self.ubm_covariances_, self.T_)
            if self.workspace_bytes is not None:
                self._ext.set_workspace(self.workspace_bytes)
        return self._ext

    def _set_ubm(self, ubm):
        gmm_train._check_fitted_ubm(ubm)
        w, mu, cv = gmm_train._diag_ubm_arrays(ubm)
        self.ubm_weights_, self.ubm_means_, self.ubm_covariances_ = w, mu, cv
        self._ext = None

    def fit(self, ubm, Xs=None, stats=None):
        self._set_ubm(ubm)
        nk, sx = self._stats(Xs, stats)
        K, D = self.ubm_means_.shape
        if nk.ndim != 2 or nk.shape[1] != K or sx.shape != (nk.shape[0], K, D) or nk.shape[0] < 1:
            raise ValueError("expected statistics nk (U >= 1, %d) and sx (U, %d, %d)" % (K, K, D))
        self.T_ = self.init_scale * np.random.default_rng(self.seed).standard_normal((K, D, self.rank))
        self.objective_ = []
        ext = self._extractor()
        for _ in range(self.n_iter):
            r = ext.estep(nk, sx)
            self.objective_.append(r["objective"])
            self.T_ = m_step(r["A"], r["C"])
            ext.set_T(self.T_)
        self.objective_ = np.asarray(self.objective_, dtype=np.float64)
        return self

    def transform(self, Xs=None, stats=None, normalize=False):
        ext = self._extractor()
        nk, sx = self._stats(Xs, stats)
        w = ext.extract(nk, sx)
        return np.asarray(api.l2_normalize(self.ctx, w)) if normalize else w

    def save(self, path):
        if not hasattr(self, "T_"):
            raise ValueError("This TotalVariability instance is not fitted yet")
        np.savez(path, T=self.T_, objective=self.objective_, ubm_weights=self.ubm_weights_, ubm_means=self.ubm_means_,
                 ubm_covariances=self.ubm_covariances_, params=np.array([self.rank, self.n_iter, self.seed], dtype=np.int64),
                 init_scale=np.float64(self.init_scale))

    @classmethod
    def load(cls, path, workspace_bytes=None, ctx=None):
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz") as z:
            rank, n_iter, seed = (int(v) for v in z["params"])
            tv = cls(rank, n_iter=n_iter, seed=seed, init_scale=float(z["init_scale"]), workspace_bytes=workspace_bytes, ctx=ctx)
            tv.T_, tv.objective_ = z["T"], z["objective"]
            tv.ubm_weights_, tv.ubm_means_, tv.ubm_covariances_ = z["ubm_weights"], z["ubm_means"], z["ubm_covariances"]
        return tv
