"""Adaptive score normalisation (AS-norm) against a cohort, for any similarity matrix: PLDA log-likelihood ratios, cosine similarities
of d-vectors.  An extension and UNPINNED: the reference has no score normalisation; Kaldi, sidekit, SpeechBrain and wespeaker ship one.
include/ssp.h (ssp_topn_stats, ssp_snorm_apply) has the definitions; tests/snorm_oracle.py restates them.

A raw score x of test vector t against enrolled speaker s becomes

    z = 1/2 ((x - mu_s) / sigma_s + (x - mu_t) / sigma_t)

mu_s, sigma_s: mean and deviation of the ``top_n`` largest scores of speaker s against the cohort (computed once, ``fit``); mu_t, sigma_t:
those of the test vector against the cohort (computed per call).  Both selections and the normalisation run on the device.

    from speech_signal_processing_amd import snorm
    norm = snorm.PldaAsNorm(model, scorer, cohort_vectors, cohort_labels, n_cohort, top_n=300)
    who = norm.score(test_vectors)["argmax"]
"""
from __future__ import annotations

import numpy as np

from . import api


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _cat(parts):
    if len(parts) == 1:
        return parts[0]
    if _is_torch(parts[0]):
        import torch
        return torch.cat(parts)
    return np.concatenate(parts)


def _check_top_n(top_n, std_floor):
    if int(top_n) != top_n or top_n < 1:
        raise ValueError("top_n must be an integer >= 1")
    if not (np.isfinite(std_floor) and std_floor > 0):
        raise ValueError("std_floor must be finite and > 0")
    return int(top_n), float(std_floor)


class AsNorm:
    """AS-norm over score matrices the caller computes.  fit(cohort_vs_enrolled): the (C, S) scores of the C cohort speakers against the
    S enrolled ones -> the enrolment-side statistics ``col_mean_`` / ``col_std_`` (S,).  normalize(scores, test_vs_cohort): (N, S) raw
    scores and the (N, C) scores of the same test vectors against the cohort -> {"argmax", "max"[, "scores"]}.  numpy in, numpy out; torch
    CUDA in, torch out."""

    def __init__(self, top_n=300, std_floor=1e-6, ctx=None):
        self.top_n, self.std_floor = _check_top_n(top_n, std_floor)
        self.ctx = ctx

    def fit(self, cohort_vs_enrolled):
        self.ctx = self.ctx or api.default_context()
        st = api.topn_stats(self.ctx, cohort_vs_enrolled, self.top_n, axis=0)
        self.col_mean_, self.col_std_ = st["mean"], st["std"]
        return self

    def _cols(self, like):
        """the enrolment-side statistics on the side ``like`` lives"""
        m, s = self.col_mean_, self.col_std_
        if _is_torch(like) and not _is_torch(m):
            import torch
            m, s = torch.from_numpy(m).to(like.device), torch.from_numpy(s).to(like.device)
            self.col_mean_, self.col_std_ = m, s
        elif not _is_torch(like) and _is_torch(m):
            m, s = m.cpu().numpy(), s.cpu().numpy()
        return m, s

    def normalize(self, scores, test_vs_cohort, out=True):
        """out: True — "scores" is a new matrix; False — the decision only; "inplace" — ``scores`` itself is overwritten and returned"""
        if not hasattr(self, "col_mean_"):
            raise ValueError("This AsNorm instance is not fitted yet")
        if int(scores.shape[0]) != int(test_vs_cohort.shape[0]):
            raise ValueError("scores and test_vs_cohort must have one row per test vector")
        st = api.topn_stats(self.ctx, test_vs_cohort, self.top_n, axis=1)
        cm, cs = self._cols(scores)
        return api.snorm_apply(self.ctx, scores, st["mean"], st["std"], cm, cs, self.std_floor, out=scores if out == "inplace" else bool(out))


class _Slabbed:
    """shared by the two back ends below: test vectors in slabs of whole rows, slab rows x (S + C) x 4 bytes under ``workspace``"""

    def _slab_rows(self):
        return max(1, int(self.workspace) // (4 * (self.S + self.C)))

    def _run(self, T, scores, pair):
        N = int(T.shape[0])
        rows = self._slab_rows()
        parts = {"argmax": [], "max": []}
        if scores:
            parts["scores"] = []
        for r0 in range(0, max(N, 1), rows):
            a, b = pair(T[r0:r0 + rows])
            res = self.norm.normalize(a, b, out="inplace" if scores else False)
            for k in parts:
                parts[k].append(res[k])
        return {k: _cat(v) for k, v in parts.items()}


class PldaAsNorm(_Slabbed):
    """AS-norm of PLDA log-likelihood ratios.  model: a fitted plda.Plda; scorer: the api.PldaScorer of the S enrolled speakers
    (model.enroll); cohort_X, cohort_labels, n_cohort: vectors of the C cohort speakers, enrolled with the same model.  The cohort
    speakers' transformed mean vectors, rounded to float32, are scored as test vectors against ``scorer`` for the enrolment side.
    score(X): projects once, scores against the enrolled and the cohort speakers, normalises; in slabs of whole rows so that the two
    score matrices of a slab stay under ``workspace`` bytes (one row always runs).  A row's result does not depend on the slab size."""

    def __init__(self, model, scorer, cohort_X, cohort_labels, n_cohort, top_n=300, std_floor=1e-6, workspace=1 << 30):
        self.model, self.scorer, self.workspace = model, scorer, int(workspace)
        model._check_fitted()
        self.ctx = model.ctx
        self.norm = AsNorm(top_n, std_floor, ctx=self.ctx)
        self.cohort_scorer = model.enroll(cohort_X, cohort_labels, int(n_cohort))
        self.S, self.C = int(scorer.S), int(n_cohort)
        lab = np.asarray(cohort_labels.cpu().numpy() if _is_torch(cohort_labels) else cohort_labels).astype(np.int32)
        T = model.project(cohort_X)
        if _is_torch(T):
            import torch
            lab = torch.as_tensor(lab, device=T.device)
        cent = api.centroids(self.ctx, T, lab, self.C)   # float32: the cohort speakers as test vectors
        self.norm.fit(scorer.score(cent, llr=True, argmax=False, maxval=False)["llr"])

    def score(self, X, scores=False):
        """-> {"argmax" (N,) int32, "max" (N,) float32[, "scores" (N, S) float32]} of the normalised ratios"""
        T = self.model.project(X)

        def pair(t):
            return (self.scorer.score(t, llr=True, argmax=False, maxval=False)["llr"],
                    self.cohort_scorer.score(t, llr=True, argmax=False, maxval=False)["llr"])
        return self._run(T, scores, pair)


class CosineAsNorm(_Slabbed):
    """AS-norm of cosine similarities, the d-vector side: similarity = 1 - the distance of api.cosine_identify(..., dist=True) (the
    subtraction is one elementwise pass in the caller's array library).  centroids (S, d): the enrolled speakers; cohort_centroids (C, d)."""

    def __init__(self, centroids, cohort_centroids, top_n=300, std_floor=1e-6, workspace=1 << 30, ctx=None):
        self.ctx = ctx or api.default_context()
        self.centroids, self.cohort, self.workspace = centroids, cohort_centroids, int(workspace)
        self.S, self.C = int(centroids.shape[0]), int(cohort_centroids.shape[0])
        self.norm = AsNorm(top_n, std_floor, ctx=self.ctx).fit(self._sim(cohort_centroids, centroids))

    def _sim(self, X, Cn):
        d = api.cosine_identify(self.ctx, X, Cn, dist=True, argmin=False, minval=False)["dist"]
        return 1.0 - d

    def score(self, X, scores=False):
        return self._run(X, scores, lambda x: (self._sim(x, self.centroids), self._sim(x, self.cohort)))
