"""A PLDA back end for fixed-length embeddings (i-vectors, d-vectors): LDA, length normalisation, two-covariance Gaussian PLDA and
log-likelihood-ratio scoring against speakers enrolled from n sessions each (Ioffe 2006; Prince & Elder 2007; Sizov, Lee & Kinnunen 2014;
the EM of Kaldi's PldaEstimator; length normalisation after Garcia-Romero & Espy-Wilson 2011).  An extension and UNPINNED: the reference
has no back end; sidekit and Kaldi ship this chain.  include/ssp.h (ssp_plda_*) has the definitions; tests/plda_oracle.py restates them in
float64.

The class statistics (api.plda_stats) and the scoring sweep (api.PldaScorer) run on the device; the EM, the diagonalisation and LDA need
only S_w, the class means and the counts and run on the host in float64, like ivector.m_step.  Centring, projection and length
normalisation are api.dense_forward and api.l2_normalize.

    from speech_signal_processing_amd import plda
    model = plda.Plda(n_iter=10, lda_dim=150).fit(train_vectors, train_labels)
    scorer = model.enroll(enrol_vectors, enrol_labels, n_speakers)
    who = model.identify(scorer, test_vectors)
"""
from __future__ import annotations

import numpy as np

from . import api

MAX_DIM = api.PLDA_MAX_Q


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _first_bad_row(X):
    """index of the first row of X with a non-finite entry, or -1"""
    if _is_torch(X):
        import torch
        ok = torch.isfinite(X).all(dim=1)
        return -1 if bool(ok.all()) else int(torch.nonzero(~ok)[0])
    ok = np.isfinite(np.asarray(X)).all(axis=1)
    return -1 if ok.all() else int(np.argmin(ok))


def class_stats(X, labels, n_classes=None, ctx=None):
    """api.plda_stats with the checks of this layer: n_classes defaults to max(labels) + 1; ValueError naming the first non-finite row.
    -> {"sum" (S, q), "count" (S,), "mean" (q,), "sw" (q, q)} on the host."""
    ctx = ctx or api.default_context()
    if n_classes is None:
        n_classes = int(labels.max()) + 1 if len(labels) else 0
    if len(labels) < 1:
        raise ValueError("at least one row is needed")
    st = api.plda_stats(ctx, X, labels, int(n_classes))
    if not (np.isfinite(st["sw"]).all() and np.isfinite(st["sum"]).all()):
        bad = _first_bad_row(X)
        raise ValueError("row %d contains NaN or infinity" % bad if bad >= 0 else "the statistics overflow")
    return st


def _fix_signs(rows):
    """the largest-magnitude entry of each row positive"""
    big = rows[np.arange(rows.shape[0]), np.abs(rows).argmax(axis=1)]
    return rows * np.where(big < 0, -1.0, 1.0)[:, None]


def _whiten(Sw, M):
    """L^-1 M L^-T and L^-1 for S_w = L L' -> (eigenvalues descending, rows = eigenvectors' L^-1: the simultaneous diagonaliser)"""
    L = np.linalg.cholesky(Sw)
    Li = np.linalg.solve(L, np.eye(L.shape[0]))
    Mw = Li @ M @ Li.T
    lam, U = np.linalg.eigh((Mw + Mw.T) * 0.5)
    order = np.argsort(-lam, kind="stable")
    return lam[order], _fix_signs(U[:, order].T @ Li)


def _nonempty(stats):
    cnt = np.asarray(stats["count"], dtype=np.int64)
    keep = cnt > 0
    if int(keep.sum()) < 2:
        raise ValueError("fewer than two classes have rows: a between-class covariance needs at least two")
    return cnt[keep], np.asarray(stats["sum"], dtype=np.float64)[keep] / cnt[keep, None]


def em(sw, class_means, counts, mean, n_iter=10):
    """The EM of the two-covariance model from W = B = I (include/ssp.h): sw (q, q) the within-class scatter, class_means (S, q) and counts
    (S,) of the classes that have rows, mean (q,) of all rows.  -> (W, B, objective (n_iter,)); objective[it] belongs to the (W, B) that
    iteration ``it`` started from and never decreases."""
    sw = np.asarray(sw, dtype=np.float64)
    m = np.asarray(class_means, dtype=np.float64) - np.asarray(mean, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    q, S, N = sw.shape[0], m.shape[0], int(counts.sum())
    groups = [(int(c), int((counts == c).sum()), m[counts == c].T @ m[counts == c]) for c in np.unique(counts)]
    W, B, I = np.eye(q), np.eye(q), np.eye(q)
    obj = []
    for _ in range(int(n_iter)):
        Wi, Bi = np.linalg.inv(W), np.linalg.inv(B)
        ldW = np.linalg.slogdet(W)[1]
        o = -0.5 * np.trace(Wi @ sw)
        Bn, Wn = np.zeros((q, q)), sw.copy()
        for c, k, F in groups:
            T = B + W / c
            o -= 0.5 * (k * ((c - 1) * ldW + np.linalg.slogdet(T)[1]) + np.trace(np.linalg.solve(T, F)))
            V = np.linalg.inv(Bi + c * Wi)
            G = c * V @ Wi
            H = I - G
            Bn += k * V + G @ F @ G.T
            Wn += c * (k * V + H @ F @ H.T)
        obj.append(o)
        B, W = (Bn + Bn.T) / (2.0 * S), (Wn + Wn.T) / (2.0 * N)
    return W, B, np.asarray(obj, dtype=np.float64)


def diagonalise(W, B):
    """-> (A, psi): A W A' = I, A B A' = diag(psi), psi descending, the largest-magnitude entry of each row of A positive"""
    psi, A = _whiten(np.asarray(W, dtype=np.float64), np.asarray(B, dtype=np.float64))
    return A, np.maximum(psi, 0.0)


def pairwise_coeffs(psi):
    """Plda.pairwise_coeffs for a given psi (q,) >= 0"""
    psi = np.asarray(psi, dtype=np.float64)
    if psi.ndim != 1 or not np.isfinite(psi).all() or (psi < 0).any():
        raise ValueError("psi must be a finite vector >= 0")
    g = psi / (2.0 * psi + 1.0)
    h = 0.5 * psi * psi / ((psi + 1.0) * (2.0 * psi + 1.0))
    c0 = -0.5 * float(np.sum(np.log(2.0 * psi + 1.0) - 2.0 * np.log1p(psi)))
    return g.astype(np.float32), h.astype(np.float32), float(np.float32(c0))


class Lda:
    """Linear discriminant analysis from the device's class statistics: the top ``n_components`` generalised eigenvectors of
    S_b v = lambda S_w v, v' S_w v = 1.  ``mean_`` (q,), ``components_`` (q, p) and ``eigenvalues_`` (p,) are set by fit."""

    def __init__(self, n_components, ctx=None):
        if int(n_components) != n_components or n_components < 1:
            raise ValueError("n_components must be an integer >= 1")
        self.n_components = int(n_components)
        self.ctx = ctx

    def fit(self, X, labels, stats=None):
        self.ctx = self.ctx or api.default_context()
        st = stats or class_stats(X, labels, ctx=self.ctx)
        return self._fit_stats(st)

    def _fit_stats(self, st):
        cnt, means = _nonempty(st)
        q, N, S = st["sw"].shape[0], int(cnt.sum()), int(cnt.size)
        if self.n_components > min(q, S - 1):
            raise ValueError("n_components=%d exceeds min(q, classes - 1) = %d" % (self.n_components, min(q, S - 1)))
        if N - S < q:
            raise ValueError("N - S = %d < q = %d: the within-class scatter is singular" % (N - S, q))
        m = means - st["mean"]
        Sb = (m * cnt[:, None]).T @ m
        lam, V = _whiten(st["sw"], Sb)
        self.mean_ = np.asarray(st["mean"], dtype=np.float64)
        self.components_ = np.ascontiguousarray(V[:self.n_components].T)
        self.eigenvalues_ = lam[:self.n_components]
        return self

    def transform(self, X):
        """(X - mean) @ components, float32, on the device (api.dense_forward); numpy in, numpy out; torch in, torch out"""
        if not hasattr(self, "components_"):
            raise ValueError("This Lda instance is not fitted yet")
        self.ctx = self.ctx or api.default_context()
        return _affine(self.ctx, X, self.components_.T, -(self.components_.T @ self.mean_))


def _affine(ctx, X, Wt, bias):
    """X @ Wt.T + bias through ssp_dense_forward, on the side X lives"""
    Wt = np.ascontiguousarray(Wt, dtype=np.float32)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    if _is_torch(X):
        import torch
        return api.dense_forward(ctx, X, torch.from_numpy(Wt).to(X.device), torch.from_numpy(bias).to(X.device))
    return api.dense_forward(ctx, np.ascontiguousarray(X, dtype=np.float32), Wt, bias)


class Plda:
    """Two-covariance Gaussian PLDA with optional LDA and length normalisation in front.

    fit(X, labels): class statistics on the device, LDA (lda_dim) from them, the vectors centred, projected and length-normalised on the
    device, statistics of the projected vectors, then ``n_iter`` EM iterations and the diagonalisation on the host.  Sets ``mean_`` (q,),
    ``lda_`` ((q, p) or None), ``plda_mean_`` (p,: the mean of the projected training vectors), ``within_`` / ``between_`` (p, p),
    ``transform_`` (A, (p, p)), ``psi_`` (p,) and ``objective_`` (n_iter,).
    project(X): centre -> LDA -> length-norm -> A (x' - plda_mean_), float32.  enroll / score / identify: api.PldaScorer."""

    def __init__(self, n_iter=10, lda_dim=None, length_norm=True, ctx=None):
        if int(n_iter) != n_iter or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        if lda_dim is not None and (int(lda_dim) != lda_dim or lda_dim < 1):
            raise ValueError("lda_dim must be None or an integer >= 1")
        self.n_iter, self.lda_dim, self.length_norm = int(n_iter), None if lda_dim is None else int(lda_dim), bool(length_norm)
        self.ctx = ctx

    # ---- the front end: everything before A
    def _front(self, X):
        if self.lda_ is None and not self.length_norm:
            return X
        q = self.mean_.shape[0]
        P = np.eye(q) if self.lda_ is None else self.lda_.T
        Y = _affine(self.ctx, X, P, -(P @ self.mean_))
        return api.l2_normalize(self.ctx, Y) if self.length_norm else Y

    def _check_fitted(self):
        if not hasattr(self, "transform_"):
            raise ValueError("This Plda instance is not fitted yet")
        self.ctx = self.ctx or api.default_context()

    def fit(self, X, labels):
        self.ctx = self.ctx or api.default_context()
        if getattr(X, "ndim", 0) != 2:
            raise ValueError("X must be (N, q)")
        if int(X.shape[1]) > MAX_DIM:
            raise NotImplementedError("q=%d exceeds the supported dimension (%d)" % (int(X.shape[1]), MAX_DIM))
        st = class_stats(X, labels, ctx=self.ctx)
        n_classes = int(st["count"].shape[0])
        _nonempty(st)
        self.mean_ = st["mean"]
        self.lda_ = None
        if self.lda_dim is not None:
            self.lda_ = Lda(self.lda_dim, ctx=self.ctx)._fit_stats(st).components_
        if self.lda_ is not None or self.length_norm:
            st = class_stats(self._front(X), labels, n_classes=n_classes, ctx=self.ctx)
        self._fit_stats(st)
        return self

    def _fit_stats(self, st):
        """the host half of fit: EM and diagonalisation from the statistics of the projected vectors"""
        cnt, means = _nonempty(st)
        p, N, S = st["sw"].shape[0], int(cnt.sum()), int(cnt.size)
        if N - S < p:
            raise ValueError("N - S = %d < q = %d after projection: the within-class covariance W is singular "
                             "(more rows, fewer classes or a smaller lda_dim)" % (N - S, p))
        self.plda_mean_ = np.asarray(st["mean"], dtype=np.float64)
        self.within_, self.between_, self.objective_ = em(st["sw"], means, cnt, self.plda_mean_, self.n_iter)
        self.transform_, self.psi_ = diagonalise(self.within_, self.between_)
        return self

    def project(self, X):
        self._check_fitted()
        return _affine(self.ctx, self._front(X), self.transform_, -(self.transform_ @ self.plda_mean_))

    def pairwise_coeffs(self):
        """-> (g, h, c0) of api.pairwise_scores for the log-likelihood ratio of two PROJECTED vectors, one of them the single enrolment
        vector of a speaker (symmetric in the two):  LLR = sum_d g_d x_d y_d - sum_d h_d (x_d^2 + y_d^2) + c0 with
        g = psi / (2 psi + 1), h = psi^2 / (2 (psi + 1)(2 psi + 1)), c0 = -1/2 sum_d log((2 psi_d + 1) / (psi_d + 1)^2); formed in
        float64 and rounded once: g, h float32 (q,), c0 a float"""
        self._check_fitted()
        return pairwise_coeffs(self.psi_)

    def enroll(self, X, labels, n_speakers, flags=0):
        """-> api.PldaScorer of ``n_speakers`` speakers: the means of their projected vectors (ssp_centroids) and their counts"""
        self._check_fitted()
        lab = np.asarray(labels.cpu().numpy() if _is_torch(labels) else labels).astype(np.int64)
        if lab.ndim != 1 or lab.shape[0] != int(X.shape[0]):
            raise ValueError("one label per row of X")
        if lab.size and (lab.min() < 0 or lab.max() >= int(n_speakers)):
            raise ValueError("a label outside [0, %d)" % int(n_speakers))
        counts = np.bincount(lab, minlength=int(n_speakers))
        if (counts < 1).any():
            raise ValueError("speaker %d has no enrolment vector" % int(np.argmin(counts)))
        bad = _first_bad_row(X)
        if bad >= 0:
            raise ValueError("row %d contains NaN or infinity" % bad)
        T = self.project(X)
        if _is_torch(T):
            import torch
            dev_lab = labels if _is_torch(labels) else torch.as_tensor(lab.astype(np.int32), device=T.device)
            cent = api.centroids(self.ctx, T, dev_lab, int(n_speakers))
        else:
            cent = api.centroids(self.ctx, T, lab.astype(np.int32), int(n_speakers))
        cent = cent.cpu().numpy() if _is_torch(cent) else cent
        return api.PldaScorer(self.ctx, self.psi_, cent.astype(np.float64), counts, flags=flags)

    def score(self, scorer, X, llr=False):
        """-> api.PldaScorer.score of the projected vectors: {"argmax", "max"[, "llr"]}"""
        return scorer.score(self.project(X), llr=llr)

    def identify(self, scorer, X):
        """the enrolled speaker with the largest log-likelihood ratio for every row of X (N,) int32"""
        return self.score(scorer, X)["argmax"]

    def save(self, path):
        self._check_fitted()
        np.savez(path, mean=self.mean_, lda=np.zeros((0, 0)) if self.lda_ is None else self.lda_, plda_mean=self.plda_mean_, within=self.within_,
                 between=self.between_, transform=self.transform_, psi=self.psi_, objective=self.objective_,
                 params=np.array([self.n_iter, -1 if self.lda_dim is None else self.lda_dim, int(self.length_norm)], dtype=np.int64))

    @classmethod
    def load(cls, path, ctx=None):
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz") as z:
            n_iter, lda_dim, ln = (int(v) for v in z["params"])
            m = cls(n_iter=n_iter, lda_dim=None if lda_dim < 0 else lda_dim, length_norm=bool(ln), ctx=ctx)
            m.mean_, m.plda_mean_, m.within_, m.between_ = z["mean"], z["plda_mean"], z["within"], z["between"]
            m.transform_, m.psi_, m.objective_ = z["transform"], z["psi"], z["objective"]
            m.lda_ = z["lda"] if z["lda"].size else None
        return m
