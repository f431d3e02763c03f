"""GPU-backed EM training of diagonal GMMs with the call surface of the class the reference trains with:
``sklearn.mixture.GaussianMixture(n_components, covariance_type='diag')`` (GMM_UBM.py:158-170).

The O(frames x K x D) work of every EM iteration — E step and the resp.T @ X / resp.T @ X^2 sums — runs in HIP kernels
(``ssp_gmm_em_stats``); the O(K x D) closing arithmetic of the M step and the convergence test are the float64 lines of
sklearn's ``_m_step`` / ``fit_predict`` restated here on the host.  Trained objects duck-type a fitted sklearn model
(``weights_``, ``means_``, ``covariances_``, ``precisions_cholesky_``, ``converged_``, ``n_iter_``, ``lower_bound_``),
so ``GMM_UBM.score_matrix`` / ``api.GmmScorer.from_sklearn`` take them as they take sklearn's.

Initialisation.  With ``weights_init`` / ``means_init`` / ``precisions_init`` given, the start is exactly sklearn's and
so is every iterate (parity tests).  Otherwise ``init_params='kmeans'`` (sklearn's default too): k-means++ seeding on a
subsample (sequential sampling; on the host as sklearn does it, or with ``seeding='device'`` the same draws and the same picks through
``ssp_kmeanspp_seed`` on the GPU), Lloyd iterations on the GPU — the E/M statistics
kernels at a small shared spherical variance are the hard-assignment limit of the same sums — and the component weights,
means and variances of the resulting clusters as the start, like sklearn's ``_initialize_parameters``.  The random streams
differ from sklearn's, so trained models agree in quality, not bit for bit.  ``init_params='random_from_data'``: K distinct
frames as means, the global variance as every covariance, uniform weights.

``covariance_type='full'`` (sklearn's default) has the same surface: the O(frames x K x D^2) statistics come from
``ssp_gmm_full_em_stats`` about the global mean (no need to centre the features first), the M step is sklearn's
``_estimate_gaussian_covariances_full`` from those raw moments and ``_compute_precision_cholesky`` in float64 (``_m_step_full``), the
start is sklearn's ``_initialize`` for given ``*_init`` and otherwise the stage above with the clusters' full covariances; fitted
``covariances_`` / ``precisions_cholesky_`` / ``precisions_`` are (K, D, D), and scoring goes through ``api.GmmFullScorer``.
``'tied'`` and ``'spherical'`` are refused.
"""
from __future__ import annotations

import numpy as np

from . import api


def _nonfinite_message(what, row=None):
    """sklearn's input validation in this layer's words: the model / utterance and the first offending row are named"""
    at = "" if row is None else " (first at row %d)" % row
    return "Input X%s contains NaN, infinity or a value too large for float32%s." % (what, at)


def _first_bad_row(X):
    """index of the first row of the device matrix X with a non-finite entry, or None: ONE reduction over what already sits on the device
    (the row index is only looked up when the answer is yes)"""
    import torch
    if bool(torch.isfinite(X).all()):
        return None
    return int(torch.nonzero(~torch.isfinite(X).all(dim=1))[0, 0])


def _kmeanspp_draws(rng, n, K):
    """Every random draw of one k-means++ seeding of n rows, in the order GaussianMixture._kmeanspp has always drawn them: the sorted
    subsample of min(n, max(20000, 50 K)) rows (rng.choice), the position of the first centre in it (rng.randint), and the K - 1 rows of
    2 + int(ln K) uniforms (rng.uniform) -> (idx int64, first, u (K - 1, L)).  Both seedings draw through this, so they consume a
    RandomState identically."""
    idx = np.sort(rng.choice(n, size=min(n, max(20000, 50 * K)), replace=False))
    first = int(rng.randint(len(idx)))
    L = 2 + int(np.log(K))
    u = np.empty((K - 1, L))
    for k in range(1, K):
        u[k - 1] = rng.uniform(size=L)
    return idx, first, u


_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
                "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.")


def _lower_inverse_t(L):
    """solve_triangular(L, I, lower=True).T by forward substitution, float64"""
    D = L.shape[0]
    inv = np.zeros((D, D))
    for i in range(D):
        row = -L[i, :i] @ inv[:i]
        row[i] += 1.0
        inv[i] = row / L[i, i]
    return inv.T


def precision_cholesky_full(covariances):
    """sklearn's _compute_precision_cholesky for covariance_type='full': U_k = solve_triangular(cholesky(Sigma_k, lower=True), I,
    lower=True).T, upper triangular, (K, D, D) float64; its ValueError when a covariance has no Cholesky factor."""
    covariances = np.asarray(covariances, dtype=np.float64)
    out = np.empty_like(covariances)
    for k, cov in enumerate(covariances):
        try:
            if not np.isfinite(cov).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(cov)
        except np.linalg.LinAlgError:
            raise ValueError(_ILL_DEFINED) from None
        out[k] = _lower_inverse_t(L)
    return out


def precision_cholesky_from_precisions_full(precisions):
    """sklearn's _compute_precision_cholesky_from_precisions for 'full': the upper-triangular U with U U^T = precision, J L J of the
    Cholesky factor L of the row- and column-reversed matrix"""
    precisions = np.asarray(precisions, dtype=np.float64)
    return np.stack([np.linalg.cholesky(p[::-1, ::-1])[::-1, ::-1] for p in precisions])


class GaussianMixture:
    def __init__(self, n_components=1, covariance_type='diag', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 weights_init=None, means_init=None, precisions_init=None, random_state=None, init_params='kmeans', ctx=None,
                 seeding='host'):
        if covariance_type not in ('diag', 'full'):
            raise ValueError("only covariance_type='diag' (what GMM_UBM.py:158,169 uses) and 'full' (sklearn's default) are supported")
        if n_components < 1 or max_iter < 1 or n_init < 1 or tol < 0 or reg_covar < 0:
            raise ValueError("invalid GaussianMixture parameter")
        self.n_components = int(n_components)
        self.covariance_type = covariance_type
        self.tol, self.reg_covar, self.max_iter, self.n_init = float(tol), float(reg_covar), int(max_iter), int(n_init)
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.random_state = random_state
        if init_params not in ('kmeans', 'random_from_data'):
            raise ValueError("init_params must be 'kmeans' or 'random_from_data'")
        self.init_params = init_params
        if seeding not in ('host', 'device'):
            raise ValueError("seeding must be 'host' or 'device'")
        self.seeding = seeding
        self._ctx = ctx

    def __getstate__(self):  # picklable like the sklearn object it stands in for (GMM_UBM.py:173-179): no device handles
        st = dict(self.__dict__)
        st["_ctx"] = None
        return st

    # ---- sklearn's M step (mixture/_gaussian_mixture.py:_estimate_gaussian_parameters, _m_step), float64
    def _m_step(self, st, n):
        nk = st["nk"] + 10 * np.finfo(np.float64).eps
        means = st["sx"] / nk[:, None]
        avg_X2 = st["sxx"] / nk[:, None]
        covars = avg_X2 - 2 * (means * st["sx"] / nk[:, None]) + means ** 2 + self.reg_covar
        weights = nk / n
        return weights / weights.sum(), means, covars

    def _rows(self, X, idx):
        return np.asarray(X[idx].cpu() if api._is_torch(X) else X[idx], dtype=np.float64)

    def _kmeanspp(self, X, n, D, rng):
        """k-means++ seeds on <= 20000 sampled frames (host; the only random draws of the k-means start)"""
        K = self.n_components
        idx, first, u = _kmeanspp_draws(rng, n, K)
        sub = self._rows(X, idx)
        centres = np.empty((K, D))
        centres[0] = sub[first]
        d2 = ((sub - centres[0]) ** 2).sum(1)
        sq = (sub * sub).sum(1)
        for k in range(1, K):  # D^2 sampling, best of 2 + log K candidates (sklearn's kmeans_plusplus)
            cand = np.searchsorted(np.cumsum(d2), u[k - 1] * d2.sum())
            cand = np.clip(cand, 0, len(sub) - 1)
            # |s - c|^2 = |s|^2 + |c|^2 - 2 s.c as one small matrix product (the broadcast difference cost 0.5 s at K = 64)
            dc = np.maximum(sq[:, None] + sq[cand][None, :] - 2.0 * (sub @ sub[cand].T), 0.0)
            pot = np.minimum(d2[:, None], dc).sum(0)
            b = int(np.argmin(pot))
            centres[k] = sub[cand[b]]
            d2 = np.minimum(d2, dc[:, b])
        return centres

    def _device_seeding(self, D):
        """seeding='device' and the kernel takes this feature dimension (otherwise: the host seeding)"""
        return self.seeding == 'device' and D <= api.KMEANSPP_MAX_D

    def _seeds(self, ctx, X, n, D, rng):
        """the k-means++ centres of one start: on the host, or (seeding='device') the same draws through ONE ssp_kmeanspp_seed problem on
        the device matrix X — only the K centres come back"""
        if not self._device_seeding(D):
            return self._kmeanspp(X, n, D, rng)
        idx, first, u = _kmeanspp_draws(rng, n, self.n_components)
        res = api.kmeanspp_seeds(ctx, X, self.n_components, [first], u[None], sel=idx if len(idx) < n else None)
        return res["centres"][0]

    @staticmethod
    def _lloyd_start(K, D, gvar):
        """(weights, spherical variances) of the Lloyd passes: the hard-assignment limit of the E step"""
        return np.full(K, 1.0 / K), np.full((K, D), max(1e-2 * float(gvar.mean()), 1e-12))

    @staticmethod
    def _lloyd_update(st, centres, gvar):
        """one Lloyd step from the statistics at `centres` -> (new centres, done)"""
        nk = np.maximum(st["nk"], 1e-12)
        new = np.where(st["nk"][:, None] > 0.5, st["sx"] / nk[:, None], centres)  # an empty cluster keeps its centre
        shift = float(((new - centres) ** 2).sum())
        return new, shift <= 1e-4 * float(gvar.sum())

    def _kmeans(self, ctx, X, n, D, rng, gvar):
        """k-means++ seeds (on <= 20000 sampled frames; host or device, see ``seeding``) + Lloyd on the GPU; returns the clusters'
        (nk, sx, sxx)."""
        K = self.n_components
        centres = self._seeds(ctx, X, n, D, rng)
        w, tau = self._lloyd_start(K, D, gvar)
        st = None
        for _ in range(30):
            st = api.gmm_em_stats(ctx, w, centres, tau, X)
            centres, done = self._lloyd_update(st, centres, gvar)
            if done:
                break
        return st, centres

    def _need_start(self):
        return self.means_init is None or self.precisions_init is None or self.weights_init is None

    def _global_var(self, g, n):
        """global variance (+ reg_covar) from the K = 1 statistics with unit responsibilities"""
        mu = g["sx"][0] / n
        return np.maximum(g["sxx"][0] / n - mu * mu, 0.0) + self.reg_covar

    def _initial(self, ctx, X, n, D, rng):
        K = self.n_components
        gvar = g = None
        st = centres = drawn = None
        if self._need_start():
            # global variance through the same kernels: one component with unit responsibilities
            g = api.gmm_em_stats(ctx, np.ones(1), np.zeros((1, D)), np.ones((1, D)), X)
            gvar = self._global_var(g, n)
            if self.init_params == 'kmeans' and K > 1:
                st, centres = self._kmeans(ctx, X, n, D, rng, gvar)
        if self.means_init is None and centres is None and K != 1:
            drawn = self._rows(X, np.sort(rng.choice(n, size=K, replace=False)))
        return self._start(n, D, g, gvar, st, centres, drawn)

    def _start(self, n, D, g, gvar, st, centres, drawn):
        """the initial (weights, means, covars) from the given *_init arrays, else the k-means clusters (st, centres), the frames
        drawn for 'random_from_data' and the global statistics g / variance gvar"""
        K = self.n_components
        if self.means_init is not None:
            means = np.array(self.means_init, dtype=np.float64).reshape(K, D)
        elif centres is not None:
            means = centres
        elif K == 1:
            means = (g["sx"][0] / n)[None]
        else:
            means = drawn
        if self.precisions_init is not None:
            covars = 1.0 / np.array(self.precisions_init, dtype=np.float64).reshape(K, D)
        elif st is not None:  # per-cluster variances (sklearn: _estimate_gaussian_covariances_diag of the one-hot resp)
            nk = st["nk"] + 10 * np.finfo(np.float64).eps
            covars = np.maximum(st["sxx"] / nk[:, None] - (st["sx"] / nk[:, None]) ** 2, 0.0) + self.reg_covar
            covars = np.where(st["nk"][:, None] > 1.5, covars, gvar[None])
        else:
            covars = np.tile(gvar, (K, 1))
        if self.weights_init is not None:
            weights = np.array(self.weights_init, dtype=np.float64).reshape(K)
        elif st is not None:
            weights = np.maximum(st["nk"], 1.0) / np.maximum(st["nk"], 1.0).sum()
        else:
            weights = np.full(K, 1.0 / K)
        return weights, means, covars

    # ---- covariance_type='full': sklearn's M step from the raw moments about a shift (include/ssp.h, ssp_gmm_full_em_stats), float64
    def _m_step_full(self, st, n, shift=None):
        """(weights, means, covariances (K,D,D), precisions_cholesky) from nk, sx, sxx taken about ``shift``: algebraically
        _estimate_gaussian_parameters / _estimate_gaussian_covariances_full, then _compute_precision_cholesky (its ValueError too)"""
        nk = st["nk"] + 10 * np.finfo(np.float64).eps
        m = st["sx"] / nk[:, None]
        covs = st["sxx"] / nk[:, None, None] - m[:, :, None] * m[:, None, :]
        D = m.shape[1]
        covs[:, np.arange(D), np.arange(D)] += self.reg_covar
        weights = nk / n
        means = m if shift is None else m + np.asarray(shift, dtype=np.float64)[None]
        return weights / weights.sum(), means, covs, precision_cholesky_full(covs)

    def _full_start(self, ctx, X, n, D, rng, shift):
        """the initial (weights, means, precisions_cholesky) of one 'full' start: the *_init arrays as sklearn's _initialize takes them, else
        the k-means++ / Lloyd stage of the 'diag' path with the clusters' full covariances from ONE ssp_gmm_full_em_stats call at the final
        centres (a small shared spherical variance: the hard-assignment limit); a cluster of fewer than D + 1 frames takes the global
        covariance.  'random_from_data': K frames as means, the global covariance, uniform weights."""
        K = self.n_components
        eye = np.eye(D)
        weights = means = U = None
        if self.weights_init is not None:
            weights = np.array(self.weights_init, dtype=np.float64).reshape(K)
        if self.means_init is not None:
            means = np.array(self.means_init, dtype=np.float64).reshape(K, D)
        if self.precisions_init is not None:
            U = precision_cholesky_from_precisions_full(np.array(self.precisions_init, dtype=np.float64).reshape(K, D, D))
        if weights is not None and means is not None and U is not None:
            return weights, means, U
        g = api.gmm_full_em_stats(ctx, np.ones(1), shift[None], eye[None], X, shift=shift)
        gm = g["sx"][0] / n
        gcov = g["sxx"][0] / n - np.outer(gm, gm) + self.reg_covar * eye
        gvar = np.maximum(np.diag(gcov), self.reg_covar)
        st = None
        if self.init_params == 'kmeans' and K > 1 and (means is None or U is None or weights is None):
            _, centres = self._kmeans(ctx, X, n, D, rng, gvar)
            tau = max(1e-2 * float(gvar.mean()), 1e-12)
            st = api.gmm_full_em_stats(ctx, np.full(K, 1.0 / K), centres, np.tile(eye / np.sqrt(tau), (K, 1, 1)), X, shift=shift)
            if means is None:
                means = centres
        if means is None:
            means = (gm + shift)[None] if K == 1 else self._rows(X, np.sort(rng.choice(n, size=K, replace=False)))
        if U is None:
            covs = np.tile(gcov, (K, 1, 1))
            if st is not None:
                nk = st["nk"] + 10 * np.finfo(np.float64).eps
                m = st["sx"] / nk[:, None]
                own = st["sxx"] / nk[:, None, None] - m[:, :, None] * m[:, None, :] + self.reg_covar * eye[None]
                covs = np.where((st["nk"] >= D + 1)[:, None, None], own, covs)
            try:
                U = precision_cholesky_full(covs)
            except ValueError:  # (a cluster whose frames span no D dimensions: the global covariance, as for a small one)
                U = precision_cholesky_full(np.tile(gcov, (K, 1, 1)))
        if weights is None:
            weights = np.maximum(st["nk"], 1.0) / np.maximum(st["nk"], 1.0).sum() if st is not None else np.full(K, 1.0 / K)
        return weights, means, U

    def _fit_full(self, ctx, X, n, D, rng):
        import torch
        shift = (X.sum(dim=0, dtype=torch.float64) / n).cpu().numpy()  # the global mean: where the statistics' float32 rounding happens
        best = None
        for _ in range(self.n_init):
            weights, means, U = self._full_start(ctx, X, n, D, rng, shift)
            covars = None
            lower, converged, n_iter = -np.inf, False, 0
            for n_iter in range(1, self.max_iter + 1):
                prev = lower
                st = api.gmm_full_em_stats(ctx, weights, means, U, X, shift=shift)
                weights, means, covars, U = self._m_step_full(st, n, shift)
                lower = st["loglik_sum"] / n
                if abs(lower - prev) < self.tol:
                    converged = True
                    break
            if best is None or lower > best[0]:
                best = (lower, weights, means, covars, n_iter, converged, U)
        self.lower_bound_, self.weights_, self.means_, self.covariances_, self.n_iter_, self.converged_, self.precisions_cholesky_ = best
        self.precisions_ = np.einsum('kij,klj->kil', self.precisions_cholesky_, self.precisions_cholesky_)
        return self

    def fit(self, X, y=None):
        """EM until |delta lower bound| < tol or max_iter (sk:mixture/_base.py fit_predict), best of n_init starts."""
        ctx = self._ctx or api.default_context()
        if not api._is_torch(X):
            X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("X must be (n_samples, n_features)")
        n, D = int(X.shape[0]), int(X.shape[1])
        if n < self.n_components:
            raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d"
                             % (self.n_components, n))
        if not api._is_torch(X):  # one upload for every EM / Lloyd iteration instead of one per ssp_gmm_em_stats call
            import torch
            X = torch.from_numpy(X).to("cuda:%d" % ctx.device)
            torch.cuda.synchronize()
        # sklearn validates its input (ValueError on NaN / infinity); the EM kernels answer such a row with NaN statistics, and
        # |NaN - prev| < tol never holds: without this look the loop would run max_iter iterations and leave a model of NaNs
        bad = _first_bad_row(X) if n > 0 else None
        if bad is not None:
            raise ValueError(_nonfinite_message("", bad))
        rng = np.random.RandomState(self.random_state) if not isinstance(self.random_state, np.random.RandomState) else self.random_state
        if self.covariance_type == 'full':
            if D > api.GMM_FULL_MAX_D:
                raise NotImplementedError("covariance_type='full' covers at most %d features" % api.GMM_FULL_MAX_D)
            return self._fit_full(ctx, X, n, D, rng)
        best = None
        for _ in range(self.n_init):
            weights, means, covars = self._initial(ctx, X, n, D, rng)
            lower, converged, n_iter = -np.inf, False, 0
            for n_iter in range(1, self.max_iter + 1):
                prev = lower
                st = api.gmm_em_stats(ctx, weights, means, covars, X)
                weights, means, covars = self._m_step(st, n)
                lower = st["loglik_sum"] / n
                if abs(lower - prev) < self.tol:
                    converged = True
                    break
            if best is None or lower > best[0]:
                best = (lower, weights, means, covars, n_iter, converged)
        self.lower_bound_, self.weights_, self.means_, self.covariances_, self.n_iter_, self.converged_ = best
        self.precisions_cholesky_ = 1.0 / np.sqrt(self.covariances_)
        self.precisions_ = self.precisions_cholesky_ ** 2
        return self

    # ---- scoring through the MFMA scorer (api.GmmScorer), same numbers as sklearn's methods
    def _scorer(self):
        ctx = self._ctx or api.default_context()
        if self.covariance_type == 'full':
            return api.GmmFullScorer(ctx, self.weights_[None], self.means_[None], self.precisions_cholesky_[None], has_ubm=False), ctx
        return api.GmmScorer(ctx, self.weights_[None], self.means_[None], self.covariances_[None], has_ubm=False), ctx

    # (sklearn raises ValueError on a NaN / infinite entry; the scorer answers one with NaN at that frame and in the utterance's score
    #  — include/ssp.h, ssp_gmm_score — so the answer is read off the result: no extra pass over X)
    def score_samples(self, X):
        sc, ctx = self._scorer()
        X = np.ascontiguousarray(X, dtype=np.float32)
        seg = api.Segments.from_lengths(ctx, [X.shape[0]])
        ll = np.asarray(sc.score(X, seg, loglik=True, scores=False, argmax=False)["loglik"], dtype=np.float64)[0]
        bad = np.flatnonzero(~np.isfinite(ll))
        if bad.size:
            raise ValueError(_nonfinite_message("", int(bad[0])))
        return ll

    def score(self, X, y=None):
        sc, ctx = self._scorer()
        X = np.ascontiguousarray(X, dtype=np.float32)
        seg = api.Segments.from_lengths(ctx, [X.shape[0]])
        v = float(np.asarray(sc.score(X, seg, loglik=False, scores=True, argmax=False)["scores"])[0, 0])
        if X.shape[0] > 0 and not np.isfinite(v):
            raise ValueError(_nonfinite_message(""))
        return v


def _m_step_many(nk, sx, sxx, n, reg_covar):
    """GaussianMixture._m_step over a batch of models, element for element the same float64 operations: nk (B,K), sx / sxx (B,K,D),
    n (B,) frames per model."""
    nk = nk + 10 * np.finfo(np.float64).eps
    means = sx / nk[:, :, None]
    avg_X2 = sxx / nk[:, :, None]
    covars = avg_X2 - 2 * (means * sx / nk[:, :, None]) + means ** 2 + reg_covar
    weights = nk / n[:, None]
    return weights / weights.sum(axis=1, keepdims=True), means, covars


def _per_model(v, M, base_ndim):
    """an *_init argument of fit_many: None, one array for every model, or a sequence of M arrays -> list of M"""
    if v is None:
        return [None] * M
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == base_ndim + 1 and a.shape[0] == M:
        return [a[m] for m in range(M)]
    return [v] * M


def _fits_one_by_one(gms):
    """the models of a fit_many call are covariance_type='full': fitted one after the other (no batched full-covariance kernel)"""
    return gms[0].covariance_type == 'full'


def _host_f32(X):
    if api._is_torch(X):
        X = X.detach().cpu().numpy()
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise ValueError("X must be (n_samples, n_features)")
    return X


def fit_many(Xs, n_components=1, profile=None, **kwargs):
    """Fit one GaussianMixture per array of ``Xs`` (the per-speaker loop of GMM_UBM.py:154-170) with ONE ssp_gmm_em_stats_batch call
    per iteration for all models still running; returns the fitted GaussianMixture objects in the order of ``Xs``.

    ``kwargs`` are the constructor's; ``weights_init`` / ``means_init`` / ``precisions_init`` may be one array or a sequence of M.
    The features go to the device once.  Every stage is batched over the models (and ``n_init`` starts) still active: the global
    variance pass, Lloyd with per-model stop tests, EM with per-model convergence and best-start selection.  k-means++ seeding runs on
    the host by default: an int or None ``random_state`` gives every model its own RandomState (as a loop of ``fit`` does; the seeding then
    runs in a thread pool), a shared RandomState instance is drawn from in model order, as the loop draws.  ``seeding='device'``: the same
    draws, then ONE ssp_kmeanspp_seed call for every (model, start) on the uploaded matrix (D <= 64; above that the host seeding).  For K <= 64, D <= 47 the fitted
    attributes are bit for bit those of ``GaussianMixture(**kwargs).fit(X)`` per model.  D > 47: the loop of ``fit``.
    ``profile``: a dict that receives the time split (kernel ms, host M step, k-means++ seconds and — device seeding — its kernel ms;
    measurement only)."""
    import time
    Xs = list(Xs)
    M = len(Xs)
    if M == 0:
        return []
    inits = {name: _per_model(kwargs.pop(name, None), M, nd)
             for name, nd in (("weights_init", 1), ("means_init", 2),
                              ("precisions_init", 3 if kwargs.get("covariance_type", "diag") == "full" else 2))}
    gms = [GaussianMixture(n_components=n_components, weights_init=inits["weights_init"][m], means_init=inits["means_init"][m],
                           precisions_init=inits["precisions_init"][m], **kwargs) for m in range(M)]
    hosts = [_host_f32(X) for X in Xs]
    D = int(hosts[0].shape[1])
    K = gms[0].n_components
    for X in hosts:
        if X.shape[1] != D:
            raise ValueError("every X must have the same number of features")
        if X.shape[0] < K:
            raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d" % (K, X.shape[0]))
    if 2 * D + 1 > 96 or _fits_one_by_one(gms):  # no batched kernel (ssp_gmm_em_stats_batch: D <= 47, 'diag' only)
        out = []
        for m, (gm, X) in enumerate(zip(gms, hosts)):
            try:
                out.append(gm.fit(X))
            except ValueError as e:
                raise ValueError("model %d: %s" % (m, e)) from None
        return out
    g0 = gms[0]
    ctx = g0._ctx or api.default_context()
    ns = np.array([X.shape[0] for X in hosts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    import torch
    feats = torch.from_numpy(np.concatenate(hosts)).to("cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    # sklearn's input validation, before any model is touched: one reduction over the rows that already sit on the device
    bad = _first_bad_row(feats)
    if bad is not None:
        m = int(np.searchsorted(offs, bad, side="right")) - 1
        raise ValueError(_nonfinite_message(" of model %d" % m, bad - int(offs[m])))
    prof = profile if profile is not None else {}
    for k in ("kernel_ms", "mstep_s", "kmeanspp_s", "kmeanspp_kernel_ms", "calls", "em_iters"):
        prof.setdefault(k, 0.0)
    timing = profile is not None

    def stats(w, mu, cv, models):
        st = api.gmm_em_stats_batch(ctx, w, mu, cv, feats, offs[models], ns[models], timing=timing)
        prof["kernel_ms"] += st.get("kernel_ms", 0.0)
        prof["calls"] += 1
        return st

    # ---- global variance of every model that needs a start (K = 1, unit responsibilities)
    g_st, gvar = [None] * M, [None] * M
    need = [m for m in range(M) if gms[m]._need_start()]
    if need:
        B = len(need)
        st = stats(np.ones((B, 1)), np.zeros((B, 1, D)), np.ones((B, 1, D)), np.array(need))
        for i, m in enumerate(need):
            g_st[m] = {"nk": st["nk"][i], "sx": st["sx"][i], "sxx": st["sxx"][i], "loglik_sum": float(st["loglik_sum"][i])}
            gvar[m] = gms[m]._global_var(g_st[m], int(ns[m]))
    # ---- the random draws of every start, model by model and start by start (what a loop of fit draws, in its order)
    items = [(m, r) for m in range(M) for r in range(gms[m].n_init)]
    seeds = {}

    device = g0._device_seeding(D)

    def draw(m):
        gm, X, n = gms[m], hosts[m], int(ns[m])
        rs = gm.random_state
        rng = rs if isinstance(rs, np.random.RandomState) else np.random.RandomState(rs)
        out = []
        for _ in range(gm.n_init):
            centres = drawn = None
            if gm._need_start() and gm.init_params == 'kmeans' and K > 1:
                centres = _kmeanspp_draws(rng, n, K) if device else gm._kmeanspp(X, n, D, rng)
            if gm.means_init is None and centres is None and K != 1:
                drawn = gm._rows(X, np.sort(rng.choice(n, size=K, replace=False)))
            out.append((centres, drawn))
        return out

    t0 = time.perf_counter()
    shared = any(isinstance(gm.random_state, np.random.RandomState) for gm in gms)
    if shared or M == 1 or device:
        drawn_all = [draw(m) for m in range(M)]
    else:
        import os
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1, M))) as ex:
            drawn_all = list(ex.map(draw, range(M)))
    for m, r in items:
        seeds[(m, r)] = drawn_all[m][r]
    if device:  # ONE ssp_kmeanspp_seed call for every (model, start) on the matrix already uploaded; only the centres come back
        todo = [it for it in items if seeds[it][0] is not None]
        if todo:
            whole = all(len(seeds[it][0][0]) == int(ns[it[0]]) for it in todo)  # no model above the subsample cap: row ranges
            cnt = np.array([len(seeds[it][0][0]) for it in todo], dtype=np.int64)
            if whole:
                sel, off = None, offs[[m for m, _r in todo]]
            else:
                sel = np.concatenate([seeds[it][0][0] + offs[it[0]] for it in todo])
                off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
            res = api.kmeanspp_seeds(ctx, feats, K, [seeds[it][0][1] for it in todo], np.stack([seeds[it][0][2] for it in todo]),
                                     row_off=off, n_sel=cnt, sel=sel, timing=timing)
            prof["kmeanspp_kernel_ms"] += res.get("kernel_ms", 0.0)
            for i, it in enumerate(todo):
                seeds[it] = (res["centres"][i], seeds[it][1])
    prof["kmeanspp_s"] += time.perf_counter() - t0
    # ---- Lloyd on every k-means start at once, each with its own stop test
    lloyd = {it: None for it in items if seeds[it][0] is not None}
    cen = {it: seeds[it][0] for it in lloyd}
    active = list(lloyd)
    for _ in range(30):
        if not active:
            break
        ws, taus = zip(*(GaussianMixture._lloyd_start(K, D, gvar[m]) for m, _r in active))
        st = stats(np.stack(ws), np.stack([cen[it] for it in active]), np.stack(taus), np.array([m for m, _r in active]))
        still = []
        for i, it in enumerate(active):
            sti = {"nk": st["nk"][i], "sx": st["sx"][i], "sxx": st["sxx"][i], "loglik_sum": float(st["loglik_sum"][i])}
            lloyd[it] = sti
            cen[it], done = GaussianMixture._lloyd_update(sti, cen[it], gvar[it[0]])
            if not done:
                still.append(it)
        active = still
    # ---- starts, then EM on every start of every model at once
    par = {}
    for it in items:
        m = it[0]
        centres = cen.get(it)
        par[it] = gms[m]._start(int(ns[m]), D, g_st[m], gvar[m], lloyd.get(it), centres, seeds[it][1])
    state = {it: [-np.inf, False, 0] for it in items}  # lower bound, converged, n_iter
    tol, reg, max_iter = g0.tol, g0.reg_covar, g0.max_iter
    active = list(items)
    for n_iter in range(1, max_iter + 1):
        if not active:
            break
        models = np.array([m for m, _r in active])
        st = stats(np.stack([par[it][0] for it in active]), np.stack([par[it][1] for it in active]),
                   np.stack([par[it][2] for it in active]), models)
        prof["em_iters"] += 1
        t0 = time.perf_counter()
        n_act = ns[models].astype(np.float64)
        w, mu, cv = _m_step_many(st["nk"], st["sx"], st["sxx"], n_act, reg)
        lower = st["loglik_sum"] / n_act
        prof["mstep_s"] += time.perf_counter() - t0
        still = []
        for i, it in enumerate(active):
            par[it] = (w[i], mu[i], cv[i])
            prev = state[it][0]
            state[it] = [float(lower[i]), False, n_iter]
            if abs(state[it][0] - prev) < tol:
                state[it][1] = True
            else:
                still.append(it)
        active = still
    for m, gm in enumerate(gms):
        best = None
        for r in range(gm.n_init):
            lower, converged, n_iter = state[(m, r)]
            if best is None or lower > best[0]:
                best = (lower, *par[(m, r)], n_iter, converged)
        gm.lower_bound_, gm.weights_, gm.means_, gm.covariances_, gm.n_iter_, gm.converged_ = best
        gm.precisions_cholesky_ = 1.0 / np.sqrt(gm.covariances_)
        gm.precisions_ = gm.precisions_cholesky_ ** 2
    return gms


def _check_fitted_ubm(ubm):
    for name in ("weights_", "means_", "covariances_"):
        if not hasattr(ubm, name):
            raise ValueError("This GaussianMixture instance is not fitted yet: the UBM has no %s" % name)


def _diag_ubm_arrays(ubm):
    """-> float64 weights (K,), means (K,D), covariances (K,D) of a fitted diagonal UBM"""
    w = np.asarray(ubm.weights_, dtype=np.float64)
    mu = np.asarray(ubm.means_, dtype=np.float64)
    cv = np.asarray(ubm.covariances_, dtype=np.float64)
    if mu.ndim != 2 or cv.shape != mu.shape or w.shape != mu.shape[:1]:
        raise ValueError("only covariance_type='diag' UBMs are supported (MAP adaptation and the Baum-Welch statistics of a "
                         "covariance_type='full' UBM are not built: fit and score full models through gmm_train / GMM_UBM.score_matrix)")
    return w, mu, cv


def _shared_stats(w, mu, cv, Xs, ctx):
    """the statistics of every array of the non-empty list ``Xs`` under one model, in ONE ssp_gmm_em_stats_shared call, with sklearn's
    input validation (widths, empty arrays, non-finite rows: the message names the speaker and row) -> (ctx, frames per array, statistics)"""
    D = mu.shape[1]
    hosts = [_host_f32(X) for X in Xs]
    for X in hosts:
        if X.shape[1] != D:
            raise ValueError("X has %d features, but the UBM is expecting %d features as input." % (X.shape[1], D))
        if X.shape[0] < 1:
            raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required.")
    ctx = ctx or api.default_context()
    ns = np.array([X.shape[0] for X in hosts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    import torch
    feats = torch.from_numpy(np.concatenate(hosts)).to("cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    bad = _first_bad_row(feats)
    if bad is not None:
        m = int(np.searchsorted(offs, bad, side="right")) - 1
        raise ValueError(_nonfinite_message(" of speaker %d" % m, bad - int(offs[m])))
    return ctx, ns, api.gmm_em_stats_shared(ctx, w, mu, cv, feats, offs, ns)


def map_adapt(ubm, Xs, relevance_factor=16.0, adapt='m', ctx=None):
    """MAP adaptation of a fitted UBM to every array of ``Xs`` (Reynolds, Quatieri, Dunn 2000) — an extension: the reference trains each
    speaker's mixture independently (GMM_UBM.py:158-170).  ONE ssp_gmm_em_stats_shared call gives every speaker's n = nk, Ex = sx / n,
    Exx = sxx / n under the UBM; then in float64, with alpha = n / (n + relevance_factor) per mixture:
      'm'  means        alpha Ex + (1 - alpha) mu
      'w'  weights      alpha n / T + (1 - alpha) w, renormalised to sum 1
      'v'  covariances  alpha Exx + (1 - alpha) (sigma^2 + mu^2) - (new mean)^2, floored at the UBM's reg_covar
    ``adapt``: any non-empty combination of these letters; what is not adapted is the UBM's array, element for element (with 'm' alone
    the models are what api.MapScorer takes).  A mixture with n = 0 keeps the UBM's values.  Returns one GaussianMixture per array, every
    sklearn attribute set (converged_ = True, n_iter_ = 1).  ValueError as sklearn raises it: a non-finite row (the message names the
    speaker and row), mismatched feature widths, an unfitted ubm."""
    _check_fitted_ubm(ubm)
    if not isinstance(adapt, str) or not adapt or set(adapt) - set("mwv"):
        raise ValueError("adapt must be a non-empty combination of 'm', 'w' and 'v'")
    r = float(relevance_factor)
    if not r >= 0.0:
        raise ValueError("relevance_factor must be >= 0")
    w, mu, cv = _diag_ubm_arrays(ubm)
    K = mu.shape[0]
    Xs = list(Xs)
    if not Xs:
        return []
    ctx, ns, st = _shared_stats(w, mu, cv, Xs, ctx or getattr(ubm, "_ctx", None))
    w_new, mu_new, cv_new = _map_formulas(w, mu, cv, st["nk"], st["sx"], st["sxx"], ns, r, adapt, float(getattr(ubm, "reg_covar", 1e-6)))
    out = []
    for s in range(len(Xs)):
        gm = GaussianMixture(n_components=K, covariance_type='diag', reg_covar=float(getattr(ubm, "reg_covar", 1e-6)), ctx=ctx)
        gm.weights_ = w_new[s] if 'w' in adapt else w
        gm.means_ = mu_new[s] if 'm' in adapt else mu
        gm.covariances_ = cv_new[s] if 'v' in adapt else cv
        gm.precisions_cholesky_ = 1.0 / np.sqrt(gm.covariances_)
        gm.precisions_ = gm.precisions_cholesky_ ** 2
        gm.converged_, gm.n_iter_ = True, 1
        gm.lower_bound_ = float(st["loglik_sum"][s] / ns[s])  # of the E step under the UBM, as the first EM iteration would record it
        out.append(gm)
    return out


def _map_formulas(w, mu, cv, nk, sx, sxx, T, r, adapt, reg_covar):
    """the adaptation arithmetic over a batch: nk (S,K), sx / sxx (S,K,D), T (S,) frames -> (weights (S,K), means, covariances (S,K,D));
    every quantity is computed whatever ``adapt`` says (the caller picks)"""
    n = nk[:, :, None]
    has = n > 0.0
    safe = np.where(has, n, 1.0)
    Ex = np.where(has, sx / safe, mu[None])
    Exx = np.where(has, sxx / safe, (cv + mu * mu)[None])
    alpha = np.where(has, n / (n + r) if r > 0.0 else 1.0, 0.0) if np.isfinite(r) else np.zeros_like(n)
    m_new = alpha * Ex + (1.0 - alpha) * mu[None]
    m_used = m_new if 'm' in adapt else np.broadcast_to(mu[None], m_new.shape)
    a1 = alpha[:, :, 0]
    w_new = a1 * nk / np.asarray(T, dtype=np.float64)[:, None] + (1.0 - a1) * w[None]
    w_new = w_new / w_new.sum(axis=1, keepdims=True)
    v_new = np.maximum(alpha * Exx + (1.0 - alpha) * (cv + mu * mu)[None] - m_used ** 2, reg_covar)
    v_new = np.where(has, v_new, cv[None])  # (n = 0 keeps the UBM's values exactly: (cv + mu^2) - mu^2 rounds)
    return w_new, m_new, v_new
