"""Float64 restatement of the PLDA back end (include/ssp.h, the ssp_plda block): class statistics, the EM of the two-covariance model,
its diagonalisation, LDA, the log-likelihood ratio in its direct and its packed form — and the seeded case builders the PLDA tests share.
Written from the definitions, class by class and row by row, not from speech_signal_processing_amd/plda.py (which groups classes by
their count).  numpy only."""
import numpy as np

KC = 1024  # rows per chain of the scatter product


# ------------------------------------------------------------------------------------------------------------------------ statistics
def class_stats(X, labels, S):
    """counts (S,), sums (S, q) float64 added in row order, the mean of all rows (the class sums added in ascending class order, over
    N), the centred rows rounded to float32 once (as float32), and S_w of those rounded rows in float64"""
    X = np.asarray(X, dtype=np.float32)
    labels = np.asarray(labels)
    N, q = X.shape
    X64 = X.astype(np.float64)
    cnt = np.zeros(S, dtype=np.int64)
    sums = np.zeros((S, q))
    for s in range(S):
        rows = X64[labels == s]
        cnt[s] = rows.shape[0]
        if rows.shape[0]:
            sums[s] = np.cumsum(rows, axis=0)[-1]   # (a running sum: row order)
    mu = np.zeros(q)
    for s in range(S):
        mu = mu + sums[s]
    mu = mu / N
    means = np.divide(sums, cnt[:, None], out=np.zeros_like(sums), where=cnt[:, None] > 0)
    Xc = (X64 - means[labels]).astype(np.float32)
    Xc64 = Xc.astype(np.float64)
    return {"count": cnt, "sum": sums, "mean": mu, "class_mean": means, "xc": Xc, "sw": Xc64.T @ Xc64}


def sw_fp32_emulation(Xc):
    """the device's steps in float32: every chunk of 1024 rows one chain in row order (a multiply and an add per step, each rounded:
    no worse than the fused steps of the matrix instruction), the chunks added in float64 in ascending order"""
    Xc = np.asarray(Xc, dtype=np.float32)
    q = Xc.shape[1]
    total = np.zeros((q, q))
    for k0 in range(0, Xc.shape[0], KC):
        acc = np.zeros((q, q), dtype=np.float32)
        for x in Xc[k0:k0 + KC]:
            acc = acc + np.outer(x, x)
        total += acc.astype(np.float64)
    return total


# ------------------------------------------------------------------------------------------------------------------------------- EM
def objective(W, B, sw, class_means, counts, mu):
    """sum_s -1/2 [(n_s - 1) log|W| + log|B + W/n_s| + (m_s - mu)' (B + W/n_s)^-1 (m_s - mu)] - 1/2 tr(W^-1 S_w)"""
    ldW = np.linalg.slogdet(W)[1]
    o = -0.5 * np.trace(np.linalg.solve(W, sw))
    for m, n in zip(class_means, counts):
        T = B + W / n
        d = m - mu
        o -= 0.5 * ((n - 1) * ldW + np.linalg.slogdet(T)[1] + d @ np.linalg.solve(T, d))
    return o


def em(sw, class_means, counts, mu, n_iter):
    """Kaldi's PldaEstimator from W = B = I, one class at a time; classes without rows must have been dropped.
    -> W, B, objective (n_iter,): objective[it] belongs to the (W, B) iteration ``it`` started from"""
    sw = np.asarray(sw, dtype=np.float64)
    q, S, N = sw.shape[0], len(counts), int(np.sum(counts))
    W, B = np.eye(q), np.eye(q)
    obj = []
    for _ in range(n_iter):
        obj.append(objective(W, B, sw, class_means, counts, mu))
        Wi, Bi = np.linalg.inv(W), np.linalg.inv(B)
        b_stats, w_stats = np.zeros((q, q)), sw.copy()
        for m, n in zip(class_means, counts):
            V = np.linalg.inv(Bi + n * Wi)            # posterior covariance of the speaker variable
            d = m - mu
            w = V @ (n * (Wi @ d))                    # its posterior mean
            r = d - w
            b_stats += V + np.outer(w, w)
            w_stats += n * (V + np.outer(r, r))
        B, W = b_stats / S, w_stats / N
        B, W = (B + B.T) / 2, (W + W.T) / 2
    return W, B, np.array(obj)


def _signs(rows):
    out = rows.copy()
    for r in out:
        if r[np.argmax(np.abs(r))] < 0:
            r *= -1.0
    return out


def diagonalise(W, B):
    """A, psi: A W A' = I, A B A' = diag(psi), psi descending, the largest-magnitude entry of each row of A positive"""
    L = np.linalg.cholesky(W)
    Li = np.linalg.inv(L)
    M = Li @ B @ Li.T
    psi, U = np.linalg.eigh((M + M.T) / 2)
    order = np.argsort(-psi, kind="stable")
    return _signs(U[:, order].T @ Li), psi[order]


def lda(sw, class_means, counts, mu, p):
    """V (q, p), lambda (p,): the top p generalised eigenvectors of S_b v = lambda S_w v with v' S_w v = 1; also returns S_b"""
    d = np.asarray(class_means) - mu
    Sb = sum(n * np.outer(v, v) for v, n in zip(d, counts))
    rows, lam = diagonalise(sw, Sb)
    return rows[:p].T, lam[:p], Sb


# -------------------------------------------------------------------------------------------------------------------------- scoring
def speaker_terms(psi, enrol_mean, counts):
    """mean (S, q) and var (S, q) of the predictive density of a test vector given each speaker's enrolment"""
    psi = np.asarray(psi, dtype=np.float64)
    n = np.asarray(counts, dtype=np.float64)[:, None]
    den = n * psi + 1.0
    return n * psi * np.asarray(enrol_mean, dtype=np.float64) / den, 1.0 + psi / den


def llr_direct(psi, enrol_mean, counts, T):
    """LLR (N, S) = -1/2 sum_d [log var + (t - mean)^2 / var] + 1/2 sum_d [log(1 + psi) + t^2 / (1 + psi)]"""
    mean, var = speaker_terms(psi, enrol_mean, counts)
    T = np.asarray(T, dtype=np.float64)
    out = np.empty((T.shape[0], mean.shape[0]))
    base = 0.5 * (np.log1p(psi).sum() + (T * T / (1.0 + psi)).sum(axis=1))
    for s in range(mean.shape[0]):
        out[:, s] = -0.5 * (np.log(var[s]).sum() + ((T - mean[s]) ** 2 / var[s]).sum(axis=1)) + base
    return out


def pack(psi, enrol_mean, counts):
    """beta (S, q), alpha (S, q), c (S,) of LLR = sum beta t - 1/2 sum alpha t^2 + c"""
    mean, var = speaker_terms(psi, enrol_mean, counts)
    psi = np.asarray(psi, dtype=np.float64)
    return mean / var, 1.0 / var - 1.0 / (1.0 + psi), -0.5 * (np.log(var) - np.log1p(psi) + mean * mean / var).sum(axis=1)


def llr_packed(beta, alpha, c, T, dtype=np.float64):
    """the packed form in ``dtype`` (float32: the emulation of the device's arithmetic up to the order of the sums)"""
    T = np.asarray(T, dtype=dtype)
    return T @ beta.astype(dtype).T + (T * T) @ (-0.5 * alpha).astype(dtype).T + c.astype(dtype)


def llr_bound(ref):
    """per row: 1e-4 max(1, max |ref row|)"""
    return 1e-4 * np.maximum(1.0, np.abs(ref).max(axis=1))


def decided_rows(ref):
    """rows whose float64 gap between the best and the second-best ratio exceeds twice the row's bound (every row when S = 1)"""
    if ref.shape[1] < 2:
        return np.ones(ref.shape[0], dtype=bool)
    top = np.sort(ref, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) > 2.0 * llr_bound(ref)


# ---------------------------------------------------------------------------------------------------------------------------- cases
def counts_for(G, S, rng):
    """S enrolment counts with exactly min(G, S) distinct values, n = 1 and n = 1000 among them when G >= 2"""
    pool = {1: [1], 3: [1, 5, 1000], 32: list(range(1, 32)) + [1000], 40: list(range(1, 40)) + [1000]}[G]
    pool = pool[:S] if S < len(pool) else pool
    c = np.array([pool[i % len(pool)] for i in range(S)], dtype=np.int32)
    return c[rng.permutation(S)]


# (q, S, N, G, psi scale, seed): every q, S, N and G the issue lists; the last is the hard case with psi / 8
SCORER_CASES = [
    (5, 1, 1, 1, 1.0, 1), (5, 33, 129, 3, 1.0, 2), (5, 70, 300, 40, 1.0, 3), (64, 33, 300, 32, 1.0, 4), (64, 70, 129, 40, 1.0, 5),
    (64, 1, 129, 1, 1.0, 6), (200, 70, 300, 3, 1.0, 7), (200, 33, 1, 32, 1.0, 8), (256, 70, 300, 32, 1.0, 9), (256, 33, 129, 3, 1.0, 10),
    (256, 70, 129, 40, 1.0, 11), (5, 70, 300, 3, 0.125, 12),
]
EXCLUSION_CAP = 0.05
_CASES = {}


def scorer_case(case):
    """built directly in the diagonalised space: psi = scale 4 linspace(1, 0.05, q), y_s ~ N(0, diag psi), e_s = y_s + N(0, I / n_s),
    t = y_{s(t)} + N(0, I).  Computed once per case and shared: psi, enrol (S, q) float64, counts, T (N, q) float32, spk (N,), ref (N, S)
    float64 of the float32 T, keep (N,): the rows whose arg-max is decided"""
    if case not in _CASES:
        q, S, N, G, scale, seed = case
        rng = np.random.default_rng(1000 + seed)
        psi = scale * 4.0 * np.linspace(1.0, 0.05, q)
        counts = counts_for(G, S, rng)
        y = rng.standard_normal((S, q)) * np.sqrt(psi)
        enrol = y + rng.standard_normal((S, q)) / np.sqrt(counts)[:, None]
        spk = rng.integers(0, S, N)
        T = (y[spk] + rng.standard_normal((N, q))).astype(np.float32)
        ref = llr_direct(psi, enrol, counts, T)
        _CASES[case] = {"psi": psi, "enrol": enrol, "counts": counts, "T": T, "spk": spk, "ref": ref, "keep": decided_rows(ref),
                        "G": int(np.unique(counts).size)}
    return _CASES[case]


def end_to_end_case(seed=5, q=24, S=30, n_lo=4, n_hi=9):
    """q = 24, S speakers with 4 .. 9 training rows each, generated in an un-diagonalised space through a random mixing matrix; enrolment
    (3 rows per speaker) and test rows (4 per speaker) of the same speakers"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((q, q)) / np.sqrt(q) + np.eye(q)
    psi = 4.0 * np.linspace(1.0, 0.05, q)
    mu = rng.standard_normal(q)
    y = rng.standard_normal((S, q)) * np.sqrt(psi)

    def draw(per):
        lab = np.repeat(np.arange(S), per)
        X = mu + (y[lab] + rng.standard_normal((lab.size, q))) @ M.T
        p = rng.permutation(lab.size)
        return X[p].astype(np.float32), lab[p].astype(np.int32)
    Xtr, ltr = draw(rng.integers(n_lo, n_hi + 1, S))
    Xen, len_ = draw(np.full(S, 3))
    Xte, lte = draw(np.full(S, 4))
    return {"q": q, "S": S, "train": (Xtr, ltr), "enrol": (Xen, len_), "test": (Xte, lte)}


def front(X, mu, V=None, length_norm=True):
    """centre -> LDA -> length normalisation, float64"""
    Y = np.asarray(X, dtype=np.float64) - mu
    if V is not None:
        Y = Y @ V
    return Y / np.linalg.norm(Y, axis=1, keepdims=True) if length_norm else Y
