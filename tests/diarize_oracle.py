"""Restatement in numpy of the diarization block of include/ssp.h (ssp_pairwise_scores, ssp_ahc_cluster), an ordinary module like
tests/snorm_oracle.py.  An extension and unpinned: the reference has no diarization; test_diarize_host.py corroborates ``ahc`` with
SciPy's linkage.  ``pairwise`` is float64; ``ahc`` follows the header's definition operation by operation in the dtype it is given:
in float32 it is the bit-for-bit definition of the kernel's merges, in float64 the yardstick of the margins."""
import numpy as np

LINKAGES = ("average", "complete", "single")
N_LDS = 192   # api.AHC_N_LDS: the longest recording the kernel clusters in LDS


# ------------------------------------------------------------------------------------------------------------------------- scores
def offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off[1:])
    return off


def sq_offsets(counts):
    c = np.asarray(counts, dtype=np.int64)
    return offsets(c * c)


def pairwise(X, off, g=None, h=None, c0=0.0):
    """-> the packed float64 blocks: S[i,j] = sum_d g_d x_id x_jd - (r_i + r_j) + c0, r_i = sum_d h_d x_id^2"""
    X = np.asarray(X, dtype=np.float64)
    q = X.shape[1]
    g = np.ones(q) if g is None else np.asarray(g, dtype=np.float64)
    h = np.zeros(q) if h is None else np.asarray(h, dtype=np.float64)
    out = []
    for r in range(len(off) - 1):
        x = X[off[r]:off[r + 1]]
        ri = (x * x) @ h
        out.append(((x * g) @ x.T - (ri[:, None] + ri[None, :]) + c0).reshape(-1))
    return np.concatenate(out) if out else np.zeros(0)


def blocks(packed, counts):
    """the list of (n_r, n_r) views of a packed batch"""
    sq = sq_offsets(counts)
    return [np.asarray(packed)[sq[r]:sq[r + 1]].reshape(int(n), int(n)) for r, n in enumerate(counts)]


def parity_bound(ref_block):
    """the project's parity bound: 1e-4 max(1, max |S| of the block)"""
    fin = np.isfinite(ref_block)
    return 1e-4 * max(1.0, float(np.abs(ref_block[fin]).max()) if fin.any() else 1.0)


def plda_coeffs(psi):
    """g, h, c0 of the single-enrolment log-likelihood ratio, float64 (include/ssp.h)"""
    psi = np.asarray(psi, dtype=np.float64)
    return psi / (2 * psi + 1), 0.5 * psi ** 2 / ((psi + 1) * (2 * psi + 1)), -0.5 * np.sum(np.log((2 * psi + 1) / (psi + 1) ** 2))


# ---------------------------------------------------------------------------------------------------------------------------- AHC
def ahc(S, linkage="average", threshold=0.0, min_clusters=1, n_speakers=0, dtype=np.float32):
    """One recording: S (n, n), only the entries above the diagonal are read.  -> {"labels" (n,) int32, "n_clusters" int,
    "merge_pair" (n, 2) int32, "merge_score" (n,) dtype, "first_rejected": the score of the pair the threshold turned away (None
    when merging ended for another reason)}.  Naive: the arg-max of every merge is taken over all live pairs."""
    assert linkage in LINKAGES
    S = np.asarray(S)
    n = S.shape[0]
    pairs = np.full((n, 2), -1, dtype=np.int32)
    mscore = np.full(n, np.nan, dtype=dtype)
    res = {"labels": np.zeros(n, dtype=np.int32), "n_clusters": min(n, 1), "merge_pair": pairs, "merge_score": mscore, "first_rejected": None}
    if n == 0:
        return res
    iu = np.triu_indices(n, 1)
    if not np.isfinite(S[iu]).all():
        res["labels"][:] = -1
        res["n_clusters"] = -1
        return res
    W = np.full((n, n), -np.inf, dtype=dtype)
    W[iu] = S[iu].astype(dtype)
    W.T[iu] = W[iu]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    live = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    clus = np.arange(n)
    lo = int(n_speakers) if n_speakers > 0 else max(1, int(min_clusters))
    thr = -np.inf if n_speakers > 0 else threshold
    count, m = n, 0
    while count > lo:
        cand = np.where(upper & live[:, None] & live[None, :], W, -np.inf)
        flat = int(np.argmax(cand))            # the first maximum in row-major order: the smallest a, then the smallest b
        a, b = divmod(flat, n)
        s = W[a, b]
        if not s >= thr:
            res["first_rejected"] = s
            break
        pairs[m] = (a, b)
        mscore[m] = s
        k = live.copy()
        k[[a, b]] = False
        if linkage == "average":
            fa, fb = dtype(size[a]), dtype(size[b])
            new = (fa * W[a, k] + fb * W[b, k]) / (fa + fb)     # every operation rounded in dtype
        elif linkage == "complete":
            new = np.minimum(W[a, k], W[b, k])
        else:
            new = np.maximum(W[a, k], W[b, k])
        W[a, k] = new
        W[k, a] = new
        live[b] = False
        size[a] += size[b]
        clus[clus == b] = a
        count -= 1
        m += 1
    rank = np.cumsum(live) - 1                 # a cluster's index is its smallest member
    res["labels"] = rank[clus].astype(np.int32)
    res["n_clusters"] = count
    return res


def ahc_batch(packed, counts, linkage="average", threshold=0.0, min_clusters=1, n_speakers=None, dtype=np.float32):
    """the recordings of a packed batch -> what api.ahc_cluster(..., merges=True) returns, as numpy arrays"""
    off = offsets(counts)
    lab = np.zeros(off[-1], dtype=np.int32)
    pairs = np.full((off[-1], 2), -1, dtype=np.int32)
    ms = np.full(off[-1], np.nan, dtype=dtype)
    cnt = np.zeros(len(counts), dtype=np.int32)
    for r, B in enumerate(blocks(packed, counts)):
        one = ahc(B, linkage, threshold, min_clusters, 0 if n_speakers is None else int(n_speakers[r]), dtype)
        lab[off[r]:off[r + 1]], pairs[off[r]:off[r + 1]], ms[off[r]:off[r + 1]] = one["labels"], one["merge_pair"], one["merge_score"]
        cnt[r] = one["n_clusters"]
    return {"labels": lab, "n_clusters": cnt, "merge_pair": pairs, "merge_score": ms}


def same_partition(a, b):
    """two label vectors name the same partition"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return False
    fwd, back = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(x, y) != y or back.setdefault(y, x) != x:
            return False
    return True


# -------------------------------------------------------------------------------------------------------------------------- cases
def cluster_case(n, k, q, noise, seed):
    """-> (X (n, q) float32 with L2-normalised rows, labels (n,)): k orthonormal centres, rows = centre + noise randn / sqrt(q)"""
    rng = np.random.RandomState(seed)
    centres = np.linalg.qr(rng.randn(q, q))[0][:k]
    labels = rng.permutation(np.arange(n) % k)
    X = centres[labels] + noise * rng.randn(n, q) / np.sqrt(q)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32), labels


def case_scores(n, seed=None):
    """the float32 cosine block of cluster_case(n, 4, 32, 0.5, 100 + n), rounded from float64 (host tests; the GPU tests cluster the
    matrix the device itself produced)"""
    X, _ = cluster_case(n, 4, 32, 0.5, (100 + n) if seed is None else seed)
    return pairwise(X, np.array([0, n])).reshape(n, n).astype(np.float32)


def quantised_case(n, seed):
    """scores that are multiples of 1/4 in [-1, 1]: ties at every merge (and averages that tie again)"""
    rng = np.random.RandomState(seed)
    S = rng.randint(-4, 5, size=(n, n)).astype(np.float32) / 4
    S = np.triu(S, 1)
    return (S + S.T).astype(np.float32)


AHC_COUNTS = (1, 2, 33, 65, N_LDS, N_LDS + 1, 300)   # the ragged batch of the GPU test
E2E_N = (33, 65, 193, 257)
