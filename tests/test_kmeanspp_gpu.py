"""k-means++ seeding on the GPU (ssp_kmeanspp_seed, api.kmeanspp_seeds, GaussianMixture(seeding='device')): the picks are exactly those of
a float64 numpy restatement of the algorithm (below), whatever the launch's other problems; seeding='device' gives the seeds of
seeding='host' and leaves a RandomState where the host seeding leaves it.

Why exact equality is a fair demand.  ``restate`` also returns the two margins of a run: how close (relative to the total) a threshold
u * total ever comes to an entry of the prefix sum, and the relative gap between the best potential and the best potential of a DIFFERENT
row.  Float64 sums of ~3e4 non-negative terms in any order agree to ~1e-12 relative, so with both margins >= 1e-10 — asserted for every
case of the table, as a condition on the inputs — no summation order can change a pick."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# n, K, D, seed: wave and workgroup boundaries, the subsample cap (20000 of 20001; 25600 of 26000), L = 2, 4, 6 and 8, K = 1 with no step
CASES = [(1, 1, 5, 0), (2, 2, 1, 1), (8, 8, 7, 2), (63, 5, 7, 3), (64, 16, 26, 4), (65, 16, 39, 5), (1023, 8, 47, 6), (1024, 64, 39, 7),
         (1025, 64, 60, 8), (2500, 64, 39, 9), (4097, 16, 13, 10), (20001, 64, 39, 11), (26000, 512, 13, 12)]
MARGIN = 1e-10


def case_data(n, D, seed):
    rng = np.random.default_rng(seed)
    return (1.5 * rng.standard_normal((n, D)) + rng.standard_normal(D)).astype(np.float32)


def restate(X32, first, u):
    """The algorithm of ssp_kmeanspp_seed in float64 numpy on the float32 rows X32: picks (K,) as positions among the rows, and the two
    margins of the run (inf where a step has nothing to decide)."""
    X = np.asarray(X32, dtype=np.float64)
    n = X.shape[0]
    u = np.asarray(u, dtype=np.float64)
    picks = [int(first)]
    d2 = ((X - X[first]) ** 2).sum(1)
    cum_margin = pot_margin = np.inf
    for k in range(1, u.shape[0] + 1):
        cum = np.cumsum(d2)
        total = cum[-1]
        v = u[k - 1] * total
        cand = np.minimum(np.searchsorted(cum, v, side='left'), n - 1)
        if total > 0:
            cum_margin = min(cum_margin, min(float(np.abs(cum - t).min()) for t in v) / total)
        dc = np.stack([((X - X[c]) ** 2).sum(1) for c in cand], axis=1)
        pot = np.minimum(d2[:, None], dc).sum(0)
        b = int(np.argmin(pot))
        other = pot[cand != cand[b]]
        if other.size:
            o = float(other.min())
            pot_margin = min(pot_margin, (o - pot[b]) / o if o > 0 else 0.0)
        picks.append(int(cand[b]))
        d2 = np.minimum(d2, dc[:, b])
    return np.array(picks, dtype=np.int64), cum_margin, pot_margin


@functools.lru_cache(maxsize=None)
def case_reference(i):
    """case i of the table, computed once: (X, idx, first, u, absolute rows picked by the restatement, cum margin, potential margin).
    The draws are those of RandomState(seed) through gmm_train._kmeanspp_draws."""
    from speech_signal_processing_amd.gmm_train import _kmeanspp_draws
    n, K, D, seed = CASES[i]
    X = case_data(n, D, seed)
    idx, first, u = _kmeanspp_draws(np.random.RandomState(seed), n, K)
    picks, cm, pm = restate(X[idx], first, u)
    for a in (X, idx, u):
        a.setflags(write=False)
    return X, idx, first, u, idx[picks], cm, pm


@pytest.fixture(scope="module")
def env():
    from speech_signal_processing_amd import api
    return api, api.default_context()


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:%d" % ctx.device)  # (a copy: the shared references are read-only)


@pytest.mark.parametrize("i", range(len(CASES)), ids=["n%d-K%d-D%d" % c[:3] for c in CASES])
def test_picks_equal_the_restatement(env, i):
    api, ctx = env
    n, K, D, seed = CASES[i]
    X, idx, first, u, want, cm, pm = case_reference(i)
    print("case", CASES[i], "cum margin %.3g" % cm, "potential margin %.3g" % pm)
    assert cm >= MARGIN and pm >= MARGIN, "badly chosen input: a pick of this case hangs on the summation order"
    sel = idx if len(idx) < n else None
    r = api.kmeanspp_seeds(ctx, X, K, [first], u[None], sel=sel)
    print("picked", r["rows"][0][:8], "want", want[:8])
    assert r["rows"].dtype == np.int64 and r["rows"].shape == (1, K)
    assert np.array_equal(r["rows"][0], want)
    assert r["centres"].dtype == np.float64 and np.array_equal(r["centres"][0], X[want].astype(np.float64))
    # the same bits again, from a device tensor, and without the centres
    r2 = api.kmeanspp_seeds(ctx, _dev(ctx, X), K, [first], u[None], sel=sel, centres=False, timing=True)
    assert np.array_equal(r2["rows"], r["rows"]) and "centres" not in r2 and r2["kernel_ms"] >= 0.0


def _layout(rng, lens, gap=37):
    """rows of the problems placed out of order, with gaps: (n_rows, row_off)"""
    order = rng.permutation(len(lens))
    off = np.zeros(len(lens), np.int64)
    pos = 11
    for m in order:
        off[m] = pos
        pos += lens[m] + gap
    return pos + 5, off


@pytest.mark.parametrize("K,D", [(16, 39), (64, 47)])
def test_thirteen_problems_in_one_call(env, K, D):
    """One call has one K and one D, so the 13 problems take the table's row counts and seeds at a common (K, D).  Rows out of order with
    gaps; once as ranges and once as lists (given in another order than the ranges lie); host and device feats.  Every problem's picks
    and centres are those of its own single-problem call on a copy of its rows."""
    api, ctx = env
    rng = np.random.default_rng(100 + K)
    lens = np.array([c[0] for c in CASES], dtype=np.int64)
    P = len(lens)
    n_rows, off = _layout(rng, lens)
    X = np.full((n_rows, D), np.nan, dtype=np.float32)  # (a gap row that is read shows)
    L = api.kmeanspp_candidates(K)
    first = np.zeros(P, dtype=np.int64)
    u = np.empty((P, K - 1, L))
    single = []
    for p, (n, _K, _D, seed) in enumerate(CASES):
        X[off[p]:off[p] + n] = case_data(n, D, seed)
        rs = np.random.RandomState(seed)
        first[p] = rs.randint(n)
        u[p] = rs.uniform(size=(K - 1, L))
        single.append(api.kmeanspp_seeds(ctx, X[off[p]:off[p] + n].copy(), K, [first[p]], u[p][None]))
    sel = np.concatenate([off[p] + np.arange(lens[p]) for p in range(P)])
    sel_off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    for feats in (X, _dev(ctx, X)):
        for kw in (dict(row_off=off, n_sel=lens), dict(row_off=sel_off, n_sel=lens, sel=sel)):
            r = api.kmeanspp_seeds(ctx, feats, K, first, u, **kw)
            for p in range(P):
                assert np.array_equal(r["rows"][p], single[p]["rows"][0] + off[p]), (p, sorted(kw))
                assert np.array_equal(r["centres"][p], single[p]["centres"][0]), (p, sorted(kw))


def test_hand_made_draws(env):
    api, ctx = env
    X = case_data(300, 9, 40)
    n = len(X)
    top = 1.0 - 2.0 ** -53
    # u = 0: position 0
    r = api.kmeanspp_seeds(ctx, X, 2, [17], np.zeros((1, 1, 2)))
    assert r["rows"].tolist() == [[17, 0]]
    # u = 1 - 2^-53: the last row with d2 > 0 — n - 1; n - 2 when the last row is the first centre; before a tail of copies of it
    r = api.kmeanspp_seeds(ctx, X, 2, [0], np.full((1, 1, 2), top))
    assert r["rows"].tolist() == [[0, n - 1]]
    r = api.kmeanspp_seeds(ctx, X, 2, [n - 1], np.full((1, 1, 2), top))
    assert r["rows"].tolist() == [[n - 1, n - 2]]
    Y = X.copy()
    Y[-3:] = Y[5]
    r = api.kmeanspp_seeds(ctx, Y, 2, [5], np.full((1, 1, 2), top))
    assert r["rows"].tolist() == [[5, n - 4]]
    # all rows identical: total == 0, every pick is position 0, no error
    Z = np.tile(X[3], (100, 1))
    r = api.kmeanspp_seeds(ctx, Z, 4, [5], np.random.default_rng(0).uniform(size=(1, 3, 3)))
    assert r["rows"].tolist() == [[5, 0, 0, 0]] and np.array_equal(r["centres"][0], np.tile(X[3].astype(np.float64), (4, 1)))
    # two candidates on the same row
    r = api.kmeanspp_seeds(ctx, X, 2, [17], np.full((1, 1, 2), 0.3))
    assert np.array_equal(r["rows"][0], restate(X, 17, np.full((1, 2), 0.3))[0])
    # two candidates on two copies of one row: equal potentials, the FIRST arg-min wins though it names the later row
    W = X.copy()
    W[200] = W[100]
    d2 = ((W.astype(np.float64) - W[17].astype(np.float64)) ** 2).sum(1)
    cum = np.cumsum(d2)
    hit = lambda i: (cum[i - 1] + 0.5 * d2[i]) / cum[-1]
    for a, b in ((200, 100), (100, 200)):
        r = api.kmeanspp_seeds(ctx, W, 2, [17], np.array([[[hit(a), hit(b)]]]))
        assert r["rows"].tolist() == [[17, a]]
    # duplicate rows: plateaus in cum, and ties between copies
    rng = np.random.default_rng(41)
    V = case_data(150, 9, 42)[rng.integers(0, 150, size=700)]
    first, u = 33, rng.uniform(size=(11, 4))
    r = api.kmeanspp_seeds(ctx, V, 12, [first], u[None])
    assert np.array_equal(r["rows"][0], restate(V, first, u)[0])
    # a list that really skips rows = the call on the gathered rows
    idx = np.sort(rng.choice(700, size=333, replace=False))
    r = api.kmeanspp_seeds(ctx, V, 12, [first], u[None], sel=idx)
    g = api.kmeanspp_seeds(ctx, V[idx], 12, [first], u[None])
    assert np.array_equal(r["rows"][0], idx[g["rows"][0]]) and np.array_equal(r["centres"], g["centres"])


def test_errors(env):
    api, ctx = env
    X = case_data(200, 7, 50)
    u = np.random.default_rng(1).uniform(size=(2, 3, 3))
    off, cnt = np.array([0, 100]), np.array([100, 100])
    ok = api.kmeanspp_seeds(ctx, X, 4, [3, 4], u, row_off=off, n_sel=cnt)
    with pytest.raises(ValueError, match="problem 1.*first"):
        api.kmeanspp_seeds(ctx, X, 4, [3, 100], u, row_off=off, n_sel=cnt)
    with pytest.raises(ValueError, match="problem 0.*first"):
        api.kmeanspp_seeds(ctx, X, 4, [-1, 4], u, row_off=off, n_sel=cnt)
    bad = u.copy()
    bad[1, 2, 0] = 1.0
    with pytest.raises(ValueError, match="problem 1.*draw"):
        api.kmeanspp_seeds(ctx, X, 4, [3, 4], bad, row_off=off, n_sel=cnt)
    with pytest.raises(ValueError, match="problem 1.*outside"):
        api.kmeanspp_seeds(ctx, X, 4, [3, 4], u, row_off=np.array([0, 101]), n_sel=cnt)
    with pytest.raises(ValueError, match="problem 0.*outside"):
        api.kmeanspp_seeds(ctx, X, 4, [3, 4], u, row_off=np.array([0, 5]), n_sel=np.array([5, 5]), sel=np.array([0, 1, 2, 3, 200, 5, 6, 7, 8, 9]))
    with pytest.raises(ValueError, match="problem 1 has no rows"):
        api.kmeanspp_seeds(ctx, X, 4, [3, 0], u, row_off=off, n_sel=np.array([100, 0]))
    with pytest.raises(NotImplementedError, match="D=65"):
        api.kmeanspp_seeds(ctx, np.zeros((10, 65), np.float32), 4, [3], u[:1])
    # a NaN row: the problem that holds it is named, and nothing stays behind
    Y = X.copy()
    Y[150, 2] = np.nan
    with pytest.raises(ValueError, match="problem 1.*not finite"):
        api.kmeanspp_seeds(ctx, Y, 4, [3, 4], u, row_off=off, n_sel=cnt)
    again = api.kmeanspp_seeds(ctx, X, 4, [3, 4], u, row_off=off, n_sel=cnt)
    assert np.array_equal(again["rows"], ok["rows"]) and np.array_equal(again["centres"], ok["centres"])


@pytest.mark.parametrize("i", [9, 11], ids=["n2500", "n20001"])
def test_device_seeding_gives_the_host_seeds(env, i):
    api, ctx = env
    from speech_signal_processing_amd.gmm_train import GaussianMixture
    n, K, D, seed = CASES[i]
    X = case_reference(i)[0]
    rs_h, rs_d = np.random.RandomState(seed), np.random.RandomState(seed)
    host = GaussianMixture(n_components=K, random_state=rs_h)._kmeanspp(X, n, D, rs_h)
    dev = GaussianMixture(n_components=K, random_state=rs_d, seeding='device')._seeds(ctx, _dev(ctx, X), n, D, rs_d)
    assert np.array_equal(host, dev)
    sh, sd = rs_h.get_state(), rs_d.get_state()
    assert np.array_equal(sh[1], sd[1]) and sh[2:] == sd[2:]


def test_fit_many_device_seeding(env):
    from speech_signal_processing_amd.gmm_train import GaussianMixture, fit_many
    rng = np.random.default_rng(60)
    Xs = [(1.5 * rng.standard_normal((n, 13)) + rng.standard_normal(13) + 3.0 * rng.integers(0, 3, size=(n, 1))).astype(np.float32)
          for n in (300, 517, 640, 900)]
    prof = {}
    many = fit_many(Xs, n_components=8, seeding='device', random_state=3, profile=prof)
    assert prof["kmeanspp_kernel_ms"] > 0.0 and prof["kmeanspp_s"] > 0.0
    host = fit_many(Xs, n_components=8, seeding='host', random_state=3)
    for X, a, h in zip(Xs, many, host):
        one = GaussianMixture(n_components=8, seeding='device', random_state=3).fit(X)
        for name in ("weights_", "means_", "covariances_", "lower_bound_", "n_iter_", "converged_"):
            assert np.array_equal(getattr(a, name), getattr(one, name)), name
            assert np.array_equal(getattr(a, name), getattr(h, name)), name
