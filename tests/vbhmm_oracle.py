"""Restatement in float64 numpy of the VB-HMM resegmentation of include/ssp.h (ssp_vbhmm_resegment), an ordinary module like
tests/diarize_oracle.py.  An extension and unpinned: the VBx source is not at hand; tests/test_vbhmm_host.py corroborates this module by
brute-force enumeration of the state paths and by the dense linear-Gaussian posterior.  Forward-backward runs in the log domain with the
DENSE transition matrix; ``forward_backward_structured`` is the O(T S) form the kernel uses, in float64."""
import numpy as np

MAX_STATES = 64
LDS_BYTES = 155648        # api.VBHMM_LDS_BYTES
ALPHA_LDS_BYTES = 65536   # api.VBHMM_ALPHA_LDS_BYTES


def padded(S):
    return 16 if S <= 16 else (32 if S <= 32 else 64)


def alpha_in_lds(S, q):
    return padded(S) * (q | 1) * 4 <= ALPHA_LDS_BYTES


def n_lds(S, q):
    """the longest recording whose two T x SP buffers sit in LDS beside alpha (api.vbhmm_n_lds)"""
    a = padded(S) * (q | 1) * 4
    return (LDS_BYTES - (a if a <= ALPHA_LDS_BYTES else 0)) // (8 * padded(S))


def lse(a, axis=None):
    a = np.asarray(a, dtype=np.float64)
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        out = np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True)) + m
    return float(out.reshape(())) if axis is None else np.squeeze(out, axis=axis)


def transition(pi, P):
    """tr[i][j] = P delta_ij + (1 - P) pi_j"""
    pi = np.asarray(pi, dtype=np.float64)
    return P * np.eye(pi.shape[0]) + (1.0 - P) * pi[None, :]


def forward_backward(ll, pi, P):
    """log domain, dense transitions.  ll (T, S) over the LIVE states, pi (S,).  -> gamma (T, S), ln p(X), lfw, lbw, ln tr"""
    ll = np.asarray(ll, dtype=np.float64)
    T, S = ll.shape
    with np.errstate(divide="ignore"):
        ltr, lpi = np.log(transition(pi, P)), np.log(np.asarray(pi, dtype=np.float64))
    lfw, lbw = np.empty((T, S)), np.zeros((T, S))
    lfw[0] = ll[0] + lpi
    for t in range(1, T):
        lfw[t] = ll[t] + lse(lfw[t - 1][:, None] + ltr, axis=0)
    for t in range(T - 2, -1, -1):
        lbw[t] = lse(ltr + (ll[t + 1] + lbw[t + 1])[None, :], axis=1)
    lnp = lse(lfw[T - 1])
    return np.exp(lfw + lbw - lnp), lnp, lfw, lbw, ltr


def pi_update(gamma, lfw, lbw, ll, lnp, pi, P):
    """pi_s proportional to gamma_0s + (1 - P) pi_s sum_{t >= 1} exp(lse_i lfw[t-1][i] + ll_ts + lbw[t][s] - ln p(X))"""
    T = ll.shape[0]
    new = gamma[0].copy()
    if T > 1:
        new += (1.0 - P) * pi * np.exp(lse(lfw[:-1], axis=1)[:, None] + ll[1:] + lbw[1:] - lnp).sum(axis=0)
    return new / new.sum()


def forward_backward_structured(ll, pi, P):
    """the O(T S) recursion in the per-step-normalised linear domain, with the pi update from the same scaled quantities
    -> gamma, ln p(X), new pi"""
    ll = np.asarray(ll, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.float64)
    T, S = ll.shape
    Q = 1.0 - P
    ah = np.empty((T, S))
    lnp = 0.0
    prev = None
    for t in range(T):
        w = pi if t == 0 else P * prev + Q * pi
        m = ll[t][w > 0].max()
        a = np.where(w > 0, np.exp(ll[t] - m) * w, 0.0)
        c = a.sum()
        prev = ah[t] = a / c
        lnp += np.log(c) + m
    gamma = np.empty((T, S))
    bh = np.ones(S)
    new = np.zeros(S)
    for t in range(T - 1, -1, -1):
        g = ah[t] * bh
        gamma[t] = g / g.sum()
        if t > 0:
            den = P * ah[t - 1] + Q * pi
            new += np.where(den > 0, gamma[t] * (Q * pi) / np.where(den > 0, den, 1.0), 0.0)
            m = ll[t][bh > 0].max()
            y = np.where(bh > 0, np.exp(ll[t] - m) * bh, 0.0)
            bt = P * y + Q * (pi * y).sum()
            bh = bt / bt.max()
        else:
            new += gamma[0]
    return gamma, lnp, new / new.sum()


def start(init_labels, S, Sr, init_smoothing):
    """-> gamma (T, S), pi (S,): the softmax over the live states of init_smoothing * onehot(label); uniform for a label out of range"""
    lab = np.asarray(init_labels).reshape(-1)
    T = lab.shape[0]
    gamma, pi = np.zeros((T, S)), np.zeros(S)
    pi[:Sr] = 1.0 / Sr
    w = np.exp(-float(init_smoothing))
    den = 1.0 + (Sr - 1) * w
    for t in range(T):
        if 0 <= lab[t] < Sr:
            gamma[t, :Sr] = w / den
            gamma[t, lab[t]] = 1.0 / den
        else:
            gamma[t, :Sr] = 1.0 / Sr
    return gamma, pi


def m_step(X, phi, gamma, Fa, Fb):
    """-> N (S,), invL (S, q), alpha (S, q)"""
    X, phi = np.asarray(X, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    rho = X * np.sqrt(phi)[None, :]
    N = gamma.sum(axis=0)
    invL = 1.0 / (1.0 + (Fa / Fb) * N[:, None] * phi[None, :])
    return N, invL, (Fa / Fb) * invL * (gamma.T @ rho)


def loglik(X, phi, invL, alpha, Fa):
    X, phi = np.asarray(X, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    rho = X * np.sqrt(phi)[None, :]
    G = -0.5 * ((X * X).sum(axis=1) + X.shape[1] * np.log(2 * np.pi))
    return Fa * (rho @ alpha.T - 0.5 * ((invL + alpha ** 2) @ phi)[None, :] + G[:, None])


def states_to_labels(gamma):
    """-> states (arg-max, ties to the lowest state), labels (rank of the state among the winners by their first row), n_speakers"""
    states = np.argmax(gamma, axis=1).astype(np.int32)
    order = []
    for s in states.tolist():
        if s not in order:
            order.append(s)
    rank = {s: i for i, s in enumerate(order)}
    return states, np.array([rank[s] for s in states.tolist()], dtype=np.int32), len(order)


def resegment(X, phi, init_labels, n_init=None, S=None, loop_prob=0.99, Fa=0.3, Fb=17.0, init_smoothing=5.0, max_iters=10, epsilon=1e-4,
              trace=False):
    """One recording.  -> dict: labels, states (T,) int32, n_speakers, n_iters, elbo (max_iters,) NaN beyond n_iters, gamma (T, S), pi (S,),
    loglik (T, S) of the last iteration (inert columns NaN here: unspecified in the contract); trace=True adds "gammas", one per iteration"""
    X = np.asarray(X, dtype=np.float64)
    T, q = X.shape
    lab = np.asarray(init_labels).reshape(-1)
    S = int(S) if S is not None else int(min(MAX_STATES, max(1, lab.max(initial=-1) + 1)))
    Sr = S if n_init is None else int(min(max(int(n_init), 1), S))
    res = {"labels": np.zeros(T, dtype=np.int32), "states": np.zeros(T, dtype=np.int32), "n_speakers": 0, "n_iters": 0,
           "elbo": np.full(max_iters, np.nan), "gamma": np.zeros((T, S)), "pi": np.zeros(S), "loglik": np.full((T, S), np.nan)}
    if T == 0:
        return res
    if not np.isfinite(X).all():
        res["labels"][:], res["states"][:], res["n_speakers"] = -1, -1, -1
        res["gamma"][:], res["pi"][:] = np.nan, np.nan
        return res
    gamma, pi = start(lab, S, Sr, init_smoothing)
    gammas = []
    for i in range(max_iters):
        N, invL, alpha = m_step(X, phi, gamma[:, :Sr], Fa, Fb)
        ll = loglik(X, phi, invL, alpha, Fa)
        g, lnp, lfw, lbw, _ = forward_backward(ll, pi[:Sr], loop_prob)
        res["elbo"][i] = lnp + 0.5 * Fb * np.sum(np.log(invL) - invL - alpha ** 2 + 1.0)
        pi = np.concatenate([pi_update(g, lfw, lbw, ll, lnp, pi[:Sr], loop_prob), np.zeros(S - Sr)])
        gamma = np.concatenate([g, np.zeros((T, S - Sr))], axis=1)
        gammas.append(gamma)
        res["n_iters"] = i + 1
        res["loglik"][:, :Sr] = ll
        if i > 0 and res["elbo"][i] - res["elbo"][i - 1] < epsilon:
            break
    res["gamma"], res["pi"] = gamma, pi
    res["states"], res["labels"], res["n_speakers"] = states_to_labels(gamma)
    if trace:
        res["gammas"] = gammas
    return res


def resegment_batch(X, counts, phi, init_labels, n_init=None, S=None, **kw):
    """the recordings of a batch -> what api.vb_resegment returns with every output asked for, as numpy arrays (float64)"""
    counts = [int(c) for c in counts]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    lab = np.asarray(init_labels).reshape(-1)
    S = int(S) if S is not None else int(min(MAX_STATES, max(1, lab.max(initial=-1) + 1)))
    mi = kw.get("max_iters", 10)
    R, total = len(counts), int(off[-1])
    out = {"labels": np.zeros(total, dtype=np.int32), "states": np.zeros(total, dtype=np.int32), "n_speakers": np.zeros(R, dtype=np.int32),
           "n_iters": np.zeros(R, dtype=np.int32), "elbo": np.full((R, mi), np.nan), "gamma": np.zeros((total, S)), "pi": np.zeros((R, S)),
           "loglik": np.full((total, S), np.nan)}
    for r in range(R):
        a, b = off[r], off[r + 1]
        if a == b:
            continue
        one = resegment(np.asarray(X)[a:b], phi, lab[a:b], None if n_init is None else n_init[r], S, **kw)
        for k in ("labels", "states", "gamma", "loglik"):
            out[k][a:b] = one[k]
        out["n_speakers"][r], out["n_iters"][r], out["elbo"][r], out["pi"][r] = one["n_speakers"], one["n_iters"], one["elbo"], one["pi"]
    return out


# -------------------------------------------------------------------------------------------------------------------------- cases
def recording_case(T, q, n_true, noise, seed, run=5, wrong=0.17, spurious=2, phi_scale=4.0):
    """A synthetic recording of the kind the projected space holds: speaker means drawn from N(0, diag(phi)), rows = mean + noise N(0, I),
    speakers in runs of ``run`` windows.  The initial labels are the true ones with a share ``wrong`` re-drawn at random among the true
    clusters and ``spurious`` extra clusters of one or two windows each.  -> X float32 (T, q), phi float32 (q,), truth (T,), init (T,) int32,
    n_init"""
    rng = np.random.RandomState(seed)
    phi = (phi_scale * np.sort(rng.gamma(2.0, 0.5, q))[::-1]).astype(np.float32)
    means = rng.randn(n_true, q) * np.sqrt(phi.astype(np.float64))[None, :]
    truth = np.zeros(T, dtype=np.int64)
    t, last = 0, -1
    while t < T:
        s = rng.randint(n_true)
        if s == last:
            s = (s + 1) % n_true
        truth[t:t + run] = s
        t, last = t + run, s
    truth[:n_true] = np.arange(n_true)   # every speaker is heard
    X = (means[truth] + noise * rng.randn(T, q)).astype(np.float32)
    init = truth.copy()
    flip = rng.rand(T) < wrong
    init[flip] = (init[flip] + 1 + rng.randint(max(1, n_true - 1), size=int(flip.sum()))) % n_true
    for k in range(spurious):
        at = rng.randint(T - 1)
        init[at:at + 1 + (k % 2)] = n_true + k
    return X, phi, truth, init.astype(np.int32), n_true + spurious


def same_partition(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    fwd, back = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(x, y) != y or back.setdefault(y, x) != x:
            return False
    return a.shape == b.shape


E2E_CASES = ((33, 32, 2, 13), (130, 64, 3, 1), (200, 130, 4, 1))    # (T, q, true speakers, seed): unit noise, S = E2E_STATES
E2E_STATES = 16
# early stopping: one batch at q = 32, T = 100, four true speakers: (noise, share of wrong labels, seed); with EARLY_EPS the float64 run stops
# in iteration 3, 5 and 4 (tests/test_vbhmm_host.py asserts the margins)
EARLY_CASES = ((1.0, 0.17, 2), (1.0, 0.17, 3), (1.0, 0.35, 6))
EARLY_EPS = 3.0


def e2e_case(i):
    T, q, k, seed = E2E_CASES[i]
    return recording_case(T, q, k, 1.0, seed)


def early_batch():
    """-> X (300, 32) float32, counts, phi, init (300,) int32, n_init (3,) int32: the recordings share phi (one model), so they are drawn
    with the first case's"""
    Xs, inits, nis, phi0 = [], [], [], None
    for noise, wrong, seed in EARLY_CASES:
        X, phi, _, init, ni = recording_case(100, 32, 4, noise, seed, wrong=wrong)
        if phi0 is None:
            phi0 = phi
        Xs.append(X)
        inits.append(init)
        nis.append(ni)
    return np.concatenate(Xs), [100] * len(EARLY_CASES), phi0, np.concatenate(inits), np.array(nis, dtype=np.int32)
