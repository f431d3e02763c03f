"""Cases, references and the one comparison rule of tests/test_dense_instances_host.py and tests/test_dense_instances_gpu.py: every kernel
behind ssp_dense_forward and ssp_dnn_forward (csrc/dense.hip dense_kernel, csrc/cosine.hip cosine_reg_kernel<NQ, true>, csrc/dnn_chain.hip
dnn_chain_kernel + dnn_pack_kernel) against float64.

  ref64   oracle.ref_cpu.dense_net_forward on the float32 inputs: float64, the truth.
  band    an array of the output's shape, derived (never fitted).  One layer, output element (n, u):
              band = 1.01 (d_in + 1) 2^-23 (sum_k |x_nk| |w_ku| + |b_u|)
          The fp32 MFMA adds the d_in exact-input products in an order nobody documents, so every accumulation is charged a whole
          2^-23 (twice the unit roundoff of round-to-nearest, as cos_band does in csrc/cosine.hip), and the bias add is one step more.
          A stack carries the band forward in float64 from E_0 = 0 along the oracle's activations h_l:
              E_{l+1} = |W_l|' E_l + 1.01 (d_l + 1) 2^-23 (|W_l|' (|h_l| + E_l) + |b_l|)
          (the kernel's layer input is within E_l of h_l; a linear map moves that by at most |W|' E_l; rounding acts on operands at
          most |h_l| + E_l large).  ReLU is 1-Lipschitz and passes E through.  An element whose band is 0 must match exactly.
          Where a pre-activation of the oracle is not finite, its E is reset to 0 and its magnitude counts as 0 in the next layer's
          band: every output it reaches is non-finite itself (the non-finite cases have no zero weight) and is compared by kind, not
          by distance, and the one way back to a finite number, ReLU of -inf, is exact.
  emu32   a float32 numpy restatement (one product and one add at a time in increasing k, or pairwise): what the host file holds
          against the band, and what its mutations break.

Input kinds, each a function of (dims, N, seed): gaussian, exact, probe (module functions of those names).  The comparison:
  gaussian   |got - ref64| <= band elementwise
  exact      got == float32(ref64) bit for bit (every partial sum is an integer below 2^24: no order of accumulation rounds)
  probe      got == W (X is the identity), or float32(w) + float32(b) in float32 with a bias
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_cpu as O  # noqa: E402

U = 2.0 ** -23
SLACK = 1.01


# ------------------------------------------------------------------------------------------------- which kernel answers
def kernel_of(d_in):
    """ssp_dense_forward's choice.  csrc/dense.hip:82 (`d_in <= 256 && !getenv("SSP_DENSE_NO_REG")`: launch_dense_reg, else
    dense_kernel) and csrc/cosine.hip:834 (nq = d_in <= 64 ? 8 : d_in <= 128 ? 16 : d_in <= 192 ? 24 : 32)."""
    if d_in > 256:
        return ("tiled",)
    return ("reg", 8 if d_in <= 64 else 16 if d_in <= 128 else 24 if d_in <= 192 else 32)


CH_W, CH_MAXL = 256, 8      # csrc/dnn_chain.hip:27, :29
DBK = 32                    # csrc/dense.hip:18: the k-slab of dense_kernel


def chain_from(dims):
    """first layer that runs inside dnn_chain_kernel (len(dims) - 1: none).  csrc/dnn_chain.hip:210-211:
    from = n_layers; while (from > 0 && dims[from - 1] <= CH_W && dims[from] <= CH_W && n_layers - (from - 1) <= CH_MAXL) --from;"""
    n_layers = len(dims) - 1
    frm = n_layers
    while frm > 0 and dims[frm - 1] <= CH_W and dims[frm] <= CH_W and n_layers - (frm - 1) <= CH_MAXL:
        frm -= 1
    return frm


def n_kc(d_in):
    """k-slabs of dense_kernel (csrc/dense.hip:36)"""
    return (d_in + DBK - 1) // DBK


def route(dims):
    """the kernels a net goes through, in order: one entry per layer in front of the chain, then ("chain", depth)"""
    frm = chain_from(dims)
    r = [kernel_of(dims[l]) for l in range(frm)]
    if frm < len(dims) - 1:
        r.append(("chain", len(dims) - 1 - frm))
    return r


INSTANCES = [("cosine_reg_kernel", 8), ("cosine_reg_kernel", 16), ("cosine_reg_kernel", 24), ("cosine_reg_kernel", 32),
             ("dense_kernel",), ("dnn_chain_kernel",), ("dnn_pack_kernel",)]


def instance_name(k):
    return "cosine_reg NQ=%d DENSE" % k[1] if k[0] == "reg" else "dense_kernel" if k[0] == "tiled" else "dnn_chain depth %d" % k[1]


# ------------------------------------------------------------------------------------------------- oracle and band
def ref64(X, layers):
    with np.errstate(invalid="ignore", over="ignore"):
        return O.dense_net_forward(np.asarray(X, dtype=np.float32), layers)


def _mag(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return np.where(np.isfinite(a), a, 0.0)


def band_of(X, layers):
    """(ref64, band), both (N, units of the last layer) float64: see the module docstring"""
    h = np.asarray(X, dtype=np.float32).astype(np.float64)
    E = np.zeros_like(h)
    with np.errstate(invalid="ignore", over="ignore"):
        for W, b, act in layers:
            W64 = np.asarray(W, dtype=np.float64)
            d = W64.shape[0]
            z = h @ W64
            if b is not None:
                z = z + np.asarray(b, dtype=np.float64)
            aW = _mag(W64)
            mag = (_mag(h) + E) @ aW + (0.0 if b is None else _mag(b))
            Ez = E @ aW + SLACK * (d + 1) * U * mag
            E = np.where(np.isfinite(z), Ez, 0.0)
            h = np.maximum(z, 0.0) if act == "relu" else z
    ref = ref64(X, layers)
    assert np.array_equal(ref, h, equal_nan=True), "band_of walks another forward pass than the oracle"
    return ref, E


def ratio_of(got, ref, band):
    """the largest |got - ref| / band over the finite reference entries (0 / 0 = 0, x / 0 = inf)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref)[fin]
        bd = band[fin]
        r = np.where(err == 0.0, 0.0, err / bd)
    r = np.where(np.isnan(r), np.inf, r)          # a non-finite answer where the reference is finite
    return float(r.max())


def same_kind(got, ref):
    """isnan, isposinf and isneginf of got are those of ref"""
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
            and np.array_equal(np.isneginf(got), np.isneginf(ref)))


# ------------------------------------------------------------------------------------------------- float32 restatement
def _dot32(X, W, order, skip_slab=None):
    """float32 X @ W, one product and one add at a time.  order "strict": increasing k; "pairwise": halves down to runs of 8.
    skip_slab: the 32 columns of that k-slab are left out (a mutation)."""
    X, W = np.asarray(X, dtype=np.float32), np.asarray(W, dtype=np.float32)

    def run(lo, hi):
        acc = np.zeros((X.shape[0], W.shape[1]), np.float32)
        for k in range(lo, hi):
            if skip_slab is not None and k // DBK == skip_slab:
                continue
            acc = acc + X[:, k:k + 1] * W[k][None, :]
        return acc

    def pair(lo, hi):
        if hi - lo <= 8:
            return run(lo, hi)
        mid = (lo + hi) // 2
        return pair(lo, mid) + pair(mid, hi)

    out = run(0, X.shape[1]) if order == "strict" else pair(0, X.shape[1])
    assert out.dtype == np.float32
    return out


MUTATIONS = ("drop_last_column", "drop_last_bias", "skip_slab", "relu_on_last")


def emu32(X, layers, order="strict", mutate=None):
    """the forward pass in float32 numpy.  mutate: one of MUTATIONS, applied to the first layer that has what it breaks"""
    h = np.asarray(X, dtype=np.float32)
    L = len(layers)
    with np.errstate(invalid="ignore", over="ignore"):
        for l, (W, b, act) in enumerate(layers):
            W = np.asarray(W, dtype=np.float32)
            hin = h
            if mutate == "drop_last_column" and l == 0:
                hin = h.copy()
                hin[:, -1] = 0.0
            z = _dot32(hin, W, order, skip_slab=0 if (mutate == "skip_slab" and l == 0) else None)
            if b is not None:
                bb = np.asarray(b, dtype=np.float32).copy()
                if mutate == "drop_last_bias" and l == L - 1:
                    bb[-1] = 0.0
                z = z + bb[None, :]
            if act == "relu" or (mutate == "relu_on_last" and l == L - 1):
                z = np.where(z < 0, np.float32(0.0), z)       # (keeps a NaN, as np.maximum does)
            h = z.astype(np.float32)
    return h


# ------------------------------------------------------------------------------------------------- input kinds
def acts_of(pattern, L):
    """ReLU patterns: "ref" the reference network's (every layer but the last), "none", "last" (the last layer only), "all" """
    return [("relu" if (pattern == "all" or (pattern == "ref" and l + 1 < L) or (pattern == "last" and l + 1 == L)) else "linear")
            for l in range(L)]


def _seed(dims, N, salt):
    return [salt, N] + list(dims)


def gaussian(dims, N, bias=True, relu="ref", seed=0):
    """X ~ N(0, 1), W ~ N(0, 1) / sqrt(d_in), b ~ N(0, 1); the last input column, the last unit of every layer and the last sample are
    each scaled by 8: an error at an edge is the largest in the array"""
    rng = np.random.default_rng(_seed(dims, N, 1000 + seed))
    X = rng.standard_normal((N, dims[0]))
    if N:
        X[:, -1] *= 8
        X[-1, :] *= 8
    L = len(dims) - 1
    layers = []
    for l, act in enumerate(acts_of(relu, L)):
        W = rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])
        W[:, -1] *= 8
        b = rng.standard_normal(dims[l + 1])
        layers.append((W.astype(np.float32), b.astype(np.float32) if bias else None, act))
    return dict(kind="gaussian", dims=list(dims), N=N, X=X.astype(np.float32), layers=layers)


def exact(dims, N, bias=True, relu="ref", seed=0):
    """small signed integers, every partial sum of every layer an integer below 2^24 (exact_bound proves it): the first layer has entries
    in [-3, 3], every later layer at most two weights of +-1 per unit; biases in [-8, 8]; X in [-3, 3].  Input column d_in - 1, unit 0
    and unit units - 1 of every layer carry a non-zero weight, and the last column of the last sample is non-zero."""
    rng = np.random.default_rng(_seed(dims, N, 2000 + seed))
    X = rng.integers(-3, 4, (N, dims[0]))
    if N:
        X[-1, -1] = 3
    L = len(dims) - 1
    layers = []
    for l, act in enumerate(acts_of(relu, L)):
        d, u = dims[l], dims[l + 1]
        if l == 0:
            W = rng.integers(-3, 4, (d, u))
            W[d - 1] = np.where(W[d - 1] == 0, 2, W[d - 1])        # column d_in - 1 reaches every unit, units 0 and units - 1 among them
        else:
            W = np.zeros((d, u), np.int64)
            ka, kb = rng.integers(0, d, u), rng.integers(0, d, u)
            ka[u - 1] = d - 1
            W[kb, np.arange(u)] = rng.choice([-1, 1], u)
            W[ka, np.arange(u)] = rng.choice([-1, 1], u)           # (ka == kb: one weight)
        b = rng.integers(-8, 9, u)
        layers.append((W.astype(np.float32), b.astype(np.float32) if bias else None, act))
    return dict(kind="exact", dims=list(dims), N=N, X=X.astype(np.float32), layers=layers)


def exact_bound(c):
    """int64: the largest sum of magnitudes any output of any layer can reach, whatever the order of accumulation"""
    h = np.abs(c["X"]).astype(np.int64)
    worst = 0
    for W, b, _ in c["layers"]:
        assert np.array_equal(W, np.rint(W)) and (b is None or np.array_equal(b, np.rint(b)))
        h = h @ np.abs(W).astype(np.int64) + (0 if b is None else np.abs(b).astype(np.int64))
        worst = max(worst, int(h.max()) if h.size else 0)
    return worst


def probe(d_in, units, bias=False, relu=False, seed=0):
    """N = d_in, X the identity: Y reads every weight position of the operand image once.  -> the case and the expected bits"""
    rng = np.random.default_rng(_seed([d_in, units], d_in, 3000 + seed))
    W = rng.standard_normal((d_in, units)).astype(np.float32)
    W[np.abs(W) < np.finfo(np.float32).tiny] = 1.0                 # no subnormals (and no zeros)
    b = rng.standard_normal(units).astype(np.float32) if bias else None
    want = W.copy() if b is None else (W + b[None, :])
    assert want.dtype == np.float32
    if relu:
        want = np.where(want < 0, np.float32(0.0), want)
    c = dict(kind="probe", dims=[d_in, units], N=d_in, X=np.eye(d_in, dtype=np.float32), layers=[(W, b, "relu" if relu else "linear")])
    return c, want


# ------------------------------------------------------------------------------------------------- the non-finite table
def partial_column(d):
    """a column inside the last partial group of four (d % 4 != 0), else inside the last whole group"""
    return 4 * (d // 4) if d % 4 else max(d - 3, 0)


def integer_net(dims, N, relu="ref", seed=0):
    """a gaussian batch through integer weights WITHOUT zeros (magnitudes 1..3, biases in [-8, 8]): the oracle has no 0 * inf of its own
    and nothing overflows.  In a net of several layers sign(W_l[k, u]) = c_{l-1}[k] c_l[u]: what one +-inf input sends into a unit of
    a later layer then has one sign, so the oracle carries +-inf (not inf - inf) to the output."""
    rng = np.random.default_rng(_seed(dims, N, 4000 + seed))
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    L = len(dims) - 1
    layers = []
    c_prev = rng.choice([-1, 1], dims[0])
    for l, act in enumerate(acts_of(relu, L)):
        d, u = dims[l], dims[l + 1]
        mag = rng.integers(1, 4, (d, u))
        if L == 1:
            W = mag * rng.choice([-1, 1], (d, u))
        else:
            c = rng.choice([-1, 1], u)
            W = mag * c_prev[:, None] * c[None, :]
            c_prev = c
        b = rng.integers(-8, 9, u)
        layers.append((W.astype(np.float32), b.astype(np.float32), act))
    return dict(kind="integer", dims=list(dims), N=N, X=X, layers=layers)


NONFINITE_VALUES = (("nan", np.nan), ("posinf", np.inf), ("neginf", -np.inf))


def nonfinite_table(dims, N, relu="ref", seed=0):
    """-> (clean case, [entry]).  entry: dict(name, X, layers, sample): sample is the poisoned row of X (every other row must come out with
    the clean call's bits), or None where a weight or a bias entry carries the NaN."""
    c = integer_net(dims, N, relu=relu, seed=seed)
    d = dims[0]
    cols = []
    for col in (0, d - 1, partial_column(d)):
        if col not in cols:
            cols.append(col)
    samples = (N // 2, N - 1, 0)
    out = []
    for i, col in enumerate(cols):
        for vn, v in NONFINITE_VALUES:
            X = c["X"].copy()
            X[samples[i % 3], col] = v
            out.append(dict(name="x[%d,%d]=%s" % (samples[i % 3], col, vn), X=X, layers=c["layers"], sample=samples[i % 3], value=vn))
    L = len(c["layers"])

    def with_nan(l, what):
        layers = [(W.copy(), b.copy(), a) for W, b, a in c["layers"]]
        if what == "w":
            layers[l][0][layers[l][0].shape[0] - 1, layers[l][0].shape[1] // 2] = np.nan
        else:
            layers[l][1][layers[l][1].shape[0] - 1] = np.nan
        return layers
    out.append(dict(name="w[last layer]=nan", X=c["X"], layers=with_nan(L - 1, "w"), sample=None, value="nan"))
    out.append(dict(name="b[last layer]=nan", X=c["X"], layers=with_nan(L - 1, "b"), sample=None, value="nan"))
    if L > 1:
        out.append(dict(name="b[layer 0]=nan", X=c["X"], layers=with_nan(0, "b"), sample=None, value="nan"))
    return c, out


NONFINITE_LAYERS = ((50, 12), (130, 36), (259, 130))                      # reg NQ = 8, reg NQ = 24, tiled
NONFINITE_NETS = (([5, 17, 15, 16, 3], "none"), ([40, 32, 16], "ref"), ([300, 256, 200, 7], "ref"))
NONFINITE_N = 70


# ------------------------------------------------------------------------------------------------- the shape tables
REG_D = {8: (1, 2, 3, 5, 63, 64), 16: (65, 127, 128), 24: (129, 190, 191, 192), 32: (193, 253, 254, 255, 256)}
REG_UNITS = (1, 3, 4, 31, 32, 33, 36, 255, 256, 257, 260)
REG_N = (1, 31, 32, 33, 127, 128, 129, 257)
TILED_D = (257, 258, 259, 260, 287, 288, 289, 320, 321, 1274)
TILED_UNITS = (1, 3, 4, 127, 128, 129, 130, 132, 256, 257, 260)
TILED_N = (1, 127, 128, 129, 300)
NOREG_D = (1, 31, 32, 33, 64, 65, 96, 97, 256)                             # n_kc = 1, 1, 1, 2, 2, 3, 3, 4, 8 under SSP_DENSE_NO_REG
COMBOS = ((True, True), (False, False), (True, False), (False, True))      # (bias, relu)


def reg_shapes(nq):
    """(d_in, units, N): every d_in of the instance with every units at N = 33 and 129 and every N at units = 36 and 257"""
    out = []
    for d in REG_D[nq]:
        assert kernel_of(d) == ("reg", nq)
        for u in REG_UNITS:
            out += [(d, u, 33), (d, u, 129)]
        for n in REG_N:
            out += [(d, 36, n), (d, 257, n)]
    return sorted(set(out))


def tiled_shapes():
    """every d_in at two units / N pairs; every units and every N at d_in 257 and 289"""
    out = []
    for d in TILED_D:
        assert kernel_of(d) == ("tiled",)
        out += [(d, 130, 129), (d, 257, 300)]
    for d in (257, 289):
        for u in TILED_UNITS:
            out += [(d, u, 129), (d, u, 1)]
        for n in TILED_N:
            out += [(d, 132, n), (d, 3, n), (d, 260, n)]
    # units other than 256 with N across the 128-sample workgroup, units not a multiple of 4 above 128
    out += [(260, u, n) for u in (130, 257) for n in (127, 128, 129)]
    return sorted(set(out))


def noreg_shapes():
    return [(d, u, n) for d in NOREG_D for (u, n) in ((130, 129), (3, 1), (36, 33))]


NETS = ([1, 1], [3, 1, 7], [5, 17, 15, 16, 3], [255, 256, 255, 4], [256, 200, 256, 252], [40] + [24] * 8, [40] + [24] * 9,
        [10, 300, 20, 8], [256, 257, 256], [1274, 256, 256, 256, 256])
NET_N = (1, 15, 16, 17, 63, 64, 65, 129)
NET_RELU = ("ref", "none", "last")
CHAIN_PROBES = ((200, 256), (256, 7))


def net_relu(dims, i):
    """[5, 17, 15, 16, 3] has every hidden layer linear in every pattern but "last"; the others rotate through NET_RELU"""
    if list(dims) == [5, 17, 15, 16, 3]:
        return ("none", "last")[i % 2]
    return NET_RELU[i % 3]


def net_cases(dims):
    """the (kind, N, bias, relu pattern) list of one net: every N of NET_N once per kind, the ReLU patterns rotating, every bias None at
    one N per kind"""
    out = []
    for i, n in enumerate(NET_N):
        out.append(("gaussian", n, i != 3, net_relu(dims, i)))
        out.append(("exact", n, i != 5, net_relu(dims, i + 1)))
    return out


def make(kind, dims, N, bias, relu):
    return (gaussian if kind == "gaussian" else exact)(dims, N, bias=bias, relu=relu)


def layer_case(kind, d, u, n, bias, relu):
    return make(kind, [d, u], n, bias, "all" if relu else "none")
