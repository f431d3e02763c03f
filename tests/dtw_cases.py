"""Cases, references and the derived bound of tests/test_dtw_instances_host.py, tests/test_dtw_instances_isa.py and
tests/test_dtw_instances_gpu.py: every compiled instance of the all-pairs DTW matcher (csrc/dtw.hip: dtw1_kernel<W> for dim == 1,
dtw_kernel<W, float, false> for dim > 1) against float64, with a template on each edge of the instance's range.  An ordinary module like
tests/gmm_cases.py and tests/cosine_cases.py.

Evaluations of one (query, template) pair:
  ref64   oracle.ref_cpu.dtw_distance on the float32 inputs: float64, the truth (NaN and infinities propagate as numpy's do).
  emu32   the same recurrence in float32 numpy, one rounding per operation, swept by anti-diagonals like the oracle: at dim 1 the cost is
          |float32(x_i - y_j)|, at dim > 1 a float32 sum of squares in coordinate order and a float32 square root.  dtw1_kernel's cell is
          a subtract, an absolute value, a three-way minimum and an add — nothing the compiler may contract or reorder without fast-math —
          so at dim 1 the library equals emu32 BIT FOR BIT.  At dim > 1 the sum of squares may be fused; there the band decides.
  got     the library.

The band (no measured number enters it).  u = 2^-24.  Every rounding on a warping path multiplies its term by at most (1 + u); a path has
at most r + c - 1 cells with one add each; a cost carries one rounding at dim 1 (the subtract; |.| is exact) and at most (dim + 5) / 2
at dim > 1 (a term (x - y)^2 carries 3 roundings and up to dim roundings of the running sum, the square root halves their relative sum
and adds one of its own: (dim + 3) / 2 + 1).  So every path's float32 sum lies within (r + c - 1 + k') u / (1 - n u) of its exact sum,
relatively, and the minimum over paths of perturbed sums moves by no more than the largest perturbation:
  |got - ref64| <= 1.01 (r + c + k) 2^-24 ref64,     k = 1 at dim 1, k = dim + 3 at dim > 1
with 1.01 for the 1 / (1 - n u) denominator at every n used here (n u < 2^-10) and the rounding of ref64 itself.

Exact inputs.  Dim 1: integers in [-8, 8]; every cost and partial sum is an integer below 2^24, float32 computes it exactly.  Dim > 1: rows
a_i (3, 4, 0, ...) with integer a_i in [-8, 8]: the sum of squares is the integer 25 (a_i - b_j)^2, its correctly rounded root 5 |a_i - b_j|.
On these got == float32(ref64) bit for bit for every instance, fused or not.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_cpu as O  # noqa: E402

U32 = 2.0 ** -24

# ---- the instance table of csrc/dtw.hip (ssp_dtw_distances), restated: W columns per lane, 64 W columns per super-block
W_DIM1 = (4, 8, 12, 16, 20, 24, 32)
W_DIMN = (4, 8, 16, 32)
INSTANCES = [("dtw1_kernel", w) for w in W_DIM1] + [("dtw_kernel", w) for w in W_DIMN]
QUERY_LENS = (1, 2, 63, 64, 65, 130)                     # fewer rows than lanes, exactly as many, more
BLOCK_TEMPLATES = (2048, 2049, 2081, 4096, 4097, 6145)   # W = 32: one full block .. four blocks, the last of one column
BLOCK_QUERIES = (1, 3, 64, 70)


def widths(dim):
    return W_DIM1 if dim == 1 else W_DIMN


def pick_w(dim, max_c):
    """the W the host picks from the longest template of the call"""
    need = (int(max_c) + 63) // 64
    for w in widths(dim):
        if need <= w:
            return w
    return 32


def lo_of(dim, w):
    """the shortest longest-template that selects W"""
    ws = widths(dim)
    k = ws.index(w)
    return 1 if k == 0 else 64 * ws[k - 1] + 1


def kernel_of(dim):
    return "dtw1_kernel" if dim == 1 else "dtw_kernel"


def instance_name(dim, w):
    return "dtw1_kernel<%d>" % w if dim == 1 else "dtw_kernel<%d, float, false>" % w


def template_lens(dim, w):
    """the sweep's template lengths; 64 W last, so that it is the call's longest"""
    return [1, w - 1, w, w + 1, 65, lo_of(dim, w), 64 * w - 1, 64 * w]


def low_edge_templates(dim, w):
    """indices into template_lens of the second call: without the last two, and nothing longer than lo, so that lo itself selects W"""
    lens, lo = template_lens(dim, w), lo_of(dim, w)
    return [k for k, n in enumerate(lens[:-2]) if n <= lo]


# ------------------------------------------------------------------------------------------------- references
def ref64(x, y, normalize=False):
    with np.errstate(all="ignore"):
        return float(O.dtw_distance(np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32), normalize))


def _rows(a):
    a = np.asarray(a, dtype=np.float32)
    return a.reshape(-1, 1) if a.ndim == 1 else a


def cost32(x, y):
    """(r, c) float32 local costs, one rounding per operation"""
    x, y = _rows(x), _rows(y)
    with np.errstate(all="ignore"):
        if x.shape[1] == 1:
            return np.abs(x - y.T)
        ss = np.zeros((x.shape[0], y.shape[0]), np.float32)
        for e in range(x.shape[1]):
            df = x[:, e][:, None] - y[:, e][None, :]
            ss = ss + df * df
        return np.sqrt(ss)


def cost64(x, y):
    """(r, c) float64 local costs, the oracle's expression"""
    x, y = _rows(x).astype(np.float64), _rows(y).astype(np.float64)
    with np.errstate(all="ignore"):
        if x.shape[1] == 1:
            return np.abs(x - y.T)
        return np.sqrt(np.maximum(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1), 0.0))


def sweep(costs, dtype):
    """the recurrence over a batch of cost matrices, by anti-diagonals like the oracle, one operation of `dtype` per step.  The matrices
    are padded to one shape with zeros: a cell depends on cells of smaller or equal row and column only, so the padding reaches no cell of
    the pair itself.  -> the list of D[r - 1][c - 1]"""
    B = len(costs)
    R, Cc = max(c.shape[0] for c in costs), max(c.shape[1] for c in costs)
    cost = np.zeros((B, R, Cc), dtype)
    for b, c in enumerate(costs):
        cost[b, :c.shape[0], :c.shape[1]] = c
    D = np.full((B, R + 1, Cc + 1), np.inf, dtype)
    D[:, 0, 0] = 0
    with np.errstate(all="ignore"):
        for k in range(R + Cc - 1):
            i = np.arange(max(0, k - Cc + 1), min(R, k + 1))
            j = k - i
            D[:, i + 1, j + 1] = cost[:, i, j] + np.minimum(D[:, i, j], np.minimum(D[:, i, j + 1], D[:, i + 1, j]))
    assert D.dtype == dtype
    return [D[b, c.shape[0], c.shape[1]] for b, c in enumerate(costs)]


def emu32(x, y):
    return np.float32(sweep([cost32(x, y)], np.float32)[0])


def ref64_matrix(Q, T):
    """(n_q, n_t) float64: ref64 of every pair, the templates of a query swept together (bit-equal to ref64, tests/test_dtw_instances_host.py)"""
    return np.array([sweep([cost64(q, t) for t in T], np.float64) for q in Q], dtype=np.float64)


def emu32_matrix(Q, T):
    return np.array([sweep([cost32(q, t) for t in T], np.float32) for q in Q], dtype=np.float32)


def band(r, c, dim, ref):
    k = 1 if dim == 1 else dim + 3
    return 1.01 * (r + c + k) * U32 * np.abs(ref)


def band_matrix(Q, T, ref):
    dim = _rows(Q[0]).shape[1]
    return np.array([[band(len(q), len(t), dim, ref[a, b]) for b, t in enumerate(T)] for a, q in enumerate(Q)])


def ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


# ------------------------------------------------------------------------------------------------- inputs
def gaussian(n, dim, seed):
    rng = np.random.default_rng([0xd7, seed, n, dim])
    return (rng.standard_normal(n) if dim == 1 else rng.standard_normal((n, dim))).astype(np.float32)


def exact(n, dim, seed):
    rng = np.random.default_rng([0xe8, seed, n, dim])
    a = rng.integers(-8, 9, n).astype(np.float32)
    if dim == 1:
        return a
    out = np.zeros((n, dim), np.float32)
    out[:, 0], out[:, 1] = 3 * a, 4 * a
    return out


BUILDERS = {"gaussian": gaussian, "exact": exact}
_CASES = {}


def make_case(name, kind, dim, q_lens, t_lens, twin=None):
    """queries, templates and their references, computed once and left unchanged.  twin = (query index, template index): that template
    IS that query (same array), for the zero on the diagonal"""
    key = (name, kind, dim, tuple(q_lens), tuple(t_lens), twin)
    if key not in _CASES:
        mk = BUILDERS[kind]
        Q = [mk(n, dim, 100 + k) for k, n in enumerate(q_lens)]
        T = [mk(n, dim, 200 + k) for k, n in enumerate(t_lens)]
        if twin is not None:
            assert len(Q[twin[0]]) == len(T[twin[1]])
            T[twin[1]] = Q[twin[0]]
        ref = ref64_matrix(Q, T)
        c = {"name": name, "kind": kind, "dim": dim, "Q": Q, "T": T, "ref": ref, "emu": emu32_matrix(Q, T), "band": band_matrix(Q, T, ref),
             "rc": np.array([[len(q) + len(t) for t in T] for q in Q], dtype=np.float32), "twin": twin}
        for v in Q + T + [c["ref"], c["emu"], c["band"], c["rc"]]:
            v.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def sweep_case(kind, dim, w):
    """the instance sweep's call: template 4 (65 rows) is query 4"""
    return make_case("sweep W=%d" % w, kind, dim, QUERY_LENS, template_lens(dim, w), twin=(4, 4))


def block_case(kind, dim):
    return make_case("super-blocks", kind, dim, BLOCK_QUERIES, BLOCK_TEMPLATES)


def sub_case(c, qi, ti):
    """the call on a subset of a case's queries and templates: the same pairs, so the same references"""
    ix = np.ix_(qi, ti)
    return {"name": c["name"], "kind": c["kind"], "dim": c["dim"], "Q": [c["Q"][k] for k in qi], "T": [c["T"][k] for k in ti],
            "ref": c["ref"][ix], "emu": c["emu"][ix], "band": c["band"][ix], "rc": c["rc"][ix],
            "twin": None if c["twin"] is None or c["twin"][0] not in qi or c["twin"][1] not in ti
            else (list(qi).index(c["twin"][0]), list(ti).index(c["twin"][1]))}


# ------------------------------------------------------------------------------------------------- non-finite input
NAN, INF = np.float32(np.nan), np.float32(np.inf)
# (name, where in the query, value, where in the template, value, the float64 oracle's answer); a place is "first" / "mid" / "last" / None
NONFINITE = [("nan q first", "first", NAN, None, None, np.nan), ("nan q mid", "mid", NAN, None, None, np.nan),
             ("nan q last", "last", NAN, None, None, np.nan), ("nan t first", None, None, "first", NAN, np.nan),
             ("nan t mid", None, None, "mid", NAN, np.nan), ("nan t last", None, None, "last", NAN, np.nan),
             ("+inf q", "mid", INF, None, None, np.inf), ("+inf both", "mid", INF, "mid", INF, np.nan),
             ("-inf both", "first", -INF, "last", -INF, np.nan), ("+inf q -inf t", "mid", INF, "mid", -INF, np.inf)]


def put(seq, place, value, coord=1, at=None):
    """a copy of seq with `value` at its first / a middle / its last element (dim > 1: in coordinate `coord` of that row); at: the row"""
    if place is None:
        return seq
    s = np.array(seq, copy=True)
    n = len(s)
    row = {"first": 0, "mid": n // 2, "last": n - 1}[place] if at is None else at
    if s.ndim == 1:
        s[row] = value
    else:
        s[row, coord] = value
    return s


def nonfinite_pairs(dim, r=9, c=7, t_rows=None):
    """-> [(name, query, template, expected)] on one clean Gaussian pair; t_rows: place -> row, for a long template"""
    q, t = gaussian(r, dim, 300), gaussian(c, dim, 301)
    out = []
    for name, qp, qv, tp, tv, want in NONFINITE:
        out.append((name, put(q, qp, qv), put(t, tp, tv, at=None if t_rows is None or tp is None else t_rows[tp]), want))
    return q, t, out


def same_float(got, want):
    """NaN == NaN, +inf == +inf, else equal"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.array_equal(got, want, equal_nan=True))
