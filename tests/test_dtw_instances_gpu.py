"""Every compiled instance of the all-pairs DTW matcher (csrc/dtw.hip: dtw1_kernel<W = 4, 8, 12, 16, 20, 24, 32> for dim == 1,
dtw_kernel<W = 4, 8, 16, 32; float, false> for dim > 1) against float64, with a template on both edges of the instance's range
(the shortest longest-template that selects W; 64 W - 1, a ragged last lane; 64 W, every lane full), across the super-block edges of
W = 32 (2048 / 2049 / 4096 / 4097 / 6145 columns), with empty sequences, through device pointers at odd addresses, with its inputs
still in flight, and on input that is not finite.

The yardstick is tests/dtw_cases.py: ref64 (the oracle), emu32 (a float32 numpy restatement of the recurrence) and the derived band;
tests/test_dtw_instances_host.py checks the yardstick itself.  The rules: exact inputs — the bits of float32(ref64); dim 1 — the bits of
emu32; dim > 1 — inside the band, and 0 for a sequence against itself; normalize — the plain result divided in float32, within 1 ulp.
Every call prints what it measured as a `dtw_accuracy {json}` line (pytest -s); profiles/dtw_accuracy.md is made of those lines."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_cases as K              # noqa: E402
import stream_order as SO          # noqa: E402
import test_gpu_alignment as GA    # noqa: E402  (Arrays: guarded, skewed device arrays)

pytestmark = pytest.mark.gpu
DEVICE = 1


@pytest.fixture(scope="module")
def api():
    from speech_signal_processing_amd import api
    return api


def record(**kw):
    print("dtw_accuracy " + json.dumps({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in kw.items()}))


def check_call(api, c, w, what):
    """one call and the same call with normalize=True against the case's references; -> the plain result"""
    dim, Q, T = c["dim"], c["Q"], c["T"]
    assert K.pick_w(dim, max(len(t) for t in T)) == w, (what, "the call does not select W = %d" % w)
    ctx = api.default_context()
    got = api.dtw_distances(ctx, Q, T)
    gotn = api.dtw_distances(ctx, Q, T, normalize=True)
    assert got.shape == gotn.shape == c["ref"].shape and got.dtype == gotn.dtype == np.float32, what
    err = np.abs(got.astype(np.float64) - c["ref"])
    ratio = float(np.max(np.divide(err, c["band"], out=np.zeros_like(err), where=c["band"] > 0)))
    off_emu = int(np.count_nonzero(got != c["emu"]))
    record(instance=K.instance_name(dim, w), case=c["name"], inputs=c["kind"], dim=dim, queries=[len(q) for q in Q],
           templates=[len(t) for t in T], max_err_over_band=ratio, differ_from_emu32=off_emu, pairs=int(got.size))
    if c["kind"] == "exact":
        assert np.array_equal(got, c["ref"].astype(np.float32)), (what, "exact inputs", np.argwhere(got != c["ref"].astype(np.float32))[:4])
    elif dim == 1:
        assert np.array_equal(got, c["emu"]), (what, "bits of emu32", np.argwhere(got != c["emu"])[:4])
    else:
        assert (err <= c["band"]).all(), (what, "band", ratio, np.argwhere(err > c["band"])[:4])
    if c["twin"] is not None:
        assert c["Q"][c["twin"][0]] is c["T"][c["twin"][1]] and got[c["twin"]] == 0.0, (what, "a sequence against itself", got[c["twin"]])
    want = got / c["rc"]     # float32 / float32
    assert want.dtype == np.float32
    assert (np.abs(gotn.astype(np.float64) - want.astype(np.float64)) <= K.ulp32(want)).all(), (what, "normalize", np.argwhere(gotn != want)[:4])
    return got


# ------------------------------------------------------------------------------------------------- the instance sweep
SWEEP = [(1 if k == "dtw1_kernel" else 3, w) for k, w in K.INSTANCES] + [(13, 4)]   # dim 13: the row stride of dtw_kernel


@pytest.mark.parametrize("dim,w", SWEEP, ids=["dim%d_W%d" % s for s in SWEEP])
def test_instance_sweep(api, dim, w):
    """templates of 1, W - 1, W, W + 1, 65, lo, 64 W - 1 and 64 W columns against queries of 1, 2, 63, 64, 65 and 130 rows; then the call
    whose longest template is lo itself"""
    for kind in ("gaussian", "exact"):
        c = K.sweep_case(kind, dim, w)
        what = "%s %s" % (K.instance_name(dim, w), kind)
        assert [len(t) for t in c["T"]][-2:] == [64 * w - 1, 64 * w] and K.lo_of(dim, w) in [len(t) for t in c["T"]]
        full = check_call(api, c, w, what)
        low_t = K.low_edge_templates(dim, w)
        low = K.sub_case(c, list(range(len(c["Q"]))), low_t)
        assert max(len(t) for t in low["T"]) == K.lo_of(dim, w)
        got = check_call(api, low, w, what + " longest = lo")
        assert np.array_equal(got, full[:, low_t]), (what, "the same pairs in a call with shorter templates")


# ------------------------------------------------------------------------------------------------- super-blocks
@pytest.mark.parametrize("kind", ("gaussian", "exact"))
@pytest.mark.parametrize("dim", (1, 3))
def test_super_blocks(api, dim, kind):
    """W = 32 beyond 2048 columns: one full block with nothing parked, one and 33 columns into a second block, two full blocks, a third of
    one column, four blocks; queries of 1, 3, 64 and 70 rows in one call (every pair but the first parks its column at a non-zero offset
    of the boundary buffer, and the rows of a pair differ from the longest query's); then the same templates against a single query"""
    c = K.block_case(kind, dim)
    assert [len(t) for t in c["T"]] == [2048, 2049, 2081, 4096, 4097, 6145] and [len(q) for q in c["Q"]] == [1, 3, 64, 70]
    what = "%s super-blocks %s" % (K.instance_name(dim, 32), kind)
    full = check_call(api, c, 32, what)
    one = K.sub_case(c, [2], list(range(len(c["T"]))))
    got = check_call(api, one, 32, what + " single query")
    assert np.array_equal(got, full[2:3]), (what, "the same pairs in a call of one query")


# ------------------------------------------------------------------------------------------------- empty sequences
@pytest.mark.parametrize("dim", (1, 3))
def test_empty_sequences_score_plus_infinity(api, dim):
    c = K.make_case("empties", "gaussian", dim, (5, 70), (3, 300))
    ctx = api.default_context()
    empty = np.zeros((0,) if dim == 1 else (0, dim), np.float32)
    Q, T = [c["Q"][0], empty, c["Q"][1]], [empty, c["T"][0], c["T"][1], empty]
    for normalize in (False, True):
        base = api.dtw_distances(ctx, c["Q"], c["T"], normalize=normalize)
        got = api.dtw_distances(ctx, Q, T, normalize=normalize)
        assert got.shape == (3, 4)
        assert np.array_equal(got[np.ix_([0, 2], [1, 2])], base), (dim, normalize, "the neighbours of an empty sequence")
        rest = np.ones((3, 4), bool)
        rest[np.ix_([0, 2], [1, 2])] = False
        assert (got[rest] == np.inf).all() and rest.sum() == 8, (dim, normalize, got)
        only = api.dtw_distances(ctx, [empty], [empty, c["T"][0]], normalize=normalize)
        assert only.shape == (1, 2) and (only == np.inf).all(), (dim, normalize, only)
    assert (np.abs(api.dtw_distances(ctx, c["Q"], c["T"]).astype(np.float64) - c["ref"]) <= c["band"]).all()


# ------------------------------------------------------------------------------------------------- device pointers
def p(t):
    return C.c_void_p(t.data_ptr())


def _flat(seqs, dim):
    return np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32).reshape(-1, dim) for s in seqs]))


POINTER_CASES = {1: ((1, 65, 130), (5, 257, 300)), 3: ((2, 64), (94, 513))}     # dtw1_kernel<8>, dtw_kernel<16, float, false>


@pytest.mark.parametrize("shift", (0, 1, 2), ids=["xq4", "xq8", "xq12"])
@pytest.mark.parametrize("dim", (1, 3))
def test_device_pointers_at_odd_addresses(dim, shift):
    """ssp_dtw_distances with where = SSP_DEVICE: queries, templates and the output 4, 8 and 12 bytes past a 16-byte line, NaN in the
    guards around the inputs: the bits of the host-array call, the guard bytes untouched"""
    from speech_signal_processing_amd import _lib, api
    ctx = api.default_context(torch_stream=True)
    q_lens, t_lens = POINTER_CASES[dim]
    c = K.make_case("device pointers", "gaussian", dim, q_lens, t_lens)
    qs, ts = api.Segments.from_lengths(ctx, list(q_lens)), api.Segments.from_lengths(ctx, list(t_lens))
    skews = {"xq": GA.F32[shift], "xt": GA.F32[(shift + 1) % 3], "dist": GA.F32[(shift + 2) % 3]}
    host = api.dtw_distances(api.default_context(), c["Q"], c["T"])
    assert (np.abs(host.astype(np.float64) - c["ref"]) <= c["band"]).all() and (dim > 1 or np.array_equal(host, c["emu"]))
    for normalize in (0, 1):
        a = GA.Arrays(skews)
        xq, xt = a.inp("xq", _flat(c["Q"], dim)), a.inp("xt", _flat(c["T"], dim))
        out = a.out("dist", (len(q_lens), len(t_lens)))
        assert xq.data_ptr() % 16 == skews["xq"] and xt.data_ptr() % 16 == skews["xt"] and out.data_ptr() % 16 == skews["dist"]
        _lib.check(ctx._lib.ssp_dtw_distances(ctx._h, p(xq), qs._h, p(xt), ts._h, dim, normalize, p(out), DEVICE, None))
        got = a.finish()["dist"]
        want = api.dtw_distances(api.default_context(), c["Q"], c["T"], normalize=bool(normalize))
        assert got.dtype == np.float32 and np.array_equal(got, want), (dim, skews, normalize, np.argwhere(got != want)[:4])


# ------------------------------------------------------------------------------------------------- stream order
@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


def test_stream_order(cfg):
    """ssp_dtw_distances on device pointers while the producer of both inputs is still in flight on a side stream (NaN in the buffers
    until it arrives), the output consumed on that stream as the call returns: the bits of the call on inputs at rest"""
    ctx, _lib = cfg.ctx, cfg._lib
    q_lens, t_lens = (65, 130), (257, 1200)      # dtw1_kernel<20>
    c = K.make_case("stream order", "gaussian", 1, q_lens, t_lens)
    qs, ts = cfg.cached("dtw segments", lambda: (cfg.api.Segments.from_lengths(ctx, list(q_lens)), cfg.api.Segments.from_lengths(ctx, list(t_lens))))

    def call(d, o):
        with ctx._ordered(_lib.DEVICE):
            _lib.check(ctx._lib.ssp_dtw_distances(ctx._h, p(d["xq"]), qs._h, p(d["xt"]), ts._h, 1, 0, p(o["dist"]), _lib.DEVICE, None))
        return dict(o)
    base = cfg.race("ssp_dtw_distances", {"xq": _flat(c["Q"], 1).reshape(-1), "xt": _flat(c["T"], 1).reshape(-1)}, call,
                    outs={"dist": ((len(q_lens), len(t_lens)), "float32")}, waits=True)["dist"]
    assert np.array_equal(base, c["emu"]), (cfg.mode, np.argwhere(base != c["emu"])[:4])


# ------------------------------------------------------------------------------------------------- non-finite input
def _check_nonfinite(api, dim, clean_q, clean_t, Q, T, what):
    """all pairs of (clean + polluted queries) x (clean + polluted templates): every entry is what float64 answers; the pairs of two clean
    sequences keep the bits they have in a call that holds no bad element"""
    ctx = api.default_context()
    ref = K.ref64_matrix(Q, T)
    clean = np.array([[np.isfinite(q).all() and np.isfinite(t).all() for t in T] for q in Q])
    assert np.isfinite(ref[clean]).all() and not np.isfinite(ref[~clean]).any() and clean.sum() >= 1 and (~clean).sum() >= 20
    assert np.isnan(ref).sum() >= 10 and np.isposinf(ref).sum() >= 3, what
    for normalize in (False, True):
        base = api.dtw_distances(ctx, [clean_q], [clean_t], normalize=normalize)
        assert np.isfinite(base).all()
        got = api.dtw_distances(ctx, Q, T, normalize=normalize)
        assert got.shape == ref.shape
        bad = [(a, b, float(got[a, b]), float(ref[a, b])) for a, b in np.argwhere(~clean) if not K.same_float(got[a, b], ref[a, b])]
        assert not bad, (what, normalize, "%d of %d polluted pairs differ from float64 (query, template, got, float64)" % (len(bad), (~clean).sum()), bad[:8])
        assert (got[clean] == base[0, 0]).all(), (what, normalize, "a clean pair changed", got[clean], base)
    record(instance=K.instance_name(dim, K.pick_w(dim, max(len(t) for t in T))), case=what, dim=dim, pairs=int(ref.size),
           nan_pairs=int(np.isnan(ref).sum()), inf_pairs=int(np.isposinf(ref).sum()), clean_pairs=int(clean.sum()))


@pytest.mark.parametrize("dim", (1, 3))
def test_non_finite_input_answers_what_float64_answers(api, dim):
    """a 9 x 7 pair with NaN at the first, a middle and the last element of the query or of the template, +inf in the query alone, the same
    infinity in both (in one coordinate), opposite infinities: every combination in one call"""
    q, t, cases = K.nonfinite_pairs(dim)
    for name, qq, tt, want in cases:     # the table itself, pair by pair
        got = api.dtw_distances(api.default_context(), [qq], [tt])
        assert K.same_float(got[0, 0], want), (dim, name, float(got[0, 0]), want)
    Q = [q] + [qq for _, qq, _, _ in cases if qq is not q]
    T = [t] + [tt for _, _, tt, _ in cases if tt is not t]
    _check_nonfinite(api, dim, q, t, Q, T, "non-finite 9 x 7")
    # with empty sequences between the polluted ones (the rows of a bad element are found by its offset): empty pairs stay +inf
    empty = np.zeros((0,) if dim == 1 else (0, dim), np.float32)
    Q2, T2 = [empty, Q[1], empty, q, Q[4]], [t, empty, T[-1], empty]
    got = api.dtw_distances(api.default_context(), Q2, T2)
    for a, qq in enumerate(Q2):
        for b, tt in enumerate(T2):
            want = np.inf if len(qq) == 0 or len(tt) == 0 else np.float32(K.ref64(qq, tt))
            assert K.same_float(got[a, b], want) or (np.isfinite(want) and abs(got[a, b] - want) <= K.band(9, 7, dim, want)), (dim, a, b, got[a, b], want)


@pytest.mark.parametrize("dim", (1, 3))
def test_non_finite_input_across_super_blocks(api, dim):
    """the same cases against templates of 2049 columns (W = 32, two super-blocks): the bad element in the first block and in the second"""
    Q, T = None, None
    for at in (1000, 2048):
        q, t, cases = K.nonfinite_pairs(dim, r=9, c=2049, t_rows={"first": at, "mid": at, "last": at})
        if Q is None:
            Q, T = [q] + [qq for _, qq, _, _ in cases if qq is not q], [t]
        T += [tt for _, _, tt, _ in cases if tt is not t]
    assert len(T) == 13 and all(len(x) == 2049 for x in T)
    _check_nonfinite(api, dim, Q[0], T[0], Q, T, "non-finite 9 x 2049")
