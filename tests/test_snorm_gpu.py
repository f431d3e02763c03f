"""Score normalisation and detection-error counts on the GPU (ssp_topn_stats, ssp_snorm_apply, ssp_det_counts; api.topn_stats,
api.snorm_apply, api.det_counts, snorm.AsNorm / PldaAsNorm / CosineAsNorm, metrics.det_counts) against the restatement of
tests/snorm_oracle.py, on the smallest shapes at which each kernel can go wrong.
Bounds.  Top-N statistics: kth BIT-equal (equal as floats for +-0); mean and deviation within the project's parity bound 1e-4 max(1,
max|line|) of float64 (the error of a float32 emulation of the device's steps is printed beside the measured one).  Apply: the output
BIT-equal to the float32 restatement, max = out[argmax], ties to the first index.  Decisions: the arg-max equals the float64
restatement's on every row whose float64 best-to-second gap exceeds twice 1e-4 max(1, max|z row|) (tests/test_snorm_host.py holds the
share of rows left out under 5 %).  Histograms, NaN counts and ranges: EXACTLY the restatement's.  PLDA end to end: with delta = the
project's bound 1e-4 max(1, max|LLR|) on every ratio that enters a row, the top-N mean and deviation (order statistics, 1-Lipschitz in
the largest error) move by at most delta, x - mean by 2 delta, so a term a = (x - mean) / dev moves by at most (2 + |a|) delta / dev to
first order; the bound of a normalised score is half the sum of that over its two terms, doubled for the second-order rest."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_oracle as PO   # noqa: E402
import snorm_oracle as SN  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("mean", "std", "kth")


@pytest.fixture(scope="module")
def ctx():
    from speech_signal_processing_amd import api
    return api.default_context()


def _np(res, keys):
    return {k: (res[k].cpu().numpy() if hasattr(res[k], "cpu") else np.asarray(res[k])) for k in keys}


def _same(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in keys)


def _dev_matrix(X, pad):
    """X on the device inside a wider matrix: a view with leading dimension cols + pad whose gaps hold NaN"""
    import torch
    wide = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), device="cuda")
    wide[:, :X.shape[1]] = torch.from_numpy(X).cuda()
    return wide[:, :X.shape[1]] if pad else wide


def _check_stats(got, X_lines, n, what):
    """got: mean / std / kth of the lines (rows of X_lines)"""
    want = SN.topn_stats(X_lines, n)
    assert got["kth"].dtype == np.float32 and np.array_equal(got["kth"], want["kth"]), what   # (== : -0.0 equals +0.0)
    bound = SN.stat_bound(X_lines)
    em = np.abs(got["mean"] - want["mean"]) / bound
    es = np.abs(got["std"] - want["std"]) / bound
    emu = [SN.topn_fp32_emulation(line, n) for line in X_lines[:4]]
    emu_m = max(abs(m - want["mean"][i]) / bound[i] for i, (m, _, _) in enumerate(emu))
    emu_s = max(abs(s - want["std"][i]) / bound[i] for i, (_, s, _) in enumerate(emu))
    print("[measured] top-n %s: mean err %.3g, std err %.3g of the bound; fp32 emulation of the same steps (first lines) %.3g, %.3g" % (
        what, em.max(), es.max(), emu_m, emu_s))
    assert (em <= 1.0).all() and (es <= 1.0).all(), what


# --------------------------------------------------------------------------------------------------------------------- top-N statistics
@pytest.mark.parametrize("pad", [0, 3], ids=["dense", "ld+3"])
@pytest.mark.parametrize("shape", SN.TOPN_SHAPES, ids=lambda s: "%dx%d-top%d" % s)
def test_topn_rows(ctx, shape, pad):
    from speech_signal_processing_amd import api
    rows, cols, n = shape
    X = SN.topn_case(rows, cols)
    dev = _dev_matrix(X, pad)
    got = _np(api.topn_stats(ctx, dev, n), KEYS)
    _check_stats(got, X, n, "%s ld+%d" % (shape, pad))
    if rows > 2:
        assert got["std"][2] == 0.0 and got["mean"][2] == np.float32(0.1)          # the constant line
    if rows > 1:
        assert (got["mean"][1] < 0).all() and got["kth"][1] < 0                     # the all-negative line
    assert _same(got, _np(api.topn_stats(ctx, dev, n), KEYS), KEYS)                # same call, same bits
    last = _np(api.topn_stats(ctx, dev[rows - 1:], n), KEYS)                        # a line alone
    assert all(np.array_equal(last[k], got[k][rows - 1:]) for k in KEYS)
    if pad == 0:
        assert _same(got, _np(api.topn_stats(ctx, X, n), KEYS), KEYS)              # the host route


@pytest.mark.parametrize("shape", SN.AXIS0_SHAPES, ids=lambda s: "%dx%d" % s)
def test_topn_columns(ctx, shape):
    from speech_signal_processing_amd import api
    rows, cols = shape
    lines = SN.topn_case(cols, rows)                  # the columns, as rows
    X = np.ascontiguousarray(lines.T)
    for pad in (0, 3):
        dev = _dev_matrix(X, pad)
        got = _np(api.topn_stats(ctx, dev, SN.AXIS0_N, axis=0), KEYS)
        _check_stats(got, lines, SN.AXIS0_N, "axis 0 %s ld+%d" % (shape, pad))
        assert _same(got, _np(api.topn_stats(ctx, dev, SN.AXIS0_N, axis=0), KEYS), KEYS)
        one = _np(api.topn_stats(ctx, dev[:, cols - 1:], SN.AXIS0_N, axis=0), KEYS)
        assert all(np.array_equal(one[k], got[k][cols - 1:]) for k in KEYS)
        # the row kernel on the transposed matrix selects the same entries and adds them in the same order
        assert _same(got, _np(api.topn_stats(ctx, lines, SN.AXIS0_N, axis=1), KEYS), KEYS)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("case", [(5, 65, 7, 1), (5, 4097, 300, 1), (200, 70, 40, 0)], ids=["rows", "long-rows", "columns"])
def test_topn_non_finite_line_is_nan_and_alone(ctx, case, bad):
    from speech_signal_processing_amd import api
    rows, cols, n, axis = case
    X = SN.topn_case(rows, cols).copy()
    line = 3
    if axis == 1:
        X[line, cols // 2] = bad
    else:
        X[rows // 2, line] = bad
    got = _np(api.topn_stats(ctx, X, n, axis=axis), KEYS)
    Z = X.copy()
    if axis == 1:
        Z[line] = 0.0
    else:
        Z[:, line] = 0.0
    zero = _np(api.topn_stats(ctx, Z, n, axis=axis), KEYS)
    keep = np.arange(got["mean"].size) != line
    for k in KEYS:
        assert np.isnan(got[k][line]) and np.array_equal(got[k][keep], zero[k][keep]) and np.isfinite(zero[k]).all(), k


def test_topn_error_codes_and_the_ctx_stays_usable(ctx):
    from speech_signal_processing_amd import api, _lib
    X = SN.topn_case(5, 65)
    base = _np(api.topn_stats(ctx, X, 7), KEYS)
    out = np.zeros(5, np.float32)

    def raw(rows, cols, ld, axis, n):
        return ctx._lib.ssp_topn_stats(ctx._h, X.ctypes.data, rows, cols, ld, axis, n, out.ctypes.data, None, None, _lib.HOST, None)
    for args in ((5, 65, 65, 1, 0), (-1, 65, 65, 1, 7), (5, 0, 65, 1, 7), (5, 65, 64, 1, 7), (5, 65, 65, 2, 7)):
        assert raw(*args) == _lib.SSP_ERR_INVALID, args
    assert not out.any()
    with pytest.raises(ValueError):
        api.topn_stats(ctx, X, 0)
    with pytest.raises(NotImplementedError, match="65536"):
        api.topn_stats(ctx, np.zeros((1, 65537), np.float32), 3)
    with pytest.raises(NotImplementedError, match="65536"):
        api.topn_stats(ctx, np.zeros((65537, 1), np.float32), 3, axis=0)
    assert raw(0, 65, 65, 1, 7) == _lib.SSP_OK and not out.any()                    # rows == 0: a no-op
    assert api.topn_stats(ctx, X[:0], 7)["mean"].shape == (0,)
    assert _same(base, _np(api.topn_stats(ctx, X, 7), KEYS), KEYS)


# ------------------------------------------------------------------------------------------------------------------------------- apply
VARIANTS = {"s-norm": ("rm", "rs", "cm", "cs"), "t-norm": ("rm", "rs", None, None), "z-norm": (None, None, "cm", "cs")}
OUT = ("argmax", "max", "scores")


def _stats(g, variant, dev=False):
    import torch
    v = [None if k is None else g[k] for k in VARIANTS[variant]]
    return [torch.from_numpy(a).cuda() if dev and a is not None else a for a in v]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SN.APPLY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_apply_is_the_float32_restatement_bit_for_bit(ctx, shape, variant):
    import torch
    from speech_signal_processing_amd import api
    g = SN.apply_case(*shape)
    rm, rs, cm, cs = _stats(g, variant)
    want = SN.apply_f32(g["x"], rm, rs, cm, cs, 1e-6)
    wam, wmx = SN.decide(want)
    host = _np(api.snorm_apply(ctx, g["x"], rm, rs, cm, cs), OUT)
    assert np.array_equal(host["scores"], want) and np.array_equal(host["argmax"], wam) and np.array_equal(host["max"], wmx)
    assert host["argmax"].dtype == np.int32 and np.array_equal(host["max"], host["scores"][np.arange(shape[0]), host["argmax"]])
    d = _stats(g, variant, dev=True)
    for pad in (0, 3):
        x = _dev_matrix(g["x"], pad)
        res = api.snorm_apply(ctx, x, *d)
        assert res["scores"].is_cuda and _same(_np(res, OUT), host, OUT)
        res = api.snorm_apply(ctx, x, *d, out=x)                                   # in place
        assert res["scores"] is x and _same(_np(res, OUT), host, OUT)
    only = _np(api.snorm_apply(ctx, torch.from_numpy(g["x"]).cuda(), *d, out=False), ("argmax", "max"))
    assert _same(only, host, ("argmax", "max"))
    xh = g["x"].copy()
    assert api.snorm_apply(ctx, xh, rm, rs, cm, cs, out=xh)["scores"] is xh and np.array_equal(xh, want)   # in place on the host


def test_apply_ties_nan_rules_and_the_floor(ctx):
    from speech_signal_processing_amd import api
    g = SN.apply_case(300, 70)
    x = g["x"].copy()
    x[0, [9, 4, 66]] = 50.0            # equal scores under T-norm: equal z
    x[7, :] = -3.0                     # a constant row
    res = _np(api.snorm_apply(ctx, x, g["rm"], g["rs"]), OUT)
    assert res["argmax"][0] == 4 and res["argmax"][7] == 0
    assert np.array_equal(res["scores"], SN.apply_f32(x, g["rm"], g["rs"], None, None, 1e-6))
    rs, cm = g["rs"].copy(), g["cm"].copy()
    rs[2], cm[7] = np.nan, np.nan
    rm = g["rm"].copy()
    rm[5] = np.inf
    got = _np(api.snorm_apply(ctx, g["x"], rm, rs, cm, g["cs"]), OUT)
    want = SN.apply_f32(g["x"], rm, rs, cm, g["cs"], 1e-6)
    clean = SN.apply_f32(g["x"], g["rm"], g["rs"], g["cm"], g["cs"], 1e-6)
    assert np.array_equal(got["scores"], want, equal_nan=True)
    nan = np.isnan(got["scores"])
    assert nan[2].all() and nan[:, 7].all() and nan.sum() == 70 + 300 - 1
    untouched = np.ones_like(nan)
    untouched[[2, 5]] = False
    untouched[:, 7] = False
    assert np.array_equal(got["scores"][untouched], clean[untouched])
    wam, wmx = SN.decide(want)
    assert got["argmax"][2] == -1 and np.isnan(got["max"][2]) and np.array_equal(got["argmax"], wam)
    assert np.array_equal(got["max"], wmx, equal_nan=True) and (got["argmax"] != 7).all()
    # a zero deviation takes the floor
    zero = np.zeros(300, np.float32)
    fl = _np(api.snorm_apply(ctx, g["x"], g["rm"], zero, std_floor=0.25), OUT)
    assert np.array_equal(fl["scores"], (g["x"] - g["rm"][:, None]) / np.float32(0.25))
    for kw in ({"std_floor": 0.0}, {"std_floor": float("nan")}, {"std_floor": float("inf")}):
        with pytest.raises(ValueError):
            api.snorm_apply(ctx, g["x"], g["rm"], g["rs"], **kw)
    with pytest.raises(ValueError):
        api.snorm_apply(ctx, g["x"])
    with pytest.raises(ValueError):
        api.snorm_apply(ctx, g["x"], g["rm"], None)
    assert api.snorm_apply(ctx, g["x"][:0], g["rm"][:0], g["rs"][:0])["argmax"].shape == (0,)
    again = _np(api.snorm_apply(ctx, g["x"], rm, rs, cm, g["cs"]), OUT)
    assert _same(again, got, OUT)


def test_decision_case_through_asnorm(ctx):
    import torch
    from speech_signal_processing_amd import snorm
    g = SN.decision_case()
    norm = snorm.AsNorm(top_n=g["top_n"], ctx=ctx).fit(g["cohort_vs_enrolled"])
    res = _np(norm.normalize(g["x"], g["test_vs_cohort"]), OUT)
    z64 = g["z64"]
    err = np.abs(res["scores"] - z64).max(axis=1) / SN.z_bound(z64)
    emu = np.abs(g["z32"] - z64).max(axis=1) / SN.z_bound(z64)
    raw = g["x"].astype(np.float64).argmax(axis=1)
    print("[measured] decision case: err %.3g of the bound (fp32 emulation %.3g); %d of %d rows decided; arg-max differs from the raw one on %d rows; "
          "accuracy raw %.3f, normalised %.3f" % (err.max(), emu.max(), int(g["keep"].sum()), g["keep"].size, int((res["argmax"] != raw).sum()),
                                                  (raw == g["target"]).mean(), (res["argmax"] == g["target"]).mean()))
    assert (err <= 1.0).all()
    assert np.array_equal(res["argmax"][g["keep"]], z64.argmax(axis=1)[g["keep"]])
    assert (res["argmax"] != raw).any()
    assert np.array_equal(res["max"], res["scores"][np.arange(300), res["argmax"]])
    dev = norm.normalize(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["test_vs_cohort"]).cuda())
    assert dev["scores"].is_cuda and _same(_np(dev, OUT), res, OUT)
    assert _same(_np(norm.normalize(g["x"], g["test_vs_cohort"], out=False), ("argmax", "max")), res, ("argmax", "max"))


# ------------------------------------------------------------------------------------------------------------------- detection counts
DET = ("tar_hist", "non_hist", "nan_count", "range")


@pytest.mark.parametrize("shape", SN.DET_SHAPES, ids=lambda s: "N%d-S%d-M%d" % s)
def test_det_counts_are_exact(ctx, shape):
    import torch
    from speech_signal_processing_amd import api
    x, tgt, th = SN.det_case(*shape)
    want = SN.det_counts(x, tgt, th)
    host = api.det_counts(ctx, x, tgt, th)
    for k in DET:
        assert host[k].dtype == want[k].dtype and np.array_equal(host[k], want[k]), (k, host[k], want[k])
    dev = api.det_counts(ctx, _dev_matrix(x, 3), torch.from_numpy(tgt).cuda(), th)
    assert all(np.array_equal(dev[k], want[k]) for k in DET)
    if shape[2]:
        assert (x == th[0]).any()      # scores equal to a threshold are in the case
    if shape[0] >= 5:
        assert (tgt == -1).any() and want["nan_count"].tolist() == [1, 2]


def test_det_counts_bad_target_thresholds_and_the_default_grid(ctx):
    from speech_signal_processing_amd import api, metrics, _lib
    x, tgt, th = SN.det_case(300, 70, 1024)
    for bad in (70, -2):
        t2 = tgt.copy()
        t2[123] = bad
        with pytest.raises(ValueError, match="target"):
            api.det_counts(ctx, x, t2, th)
        outs = [np.full(1025, -5, np.int64), np.full(1025, -5, np.int64), np.full(2, -5, np.int64), np.full(4, -5, np.float32)]
        rc = ctx._lib.ssp_det_counts(ctx._h, x.ctypes.data, 300, 70, 70, t2.ctypes.data, th.ctypes.data, 1024, *[o.ctypes.data for o in outs],
                                     _lib.HOST, None)
        assert rc == _lib.SSP_ERR_INVALID and all((o == -5).all() for o in outs)   # nothing is written
    for grid in (th[::-1].copy(), np.array([0.0, np.nan], np.float32), np.zeros(4097, np.float32)):
        with pytest.raises(ValueError):
            api.det_counts(ctx, x, tgt, grid)
    want = SN.det_counts(x, tgt, th)
    assert all(np.array_equal(api.det_counts(ctx, x, tgt, th)[k], want[k]) for k in DET)   # the ctx is still usable
    # the default grid: linspace over the range of the scores that are not NaN (the case holds +-inf: none can be placed) ...
    with pytest.raises(ValueError, match="range"):
        metrics.det_counts(x, tgt, ctx=ctx)
    fin = np.where(np.isinf(x), np.float32(0), x)
    c = metrics.det_counts(fin, tgt, n_thresholds=64, ctx=ctx)
    lo, hi = np.nanmin(fin), np.nanmax(fin)
    assert np.array_equal(c["thresholds"], np.linspace(np.float64(lo), np.float64(hi), 64).astype(np.float32))
    w = SN.det_counts(fin, tgt, c["thresholds"])
    assert all(np.array_equal(c[k], w[k]) for k in DET)
    # ... and the rates read off it are those of the trial-by-trial count
    tar, non = SN.trial_scores(fin, tgt)
    bm, bf = SN.error_rates_brute(tar, non, c["thresholds"])
    _, miss, fa = metrics.error_rates(c)
    assert np.allclose(miss, bm, rtol=0, atol=1e-15) and np.allclose(fa, bf, rtol=0, atol=1e-15)
    assert abs(metrics.eer(c)[0] - SN.eer_brute(bm, bf, c["thresholds"])[0]) <= 1e-12
    assert abs(metrics.min_dcf(c) - SN.min_dcf_brute(bm, bf, 0.01, 1.0, 1.0)) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------- end to end
def test_plda_asnorm_end_to_end_and_slabs(ctx):
    """plda_oracle.end_to_end_case(): the training speakers double as the cohort (C = 30), top 10.  The restatement is driven by the
    oracle's float64 ratios of the fitted model's own parameters (the fit itself is tests/test_plda_gpu.py's subject)."""
    from speech_signal_processing_amd import plda, snorm
    e = PO.end_to_end_case()
    (Xtr, ltr), (Xen, len_), (Xte, lte) = e["train"], e["enrol"], e["test"]
    S, top = e["S"], 10
    model = plda.Plda(n_iter=5, ctx=ctx).fit(Xtr, ltr)
    scorer = model.enroll(Xen, len_, S)
    norm = snorm.PldaAsNorm(model, scorer, Xtr, ltr, S, top_n=top, workspace=1 << 30)
    got = norm.score(Xte, scores=True)
    assert got["scores"].shape == (Xte.shape[0], S) and got["argmax"].dtype == np.int32

    def proj(X):
        return (PO.front(X, model.mean_) - model.plda_mean_) @ model.transform_.T

    def means(T, lab):
        return np.stack([T[lab == s].mean(axis=0) for s in range(S)])
    enrol, n_en = means(proj(Xen), len_), np.bincount(len_, minlength=S)
    cohort, n_co = means(proj(Xtr), ltr), np.bincount(ltr, minlength=S)
    t = proj(Xte)
    x = PO.llr_direct(model.psi_, enrol, n_en, t)
    tc = PO.llr_direct(model.psi_, cohort, n_co, t)
    ce = PO.llr_direct(model.psi_, enrol, n_en, cohort.astype(np.float32))
    st, se = SN.topn_stats(tc, top), SN.topn_stats(ce, top, axis=0)
    z = SN.apply_f64(x, st["mean"], st["std"], se["mean"], se["std"], 1e-6)
    delta = 1e-4 * np.maximum(1.0, np.maximum(np.abs(x).max(axis=1), np.abs(tc).max(axis=1)))
    delta = np.maximum(delta, 1e-4 * max(1.0, np.abs(ce).max()))[:, None]
    a = np.abs(x - se["mean"][None]) / se["std"][None]
    b = np.abs(x - st["mean"][:, None]) / st["std"][:, None]
    bound = 2.0 * 0.5 * delta * ((2.0 + a) / se["std"][None] + (2.0 + b) / st["std"][:, None])
    err = np.abs(got["scores"] - z) / bound
    print("[measured] PLDA AS-norm end to end: err %.3g of the bound (bound %.3g .. %.3g, max|z| %.3g); accuracy raw %.3f, normalised %.3f" % (
        err.max(), bound.min(), bound.max(), np.abs(z).max(), (x.argmax(axis=1) == lte).mean(), (got["argmax"] == lte).mean()))
    assert (err <= 1.0).all()
    assert np.array_equal(got["max"], got["scores"][np.arange(Xte.shape[0]), got["argmax"]])
    # slabs: 1 slab above, then 7 rows a slab (18 slabs) and one row a slab — the same bits
    for ws in (7 * 4 * 2 * S, 1):
        small = snorm.PldaAsNorm(model, scorer, Xtr, ltr, S, top_n=top, workspace=ws)
        assert -(-Xte.shape[0] // small._slab_rows()) > 2
        assert _same(small.score(Xte, scores=True), got, OUT)
    assert _same(norm.score(Xte), got, ("argmax", "max"))


def test_cosine_asnorm(ctx):
    import torch
    from speech_signal_processing_amd import snorm
    rng = np.random.default_rng(77)
    S, Cc, d, N, top = 33, 70, 64, 129, 20
    cent = rng.standard_normal((S, d)).astype(np.float32)
    coh = rng.standard_normal((Cc, d)).astype(np.float32)
    spk = rng.integers(0, S, N)
    X = (cent[spk] + 0.7 * rng.standard_normal((N, d))).astype(np.float32)

    def sim(A, B):
        A, B = A.astype(np.float64), B.astype(np.float64)
        return (A / np.linalg.norm(A, axis=1, keepdims=True)) @ (B / np.linalg.norm(B, axis=1, keepdims=True)).T
    x, tc, ce = sim(X, cent), sim(X, coh), sim(coh, cent)
    st, se = SN.topn_stats(tc.astype(np.float32), top), SN.topn_stats(ce.astype(np.float32), top, axis=0)
    z = SN.apply_f64(x, st["mean"], st["std"], se["mean"], se["std"], 1e-6)
    norm = snorm.CosineAsNorm(cent, coh, top_n=top, ctx=ctx)
    got = norm.score(X, scores=True)
    # cosines within 5e-6 (the bound of the sweep's parity test); the terms as in the PLDA case above
    delta = 5e-6
    a, b = np.abs(x - se["mean"][None]) / se["std"][None], np.abs(x - st["mean"][:, None]) / st["std"][:, None]
    bound = 2.0 * 0.5 * delta * ((2.0 + a) / se["std"][None] + (2.0 + b) / st["std"][:, None])
    err = np.abs(got["scores"] - z) / bound
    print("[measured] cosine AS-norm: err %.3g of the bound; accuracy %.3f" % (err.max(), (got["argmax"] == spk).mean()))
    assert (err <= 1.0).all()
    keep = SN.decided_rows(z)
    assert np.array_equal(got["argmax"][keep], z.argmax(axis=1)[keep])
    dev = snorm.CosineAsNorm(torch.from_numpy(cent).cuda(), torch.from_numpy(coh).cuda(), top_n=top, workspace=40 * 4 * (S + Cc), ctx=ctx)
    res = dev.score(torch.from_numpy(X).cuda(), scores=True)
    assert res["scores"].is_cuda and _same(_np(res, OUT), got, OUT)
