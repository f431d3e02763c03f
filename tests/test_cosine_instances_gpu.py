"""Every compiled instance of the cosine scorer (csrc/cosine.hip: cosine_reg_kernel<NQ = 8, 16, 24, 32>, cosine_bf16x3_kernel<NK = 4, 8,
12, 16; SPLIT = 1, 3>, the tiled cosine_kernel for d > 256) against float64, on both edges of the widths it covers, around the 32-row
centroid tile and the 128-row workgroup, with margins below, on and above the error bands, at every length of the device-side lists.

The yardstick is tests/cosine_cases.py: ref64 (the oracle), emu32 (a float32 numpy restatement of the fp32 kernel's formula), the
emulated split-precision sweeps, ONE comparison for distances and minima and ONE arg-min rule for every precision;
tests/test_cosine_instances_host.py checks the yardstick itself and the bands.  Every test prints what it measured as a
`cosine_accuracy {json}` line (pytest -s); profiles/cosine_accuracy.md is made of those lines."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from speech_signal_processing_amd import api
    return api


def record(**kw):
    print("cosine_accuracy " + json.dumps({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in kw.items()}))


def identify(api, c, precision=0, dist=False, N=None):
    X = c["X"] if N is None else c["X"][:N]
    r = api.cosine_identify(api.default_context(), X, c["C"], dist=dist, precision=precision)
    return {k: (np.asarray(v) if k in ("dist", "argmin", "min") else v) for k, v in r.items()}


def row_tol(c):
    """(N,) the per-entry limit at each row's float64 minimum"""
    ref = np.nan_to_num(c["ref"], nan=np.inf)
    return c["tol"][np.arange(c["N"]), ref.argmin(axis=1)]


def check_precision0(api, c, what):
    """distances, arg-min and minimum with the distance matrix, then the same bits without it; returns the result without"""
    rd = identify(api, c, 0, dist=True)
    assert rd["dist"].shape == c["ref"].shape and rd["dist"].dtype == np.float32
    r_d = K.compare(rd["dist"], c["ref"], c["emu"], "%s dist" % what)
    fin = np.isfinite(c["ref"]).all(axis=1)
    r_m = K.compare(rd["min"][fin], c["ref"][fin].min(axis=1), c["emu"][fin].min(axis=1), "%s min" % what)
    left = K.check_argmin(rd["argmin"], c["ref"], c["tol"], c["C"], "%s arg-min" % what)
    # the minimum and the arg-min are the distance matrix's own (numpy: the first index of the smallest)
    assert np.array_equal(rd["min"][fin], rd["dist"][fin].min(axis=1)) and np.array_equal(rd["argmin"][fin], rd["dist"][fin].argmin(axis=1)), what
    r0 = identify(api, c, 0)
    assert np.array_equal(r0["argmin"], rd["argmin"]) and np.array_equal(r0["min"], rd["min"], equal_nan=True), (what, "without dist")
    record(case=c["name"], N=c["N"], S=c["S"], d=c["d"], precision=0, instance=K.instance(c["d"], 0), max_ratio=r_d["max_ratio"],
           rms_ratio=r_d["rms_ratio"], max_vs_emu=r_d["max_vs_emu"], rms_vs_emu=r_d["rms_vs_emu"], max_err=float("%.3e" % r_d["max_err"]),
           emu_max_err=float("%.3e" % r_d["emu_max_err"]), min_max_ratio=r_m["max_ratio"], left_out=left)
    return r0


def check_split(api, c, precision, r0, what):
    """precision 1 / 2: the arg-min rule, the minimum inside its band, exact where every row was scored again"""
    r = identify(api, c, precision)
    left = K.check_argmin(r["argmin"], c["ref"], c["tol"], c["C"], "%s arg-min" % what)
    d, N = c["d"], c["N"]
    allowed = np.full(N, K.band(d) if precision == 1 else K.band1(d))
    if precision == 2 and c["S"] > 1:
        # rows the first sweep MAY have decided are held to band1; those it certainly handed on (emulation) to band
        sure1, _ = K.listed(c["cos_hi"], 2 * K.band1(d), K.order_slack(d))
        allowed = np.where(sure1, K.band(d), K.band1(d))
    used = K.check_min(r["min"], c["ref"], allowed + row_tol(c), "%s min" % what)
    assert 0 <= r["rescored"] <= N and (precision == 1 or r["rescored"] <= r["split_rows"] <= N), (what, r["rescored"], r["split_rows"])
    if r["rescored"] == N:   # "exact on the re-scored rows"
        assert np.array_equal(r["min"], r0["min"], equal_nan=True) and np.array_equal(r["argmin"], r0["argmin"]), (what, "every row re-scored")
    record(case=c["name"], N=N, S=c["S"], d=d, precision=precision, instance=K.instance(d, precision), min_over_allowance=used,
           rescored=r["rescored"], split_rows=r["split_rows"], listed_share=r["rescored"] / N, split_share=r["split_rows"] / N, left_out=left)
    return r


# ------------------------------------------------------------------------------------------------- the instance sweep
SWEEP = [(d, K.SWEEP_N) for d in K.SWEEP_D] + list(K.SMALL_N)


@pytest.mark.parametrize("d,N", SWEEP, ids=["d%d_N%d" % s for s in SWEEP])
def test_instance_sweep(api, d, N):
    c = K.sweep_case(d)
    if N != K.SWEEP_N:
        c = K.head_of(c, N)
    what = "d=%d S=%d N=%d" % (d, c["S"], N)
    print("instance list: %s: %s | %s" % (what, K.instance(d, 0), K.instance(d, 2)))
    r0 = check_precision0(api, c, what + " precision 0")
    for precision in (1, 2):
        check_split(api, c, precision, r0, "%s precision %d" % (what, precision))


# ------------------------------------------------------------------------------------------------- the tiled kernel
@pytest.mark.parametrize("d,S,N", K.TILED, ids=["d%d_S%d_N%d" % t for t in K.TILED])
def test_tiled_kernel(api, d, S, N):
    c = K.tiled_case(d, S, N)
    what = "tiled d=%d S=%d N=%d" % (d, S, N)
    r0 = check_precision0(api, c, what)
    for precision in (1, 2):
        with pytest.raises(NotImplementedError, match="d <= 256"):
            identify(api, c, precision)
    after = identify(api, c, 0)     # a refused call leaves nothing behind
    assert np.array_equal(after["argmin"], r0["argmin"]) and np.array_equal(after["min"], r0["min"])


# ------------------------------------------------------------------------------------------------- the margin ladder
@pytest.mark.parametrize("d", K.LADDER_D)
def test_margin_ladder(api, d):
    """rows whose two best float64 cosines are band x {1/4 .. 8} and band1 x {1/4 .. 8} apart: the arg-min is float64's at precision 1 and 2,
    and the NUMBER of rows each sweep hands on lies between the emulation's two counts — margin below twice the band minus / plus
    4 d 2^-23 for the matrix core's summation order.  A band that is too small in the kernel falls under the lower count."""
    c = K.ladder_case(d)
    slack = K.order_slack(d)
    sure3, maybe3 = K.listed(c["cos_x3"], 2 * K.band(d), slack)
    sure1, maybe1 = K.listed(c["cos_hi"], 2 * K.band1(d), slack)
    r0 = identify(api, c, 0)
    K.check_argmin(r0["argmin"], c["ref"], c["tol"], c["C"], "ladder d=%d precision 0" % d)
    r1 = check_split(api, c, 1, r0, "ladder d=%d precision 1" % d)
    r2 = check_split(api, c, 2, r0, "ladder d=%d precision 2" % d)
    counts = dict(p1_rescored=(int(sure3.sum()), r1["rescored"], int(maybe3.sum())),
                  p2_split_rows=(int(sure1.sum()), r2["split_rows"], int(maybe1.sum())),
                  p2_rescored=(int((sure1 & sure3).sum()), r2["rescored"], int((maybe1 & maybe3).sum())))
    # what the constants before the correction would have listed, for the record
    old3, _ = K.listed(c["cos_x3"], 2 * K.old_band(d), 0.0)
    old1, _ = K.listed(c["cos_hi"], 2 * K.old_band1(d), 0.0)
    record(case=c["name"], N=c["N"], S=c["S"], d=d, instance=K.instance(d, 2), old_band_p1_rescored=int(old3.sum()),
           old_band_p2_split_rows=int(old1.sum()), **{k: list(v) for k, v in counts.items()})
    for k, (lo, got, hi) in counts.items():
        assert lo <= got <= hi, (d, k, lo, got, hi)


# ------------------------------------------------------------------------------------------------- list lengths
@pytest.fixture(scope="module")
def list_base(api):
    return identify(api, K.list_case(0), 2)


@pytest.mark.parametrize("L", K.LIST_L)
def test_device_side_list_lengths(api, list_base, L):
    """exactly L of 1000 rows reach the fp32 kernel through both lists (a list of a list); the rows that do not are untouched by it: the
    bits they have when no row is listed"""
    c = K.list_case(L)
    r0 = identify(api, c, 0)
    r2 = check_split(api, c, 2, r0, "list L=%d precision 2" % L)
    assert r2["rescored"] == L and r2["split_rows"] >= L, (L, r2["rescored"], r2["split_rows"])
    keep = ~c["close"]
    assert np.array_equal(r2["argmin"][keep], list_base["argmin"][keep]) and np.array_equal(r2["min"][keep], list_base["min"][keep]), L
    # the listed rows carry the fp32 kernel's answer
    assert np.array_equal(r2["argmin"][c["close"]], r0["argmin"][c["close"]]) and np.array_equal(r2["min"][c["close"]], r0["min"][c["close"]]), L
    r1 = check_split(api, c, 1, r0, "list L=%d precision 1" % L)
    assert r1["rescored"] == L, (L, r1["rescored"])


# ------------------------------------------------------------------------------------------------- duplicates and ties across tiles
@pytest.mark.parametrize("d", (64, 256))
def test_duplicated_centroid_across_tiles_gives_the_first_index(api, d):
    c = K.duplicate_case(d)
    S = c["S"]
    assert np.array_equal(c["C"][3], c["C"][35]) and np.array_equal(c["C"][3], c["C"][S - 1])
    theirs = np.isin(c["label"], (3, 35, S - 1))
    assert theirs.sum() >= 100
    r0 = identify(api, c, 0)
    for precision in (0, 1, 2, 3):
        r = identify(api, c, precision, dist=(precision == 0))
        K.check_argmin(r["argmin"], c["ref"], c["tol"], c["C"], "duplicates d=%d precision %d" % (d, precision))
        assert (r["argmin"][theirs] == 3).all(), (d, precision)
        assert not np.isin(r["argmin"], (35, S - 1)).any(), (d, precision)
        assert np.array_equal(r["argmin"], r0["argmin"]), (d, precision)
        if precision in (1, 2):
            assert r["rescored"] >= int(theirs.sum())      # an exact tie cannot be called by an approximate sweep
    record(case=c["name"], N=c["N"], S=S, d=d, instance=K.instance(d, 2), tied_rows=int(theirs.sum()))


# ------------------------------------------------------------------------------------------------- row norms
@pytest.mark.parametrize("d", (64, 256))
def test_row_norms_over_eighty_binades_with_rows_that_are_not_numbers(api, d):
    c = K.norms_case(d)
    bad = c["nan_rows"]
    what = "norms d=%d" % d
    r0 = check_precision0(api, c, what + " precision 0")
    rd = identify(api, c, 0, dist=True)
    res = {0: r0}
    for precision in (1, 2):
        res[precision] = check_split(api, c, precision, r0, "%s precision %d" % (what, precision))
    # the NaN rules of test_cosine_nan_rules_match_scipy_and_the_reference_scan: a NaN stays a NaN and orders first
    assert np.isnan(rd["dist"][bad]).all()
    for precision, r in res.items():
        assert np.isnan(r["min"][bad]).all() and (r["argmin"][bad] == 0).all(), (what, precision)
        ok = np.ones(c["N"], bool)
        ok[bad] = False
        assert np.isfinite(r["min"][ok]).all(), (what, precision)


# ------------------------------------------------------------------------------------------------- the auto path
@pytest.mark.parametrize("kind", sorted(K.AUTO_KINDS))
def test_auto_path_with_nothing_and_37_rows_behind_the_pilot(api, monkeypatch, kind):
    """precision 3 at the smallest N the cost gate lets through, the pilot set to N rounded down to whole workgroups: the sweep behind the
    pilot has 0 rows (N = 47 104) and 37 rows (N = 47 141)"""
    c = K.auto_case(kind)
    monkeypatch.setenv("SSP_COS_AUTO_PILOT", str(K.AUTO_N[0]))
    for N in K.AUTO_N:
        r = identify(api, c, 3, N=N)
        auto = r["auto"]
        what = "auto %s N=%d" % (kind, N)
        left = K.check_argmin_summary(r["argmin"], c, N, what)
        record(case=c["name"], N=N, S=c["S"], d=c["d"], precision=3, instance=K.instance(c["d"], 2), auto=auto, rescored=r["rescored"],
               split_rows=r["split_rows"], left_out=left)
        assert left <= K.LEFT_OUT_CAP, (what, left)
        assert auto["pilot_rows"] == K.AUTO_N[0] and N - auto["pilot_rows"] in (0, 37), (what, auto)
        assert auto["precision_used"] == K.AUTO_KINDS[kind], (what, auto)
        allowed = {2: K.band1(c["d"]), 1: K.band(c["d"]), 0: 0.0}[auto["precision_used"]] + c["tol"][:N]
        assert (np.abs(r["min"].astype(np.float64) - c["ref_min"][:N]) <= allowed).all(), what
        if kind == "duplicates":
            assert auto["pilot_to_fp32"] == auto["pilot_rows"], (what, auto)


# ------------------------------------------------------------------------------------------------- the host-fed sliced path
def test_host_fed_sliced_path(api, monkeypatch):
    """SSP_HOST_SLICE_MB = 1, N = 8000, d = 70: slices of 3744 rows, 29 workgroups and a quarter: against float64 and bit-equal to the
    device-pointer call"""
    import torch
    monkeypatch.setenv("SSP_HOST_SLICE_MB", "1")
    c = K.sliced_case()
    assert (1 << 20) // (c["d"] * 4) == 3744 and 3744 % 128 != 0 and c["X"].nbytes >= 2 * (1 << 20)
    r = identify(api, c, 0)
    fin = np.ones(c["N"], bool)
    r_m = K.compare(r["min"], c["ref"].min(axis=1), c["emu"].min(axis=1), "host sliced min")
    left = K.check_argmin(r["argmin"], c["ref"], c["tol"], c["C"], "host sliced arg-min")
    assert fin.all() and left <= K.LEFT_OUT_CAP
    tctx = api.default_context(torch_stream=True)
    rt = api.cosine_identify(tctx, torch.from_numpy(c["X"]).cuda(), torch.from_numpy(c["C"]).cuda())
    assert np.array_equal(rt["argmin"].cpu().numpy(), r["argmin"]) and np.array_equal(rt["min"].cpu().numpy(), r["min"])
    record(case=c["name"], N=c["N"], S=c["S"], d=c["d"], precision=0, instance=K.instance(c["d"], 0) + " host-fed, 3744-row slices",
           min_max_ratio=r_m["max_ratio"], left_out=left)


# ------------------------------------------------------------------------------------------------- the search's worst triples
@pytest.mark.parametrize("i", range(len(K.OLD_BAND_TRIPLES)))
def test_worst_triples_of_the_search_with_the_old_bands(api, i):
    """(x, c0, c1) on which the hi-parts sweep prefers c1 by more than twice the band it had before the correction while float64 prefers
    c0 by more than 2 tol: 130 copies of the row (two workgroups), the float64 arg-min on each at every precision"""
    t = K.triple_case(i)
    c = dict(t)
    c.update(X=np.repeat(t["X"], 130, axis=0), N=130)
    for k in ("ref", "emu", "tol", "cos_hi", "cos_x3"):
        c[k] = np.repeat(t[k], 130, axis=0)
    assert t["ref"][0, 0] < t["ref"][0, 1]
    r0 = identify(api, c, 0)
    for precision in (0, 1, 2):
        r = check_split(api, c, precision, r0, "triple %d precision %d" % (i, precision)) if precision else r0
        assert (r["argmin"] == 0).all(), (i, precision, r["argmin"][:4])
