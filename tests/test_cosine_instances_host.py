"""The yardsticks of tests/test_cosine_instances_gpu.py, checked without a GPU (tests/cosine_cases.py): the bf16 rounding of the
emulation is torch.bfloat16's; every GPU case meets its construction conditions (at most 1 % of its rows are left out of the exact
arg-min check, the ladder's margins sit on their targets after float32 rounding with the third-best centroid far away, the list cases
have exactly L close calls); the comparison has teeth; and the two error bands of include/ssp.h (csrc/cosine.hip cos_band, cos_band1)
HOLD against an emulation of the two sweeps — with the constants the library carried until this suite (leading terms 2^-18 and 2^-9
instead of 2^-16 and 2^-8) they do not, and a short search finds a row the hi-parts sweep would settle the wrong way."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_cases as K  # noqa: E402

BAND_D = (2, 4, 16, 64, 256)


def test_bf16_rounding_of_the_emulation_is_torch_bfloat16s():
    import torch
    rng = np.random.default_rng(1)
    v = (rng.standard_normal(200000) * 10.0 ** rng.uniform(-6, 6, 200000)).astype(np.float32)
    # exact midpoints between neighbouring bf16 numbers, of both parities (ties go to the even significand), and their neighbours
    base = (v[:50000].view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    mid = base.view(np.float32)
    v = np.concatenate([v, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 2.0 ** -126, 3.3895314e38], np.float32)])
    want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()
    got = K.bf16_rne(v)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (np.abs(got.astype(np.float64) - v) <= K.U_BF16 * np.abs(v.astype(np.float64))).all()    # u = 2^-8, and it is reached:
    assert (np.abs(got.astype(np.float64) - v) / np.abs(v.astype(np.float64) + 1e-300)).max() > 0.99 * K.U_BF16 / (1 + K.U_BF16)
    # the second step: |lo| <= u |v| and |v - hi - lo| <= u^2 |v|
    lo = K.bf16_rne(v - got)
    fin = np.abs(v) > 2.0 ** -100
    assert (np.abs(lo[fin].astype(np.float64)) <= K.U_BF16 * np.abs(v[fin].astype(np.float64))).all()
    r = v[fin].astype(np.float64) - got[fin] - lo[fin]
    assert (np.abs(r) <= K.U_BF16 ** 2 * np.abs(v[fin].astype(np.float64))).all()


def test_emu32_restates_the_kernel_formula():
    """one entry by hand, in numpy float32 scalars"""
    c = K.sweep_case(17)
    X, C = c["X"], c["C"]
    i, j = 5, 3
    ss = np.float32(0)
    for k in range(17):
        ss = np.float32(ss + C[j, k] * C[j, k])
    inv = np.float32(1) / np.sqrt(ss)
    sx = np.float32(0)
    for k in range(17):
        sx = np.float32(sx + X[i, k] * X[i, k])
    ix = np.float32(1) / np.sqrt(sx)
    acc = np.float32(0)
    for k in range(17):
        acc = np.float32(acc + X[i, k] * np.float32(C[j, k] * inv))
    want = min(max(np.float32(1) - acc * ix, np.float32(0)), np.float32(2))
    assert c["emu"][i, j] == want and c["emu"].dtype == np.float32
    # float64 and float32 agree to float32 accuracy on every case entry
    assert np.abs(c["emu"] - c["ref"]).max() < 20 * 2.0 ** -24


def gpu_cases():
    for d in K.SWEEP_D:
        yield K.sweep_case(d), False
    for d, N in K.SMALL_N:
        yield K.head_of(K.sweep_case(d), N), False
    for d, S, N in K.TILED:
        yield K.tiled_case(d, S, N), False
    for d in K.LADDER_D:
        yield K.ladder_case(d), True
    for L in K.LIST_L:
        yield K.list_case(L), True
    for d in (64, 256):
        yield K.duplicate_case(d), True
        yield K.norms_case(d), False


def test_every_case_is_finite_and_keeps_the_share_of_undecided_rows_under_the_cap():
    """from ref64 and emu32 alone.  The ladder, list and duplicate cases are about ties: exempt."""
    seen = 0
    for c, about_ties in gpu_cases():
        fin = np.isfinite(c["ref"]).all(axis=1)
        assert np.isfinite(c["emu"][fin]).all(), c["name"]
        assert np.isnan(c["emu"][~fin]).all(), (c["name"], "emu32 and ref64 disagree on which rows are not numbers")
        if "nan_rows" in c:
            assert np.array_equal(np.flatnonzero(~fin), c["nan_rows"])
        else:
            assert fin.all(), c["name"]
        share = K.left_out_share(c)
        if not about_ties:
            assert share <= K.LEFT_OUT_CAP, (c["name"], share)
        seen += 1
    assert seen == len(K.SWEEP_D) + len(K.SMALL_N) + len(K.TILED) + len(K.LADDER_D) + len(K.LIST_L) + 4


def test_the_sweep_reaches_every_instance_on_both_edges_of_its_range():
    lo = 1
    for nq, nk, hi in ((8, 4, 64), (16, 8, 128), (24, 12, 192), (32, 16, 256)):
        assert all(K.pick_nq(d) == nq and K.pick_nk(d) == nk for d in range(lo, hi + 1))
        ds = [d for d in K.SWEEP_D if K.pick_nq(d) == nq]
        assert min(ds) == lo and max(ds) == hi and len(ds) >= 3, (nq, ds)
        lo = hi + 1
    assert K.pick_nq(257) == -1 and K.pick_nk(257) == 0
    assert {K.sweep_S(d) for d in K.SWEEP_D} == set(K.SWEEP_S)
    assert {d for d, _, _ in K.TILED} == {257, 288, 320, 511} and {S for _, S, _ in K.TILED} == {1, 127, 128, 129}
    assert {N for _, _, N in K.TILED} == {1, 129, 300}
    assert K.SWEEP_N == 3 * 128 + 5 and {N for _, N in K.SMALL_N} == {1, 127, 128, 129}


@pytest.mark.parametrize("d", K.LADDER_D)
def test_the_ladder_sits_on_its_rungs_after_float32_rounding(d):
    c = K.ladder_case(d)
    rows = np.arange(c["N"])
    cos = 1.0 - c["ref"]
    # rounding X and C to float32 moves a cosine by at most 4 2^-24 (each component of both vectors by 2^-24 relative, numerator and
    # norms), a margin by twice that
    margin = cos[rows, c["win"]] - cos[rows, c["lose"]]
    assert np.abs(margin - c["target"]).max() <= 2.0 ** -21, (d, np.abs(margin - c["target"]).max())
    assert np.abs(cos[rows, c["win"]] - 0.5).max() <= 2.0 ** -21          # the best cosine sits near 0.5, not near 1
    third = cos.copy()
    third[rows, c["win"]] = -np.inf
    third[rows, c["lose"]] = -np.inf
    assert (cos[rows, c["win"]] - third.max(axis=1) >= 10 * K.band1(d)).all(), (d, "a third centroid is within 10 band1")
    assert np.array_equal(c["ref"].argmin(axis=1), c["win"])
    # every rung has its 64 rows, scattered: no wave of 32 consecutive rows holds one rung only
    for which, b in ((0, K.band(d)), (1, K.band1(d))):
        for r in K.RUNGS:
            assert int(((c["which"] == which) & (c["target"] == b * r)).sum()) == K.ROWS_PER_RUNG
    assert all(len(set(c["target"][w:w + 32])) > 4 for w in range(0, c["N"] - 31, 32))
    assert len(set(c["win"])) == 8
    # the emulated sweeps list what the rungs say: everything at or under one band certainly, nothing at 4 bands or more
    for cosm, b, which in ((c["cos_x3"], K.band(d), 0), (c["cos_hi"], K.band1(d), 1)):
        sure, maybe = K.listed(cosm, 2 * b, K.order_slack(d))
        sel = c["which"] == which
        assert sure[sel & (c["target"] <= 0.5 * b)].all() and not maybe[sel & (c["target"] >= 4 * b)].any()
        assert 0 < int(sure.sum()) <= int(maybe.sum()) < c["N"]
    # the counts pin the constants: what the bands before the correction would list falls under the lower count — the hi-parts sweep at
    # every d; the bf16x3 sweep where a rung lies between the two thresholds (d = 16: one band is 5.5e-5, the old threshold 4.1e-5, the
    # lower count's 1.03e-4; from d = 64 on the slack of the summation order is as wide as the correction)
    old1, _ = K.listed(c["cos_hi"], 2 * K.old_band1(d), 0.0)
    old3, _ = K.listed(c["cos_x3"], 2 * K.old_band(d), 0.0)
    sure1, _ = K.listed(c["cos_hi"], 2 * K.band1(d), K.order_slack(d))
    sure3, _ = K.listed(c["cos_x3"], 2 * K.band(d), K.order_slack(d))
    assert int(old1.sum()) < int(sure1.sum()) and int((old1 & old3).sum()) <= int((sure1 & sure3).sum()), d
    if d == 16:
        assert int(old3.sum()) + K.ROWS_PER_RUNG // 2 < int(sure3.sum())


@pytest.mark.parametrize("L", K.LIST_L)
def test_the_list_cases_have_exactly_L_close_calls(L):
    c = K.list_case(L)
    assert int(c["close"].sum()) == L
    slack = K.order_slack(c["d"])
    sure3, maybe3 = K.listed(c["cos_x3"], 2 * K.band(c["d"]), slack)
    sure1, maybe1 = K.listed(c["cos_hi"], 2 * K.band1(c["d"]), slack)
    # the close rows go through both sweeps whatever the summation order; no other row can reach fp32
    assert np.array_equal(sure3 & sure1, c["close"]) and np.array_equal(maybe3 & maybe1, c["close"])
    assert np.array_equal(sure3, c["close"]) and np.array_equal(maybe3, c["close"])      # (precision 1: the bf16x3 sweep alone)
    # the other rows are the same rows in every case
    c0 = K.list_case(0)
    assert np.array_equal(c["C"], c0["C"]) and np.array_equal(c["X"][~c["close"]], c0["X"][~c["close"]])
    b1, b2, _ = K.top2(1.0 - c["ref"])
    assert ((b1 - b2)[~c["close"]] > 4 * K.band(c["d"])).all()


def test_the_comparison_passes_emu32_in_another_order_and_fails_one_entry_off_by_1e_4_of_its_norm():
    c = K.sweep_case(128)
    X, C = c["X"], c["C"]
    chat, _ = K.unit32(C)
    _, ix = K.unit32(X)
    acc = np.zeros((c["N"], c["S"]), np.float32)
    for k in reversed(range(c["d"])):
        acc = acc + X[:, k:k + 1] * chat[None, :, k]
    alt = np.clip(np.float32(1) - acc * ix[:, None], np.float32(0), np.float32(2))
    r = K.compare(alt, c["ref"], c["emu"], "reverse order")
    print("reverse-order float32 evaluation:", r)
    assert r["max_ratio"] < 0.5 and r["rms_ratio"] < 0.7
    # the mutation: ONE entry of ONE centroid moved by 1e-4 of the centroid's norm
    bad = C.copy()
    j = int(np.bincount(c["label"], minlength=c["S"]).argmax())
    bad[j, 0] += np.float32(1e-4 * np.linalg.norm(C[j].astype(np.float64)))
    moved = np.abs(K.ref64(X, bad) - c["ref"])
    assert (moved > 1.5 * c["tol"]).any()     # (1e-4 / sqrt(d) of a cosine: about 1e-5, the limit about 6e-6)
    with pytest.raises(AssertionError, match="x its limit"):
        K.compare(K.emu32(X, bad), c["ref"], c["emu"], "one entry moved")
    # and the arg-min rule: swapping two centroids' answers on the decided rows fails it, the float64 answer passes
    am = c["ref"].argmin(axis=1)
    assert K.check_argmin(am, c["ref"], c["tol"], C) <= K.LEFT_OUT_CAP
    wrong = am.copy()
    wrong[0] = (wrong[0] + 1) % c["S"]
    with pytest.raises(AssertionError, match="another arg-min"):
        K.check_argmin(wrong, c["ref"], c["tol"], C)
    dup = K.duplicate_case(64)
    am = K.first_of_duplicates(dup["C"])[dup["ref"].argmin(axis=1)]
    K.check_argmin(am, dup["ref"], dup["tol"], dup["C"])
    later = np.where(am == 3, 35, am)
    with pytest.raises(AssertionError, match="another arg-min|first index"):
        K.check_argmin(later, dup["ref"], dup["tol"], dup["C"])


# ------------------------------------------------------------------------------------------------- the band claims
@pytest.mark.parametrize("d", BAND_D)
def test_both_sweeps_stay_inside_their_bands_by_emulation(d):
    """the midpoint-scan family and 20 000 seeded random near-parallel pairs: max|emu_x3 - ref64| <= band(d), max|emu_hi - ref64| <=
    band1(d)"""
    e_hi, e_x3 = K.band_errors(d)
    print("cosine_band d=%d: hi parts %.3e of band1 %.3e (before the correction %.3e); bf16x3 %.3e of band %.3e (before %.3e)"
          % (d, e_hi, K.band1(d), K.old_band1(d), e_x3, K.band(d), K.old_band(d)))
    assert e_x3 <= K.band(d), (d, e_x3, K.band(d))
    assert e_hi <= K.band1(d), (d, e_hi, K.band1(d))
    # the bands are not loose by more than their accumulation terms allow: the hi-parts sweep uses over two thirds of its band somewhere
    if d in (16, 64):
        assert e_hi > 0.66 * K.band1(d)


def test_the_constants_before_the_correction_fail_the_same_claims():
    """leading terms 3.01 2^-18 / 2.01 2^-9 (u taken for 2^-9): the hi-parts sweep leaves its band at every d, the bf16x3 sweep at small
    d, where the accumulation term does not hide it"""
    for d in BAND_D:
        e_hi, e_x3 = K.band_errors(d)
        assert e_hi > K.old_band1(d), d
    assert K.band_errors(4)[1] > K.old_band(4) and K.band_errors(16)[1] > K.old_band(16)
    assert K.band_errors(256)[1] <= K.old_band(256)     # (at d = 256 the old band held, through its accumulation term alone)


@pytest.mark.parametrize("d", (4, 8, 16))
@pytest.mark.parametrize("split", (1, 3))
def test_a_bounded_search_finds_no_wrong_decision(d, split):
    """3000 steps of 64 seeded hill climbers over (x, c0, c1): float64 prefers c0 by more than 2 tol, the emulated sweep would have to
    prefer c1 by at least twice its band"""
    score, _, _ = K.search_wrong_decision(d, split, K.band1 if split == 1 else K.band)
    print("cosine_search d=%d split=%d: best (sweep margin for the wrong centroid - 2 band) = %.3e" % (d, split, score))
    assert score < 0.0, (d, split, score)


def test_the_search_finds_a_wrong_decision_with_the_constants_before_the_correction():
    """d = 4, the hi-parts sweep, old_band1: a row the first stage of the cascade would have settled against float64.  The triple it finds
    is the first of OLD_BAND_TRIPLES, which the GPU file runs."""
    score, T, m64 = K.search_wrong_decision(4, 1, K.old_band1)
    assert score >= 0.0 and m64 > 0.0, (score, m64)
    assert len(K.OLD_BAND_TRIPLES) >= 1
    for a, b in zip(T, K.OLD_BAND_TRIPLES[0]):
        assert np.array_equal(a, np.asarray(b, dtype=np.float32))
    for i in range(len(K.OLD_BAND_TRIPLES)):
        c = K.triple_case(i)
        assert c["ref"][0, 0] < c["ref"][0, 1] - 2 * c["tol"].max()                      # float64: centroid 0, by more than 2 tol
        b1, b2, am = K.top2(c["cos_hi"])
        assert am[0] == 1 and b1[0] - b2[0] >= 2 * K.old_band1(4)                         # the old first sweep settles it: centroid 1
        assert b1[0] - b2[0] < 2 * K.band1(4) - K.order_slack(4)                          # the corrected one hands it on
