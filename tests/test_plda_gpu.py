"""The PLDA back end on the GPU (ssp_plda_stats, ssp_plda_pack, ssp_plda_score; api.plda_stats, api.PldaScorer, plda.Plda) against the
float64 restatement of tests/plda_oracle.py, on the smallest shapes at which each kernel can go wrong.
Bounds.  Statistics: counts, sums and the mean exact (float64 sums in a fixed order); |S_w - oracle| <= 1e-4 max|S_w|, the project's parity
metric (the error of an fp32 emulation of the same steps is printed beside the measured one).  Scores: per row |llr - oracle| <= 1e-4
max(1, max|oracle row|) (an fp32 emulation of the packed form gave <= 1.8e-6 of such rows: the bound leaves room for summation order
only); the arg-max equals the oracle's on every row whose float64 gap between the best and the second-best ratio exceeds twice that bound
(tests/test_plda_host.py holds the share of rows left out under 5 %).  End to end: W and B after 5 EM iterations within 1e-3 max|.| of
the oracle's EM run from the oracle's statistics."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from speech_signal_processing_amd import api
    return api.default_context()


# ---------------------------------------------------------------------------------------------------------------------- statistics
# (q, N, S, labels): "random" unsorted, "sorted", "empty" = random with class 2 left without rows
STATS_CASES = [(5, 1, 1, "random"), (64, 1023, 7, "random"), (200, 1025, 40, "empty"), (256, 2500, 7, "sorted"), (5, 2500, 40, "random"),
               (256, 1025, 1, "random"), (64, 1, 7, "random"), (200, 1023, 40, "random")]
_STATS = {}


def _stats_case(case):
    if case not in _STATS:
        q, N, S, kind = case
        rng = np.random.default_rng(q * 7 + N + S)
        lab = rng.integers(0, S, N).astype(np.int32)
        if kind == "empty":
            lab[lab == 2] = 3
        if kind == "sorted":
            lab = np.sort(lab)
        X = (rng.standard_normal((N, q)) * (1.0 + rng.random(q)) + 3.0 * rng.standard_normal((S, q))[lab] + 0.5).astype(np.float32)
        _STATS[case] = (X, lab, PO.class_stats(X, lab, S))
    return _STATS[case]


@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "q%d-N%d-S%d-%s" % c)
def test_class_statistics(ctx, case):
    from speech_signal_processing_amd import api
    q, N, S, kind = case
    X, lab, want = _stats_case(case)
    got = api.plda_stats(ctx, X, lab, S)
    assert got["count"].dtype == np.int64 and np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["sum"], want["sum"])
    assert np.array_equal(got["mean"], want["mean"])
    if kind == "empty":
        assert got["count"][2] == 0 and not got["sum"][2].any()
    scale = max(np.abs(want["sw"]).max(), 1e-300)
    err = np.abs(got["sw"] - want["sw"]).max() / scale
    emu = np.abs(PO.sw_fp32_emulation(want["xc"]) - want["sw"]).max() / scale
    print("[measured] S_w %s: err %.3g of max|S_w|; fp32 emulation of the same steps %.3g" % (case, err, emu))
    assert np.abs(got["sw"] - want["sw"]).max() <= 1e-4 * np.abs(want["sw"]).max()
    assert np.array_equal(got["sw"], got["sw"].T)
    again = api.plda_stats(ctx, X, lab, S)
    assert all(np.array_equal(got[k], again[k]) for k in ("sum", "count", "mean", "sw"))


def test_class_statistics_from_device_arrays_equal_the_host_call(ctx):
    import torch
    from speech_signal_processing_amd import api
    X, lab, _ = _stats_case(STATS_CASES[2])
    host = api.plda_stats(ctx, X, lab, 40)
    dev = api.plda_stats(ctx, torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda(), 40)
    assert all(np.array_equal(host[k], dev[k]) for k in ("sum", "count", "mean", "sw"))


def test_statistics_error_codes_and_the_ctx_stays_usable(ctx):
    from speech_signal_processing_amd import api, plda
    X, lab, _ = _stats_case(STATS_CASES[1])
    base = api.plda_stats(ctx, X, lab, 7)
    for bad in (7, -1):
        l2 = lab.copy()
        l2[500] = bad
        with pytest.raises(ValueError, match="label"):
            api.plda_stats(ctx, X, l2, 7)
    with pytest.raises(NotImplementedError, match="256"):
        api.plda_stats(ctx, np.zeros((4, 257), np.float32), np.zeros(4, np.int32), 1)
    with pytest.raises(ValueError):
        api.plda_stats(ctx, X[:0], lab[:0], 7)
    with pytest.raises(ValueError):
        api.plda_stats(ctx, X, lab, 0)
    with pytest.raises(ValueError, match="one label per row"):
        api.plda_stats(ctx, X, lab[:-1], 7)
    for v in (np.nan, np.inf):
        X2 = X.copy()
        X2[321, 9] = v
        assert not np.isfinite(api.plda_stats(ctx, X2, lab, 7)["sw"]).all()   # not singled out by the library ...
        with pytest.raises(ValueError, match="row 321"):                       # ... named by the Python layer
            plda.class_stats(X2, lab, 7, ctx=ctx)
        with pytest.raises(ValueError, match="row 321"):
            plda.Plda(ctx=ctx).fit(X2, lab)
    again = api.plda_stats(ctx, X, lab, 7)
    assert all(np.array_equal(base[k], again[k]) for k in ("sum", "count", "mean", "sw"))


# -------------------------------------------------------------------------------------------------------------------------- scorer
def _scorer(ctx, g, flags=0):
    from speech_signal_processing_amd import api
    return api.PldaScorer(ctx, g["psi"], g["enrol"], g["counts"], flags=flags)


def _runs(g):
    """flags of the runs of a case: every case with G <= 32 runs a second time with the class-shared path switched off"""
    return (0, 1) if g["G"] <= 32 else (0,)


@pytest.mark.parametrize("case", PO.SCORER_CASES, ids=lambda c: "q%d-S%d-N%d-G%d-x%g" % c[:5])
def test_scores_and_decisions(ctx, case):
    g = PO.scorer_case(case)
    ref, bound = g["ref"], PO.llr_bound(g["ref"])
    for flags in _runs(g):
        sc = _scorer(ctx, g, flags)
        assert sc.n_classes == g["G"] and sc.class_shared == (g["G"] <= 32 and not flags)   # (read back from the handle)
        got = sc.score(g["T"], llr=True)
        assert got["llr"].shape == ref.shape and got["llr"].dtype == np.float32 and got["argmax"].dtype == np.int32
        err = np.abs(got["llr"].astype(np.float64) - ref).max(axis=1)
        print("[measured] %s flags %d: max err %.3g of the bound, %d rows left out" % (case, flags, (err / bound).max(), int((~g["keep"]).sum())))
        assert (err <= bound).all(), (flags, float((err / bound).max()))
        keep = g["keep"]
        assert np.array_equal(got["argmax"][keep], ref.argmax(axis=1)[keep])
        # max is llr[argmax] bit for bit, the arg-max is the FIRST index of the row's maximum
        rows = np.arange(ref.shape[0])
        assert np.array_equal(got["max"], got["llr"][rows, got["argmax"]])
        assert np.array_equal(got["argmax"], got["llr"].argmax(axis=1))
        lean = sc.score(g["T"])
        assert set(lean) == {"argmax", "max"}
        assert np.array_equal(lean["argmax"], got["argmax"]) and np.array_equal(lean["max"], got["max"])


def test_argmax_ties_go_to_the_first_index(ctx):
    g = PO.scorer_case(PO.SCORER_CASES[3])
    dup = dict(g, enrol=np.concatenate([g["enrol"], g["enrol"]]), counts=np.concatenate([g["counts"], g["counts"]]))
    S = g["enrol"].shape[0]
    for flags in (0, 1):
        got = _scorer(ctx, dup, flags).score(g["T"], llr=True)
        assert np.array_equal(got["llr"][:, :S], got["llr"][:, S:])
        assert (got["argmax"] < S).all()


@pytest.mark.parametrize("idx", [8, 4, 2], ids=["q256-G32", "q64-G40", "q5-G40"])
def test_a_rows_bits_depend_on_neither_the_batch_nor_its_place(ctx, idx):
    g = PO.scorer_case(PO.SCORER_CASES[idx])
    T = g["T"]
    N = T.shape[0]
    for flags in _runs(g):
        sc = _scorer(ctx, g, flags)
        full = sc.score(T, llr=True)
        rolled = sc.score(np.roll(T, 37, axis=0), llr=True)
        for k in ("llr", "argmax", "max"):
            assert np.array_equal(np.roll(rolled[k], -37, axis=0), full[k]), (flags, k)
        for r in (0, 31, 32, 127, 128, N - 1):
            alone = sc.score(T[r:r + 1], llr=True)
            for k in ("llr", "argmax", "max"):
                assert np.array_equal(alone[k][0], full[k][r]), (flags, r, k)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_test_vector(ctx, value):
    """NaN in its own llr row and in max, -1 in argmax; every other row bit-identical to the call with that row replaced by zeros"""
    for idx in (9, 4):
        g = PO.scorer_case(PO.SCORER_CASES[idx])
        T = g["T"].copy()
        r, q = 40, T.shape[1]
        T[r, q - 3] = value
        zeros = T.copy()
        zeros[r] = 0.0
        for flags in _runs(g):
            sc = _scorer(ctx, g, flags)
            got, want = sc.score(T, llr=True), sc.score(zeros, llr=True)
            assert np.isnan(got["llr"][r]).all() and np.isnan(got["max"][r]) and got["argmax"][r] == -1
            others = np.arange(T.shape[0]) != r
            for k in ("llr", "argmax", "max"):
                assert np.array_equal(got[k][others], want[k][others]), (flags, k)
            assert np.isfinite(want["llr"]).all() and want["argmax"][r] >= 0


def test_device_arrays_give_the_host_calls_bits(ctx):
    import torch
    g = PO.scorer_case(PO.SCORER_CASES[8])
    sc = _scorer(ctx, g)
    host = sc.score(g["T"], llr=True)
    dev = sc.score(torch.from_numpy(g["T"]).cuda(), llr=True)
    for k in ("llr", "argmax", "max"):
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), host[k])


def test_scorer_error_codes_and_the_ctx_stays_usable(ctx):
    from speech_signal_processing_amd import _lib, api
    g = PO.scorer_case(PO.SCORER_CASES[1])
    sc = _scorer(ctx, g)
    base = sc.score(g["T"], llr=True)
    with pytest.raises(ValueError):
        sc.score(g["T"][:, :-1])
    out = np.empty(4, np.int32)
    lib = ctx._lib
    assert lib.ssp_plda_score(sc._h, g["T"].ctypes.data, -1, None, out.ctypes.data, None, _lib.HOST, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_plda_score(sc._h, g["T"].ctypes.data, 4, None, out.ctypes.data, None, 7, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_plda_score(sc._h, None, 4, None, out.ctypes.data, None, _lib.HOST, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_plda_score(None, g["T"].ctypes.data, 4, None, out.ctypes.data, None, _lib.HOST, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_plda_score(sc._h, g["T"].ctypes.data, 0, None, out.ctypes.data, None, _lib.HOST, None) == _lib.SSP_OK
    for bad in ((np.array([1.0, -0.5]), np.zeros((2, 2)), [1, 1]), (np.array([1.0, 0.5]), np.zeros((2, 2)), [1, 0]),
                (np.array([1.0, np.nan]), np.zeros((2, 2)), [1, 1]), (np.array([1.0, 0.5]), np.full((2, 2), np.inf), [1, 1])):
        with pytest.raises(ValueError):
            api.PldaScorer(ctx, *bad)
    with pytest.raises(NotImplementedError):
        api.PldaScorer(ctx, np.ones(257), np.zeros((1, 257)), [1])
    h = C.c_void_p()
    assert lib.ssp_plda_pack(ctx._h, 2, None, 1, None, None, 0, C.byref(h)) == _lib.SSP_ERR_INVALID and not h.value
    again = sc.score(g["T"], llr=True)
    assert all(np.array_equal(base[k], again[k]) for k in base)
    sc.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------------------------- end to end
def test_fit_enroll_identify_save_load(ctx, tmp_path):
    from speech_signal_processing_amd import plda
    e = PO.end_to_end_case()
    (Xtr, ltr), (Xen, len_), (Xte, lte) = e["train"], e["enrol"], e["test"]
    S = e["S"]
    model = plda.Plda(n_iter=5, ctx=ctx).fit(Xtr, ltr)
    # the oracle: its own statistics of its own float64 front end, its own EM
    raw = PO.class_stats(Xtr, ltr, S)
    st = PO.class_stats(PO.front(Xtr, raw["mean"]).astype(np.float32), ltr, S)
    W, B, obj = PO.em(st["sw"], st["class_mean"], st["count"], st["mean"], 5)
    ew, eb = np.abs(model.within_ - W).max() / np.abs(W).max(), np.abs(model.between_ - B).max() / np.abs(B).max()
    print("[measured] end to end: W %.3g, B %.3g of max|.|" % (ew, eb))
    assert ew <= 1e-3 and eb <= 1e-3
    assert model.objective_.shape == (5,) and (np.diff(model.objective_) >= 0).all()
    assert np.array_equal(model.mean_, raw["mean"]) and model.lda_ is None
    A, psi = PO.diagonalise(W, B)
    assert np.abs(model.psi_ - psi).max() <= 1e-3 * psi.max()

    def proj(X):
        return (PO.front(X, raw["mean"]) - st["mean"]) @ A.T
    Ten = proj(Xen)
    enrol = np.stack([Ten[len_ == s].mean(axis=0) for s in range(S)])
    ref = PO.llr_direct(psi, enrol, np.bincount(len_, minlength=S), proj(Xte))
    keep = PO.decided_rows(ref)
    scorer = model.enroll(Xen, len_, S)
    got = model.score(scorer, Xte, llr=True)
    who = model.identify(scorer, Xte)
    assert who.dtype == np.int32 and np.array_equal(who, got["argmax"])
    print("[measured] end to end: %d of %d rows decided, accuracy %.3f, llr err %.3g of the bound" % (
        int(keep.sum()), keep.size, float((who == lte).mean()), (np.abs(got["llr"] - ref).max(axis=1) / PO.llr_bound(ref)).max()))
    assert keep.mean() >= 1.0 - PO.EXCLUSION_CAP
    assert np.array_equal(who[keep], ref.argmax(axis=1)[keep])
    model.save(str(tmp_path / "m"))
    back = plda.Plda.load(str(tmp_path / "m"), ctx=ctx)
    got2 = back.score(back.enroll(Xen, len_, S), Xte, llr=True)
    assert all(np.array_equal(got[k], got2[k]) for k in ("llr", "argmax", "max"))


def test_lda_front_end_on_the_device(ctx):
    """Plda with lda_dim: the projection is the oracle's LDA of the device's statistics, project() lands in the diagonalised space"""
    from speech_signal_processing_amd import plda
    e = PO.end_to_end_case()
    Xtr, ltr = e["train"]
    S, p = e["S"], 10
    model = plda.Plda(n_iter=3, lda_dim=p, ctx=ctx).fit(Xtr, ltr)
    raw = PO.class_stats(Xtr, ltr, S)
    V, lam, _ = PO.lda(raw["sw"], raw["class_mean"], raw["count"], raw["mean"], p)
    # (the device's S_w is within 1e-4 max|S_w| of the oracle's; the eigenvectors get the end-to-end bound of W and B)
    assert model.lda_.shape == (e["q"], p) and np.abs(model.lda_ - V).max() <= 1e-3 * np.abs(V).max()
    Y = PO.front(Xtr, raw["mean"], V)
    want = (Y - model.plda_mean_) @ model.transform_.T
    got = model.project(Xtr)
    assert got.dtype == np.float32 and got.shape == (Xtr.shape[0], p)
    # fp32 GEMMs and a normalisation of the SAME model against float64: the project's feature rule
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    lda = plda.Lda(p, ctx=ctx).fit(Xtr, ltr)
    flat = (Xtr.astype(np.float64) - lda.mean_) @ lda.components_
    assert np.abs(lda.transform(Xtr) - flat).max() <= 1e-4 * max(1.0, np.abs(flat).max())
    assert np.array_equal(lda.components_, model.lda_)


def test_the_model_takes_device_arrays(ctx):
    """fit, enroll and identify on torch CUDA tensors: the host route's model and decisions, bit for bit"""
    import torch
    from speech_signal_processing_amd import plda
    e = PO.end_to_end_case()
    (Xtr, ltr), (Xen, len_), (Xte, _) = e["train"], e["enrol"], e["test"]
    host = plda.Plda(n_iter=2, ctx=ctx).fit(Xtr, ltr)
    dev = plda.Plda(n_iter=2, ctx=ctx).fit(torch.from_numpy(Xtr).cuda(), torch.from_numpy(ltr).cuda())
    assert np.array_equal(host.within_, dev.within_) and np.array_equal(host.transform_, dev.transform_)
    want = host.score(host.enroll(Xen, len_, e["S"]), Xte, llr=True)
    got = dev.score(dev.enroll(torch.from_numpy(Xen).cuda(), len_, e["S"]), torch.from_numpy(Xte).cuda(), llr=True)
    for k in ("llr", "argmax", "max"):
        assert got[k].is_cuda and np.array_equal(got[k].cpu().numpy(), want[k])
