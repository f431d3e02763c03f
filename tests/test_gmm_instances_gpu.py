"""Every compiled instance of the GMM scorer (csrc/gmm.hip: NQ 4 .. 32 of the fp32 kernel, NK 1 .. 8 of the bf16x3 kernel, each fused and
un-fused) against float64, on both edges of the feature widths it covers, and precision 0 / 2 off the well-conditioned case.

The yardstick is tests/gmm_cases.py: ref64 (the oracle), emu32 (a float32 numpy restatement of the kernel's formula) and ONE comparison,
  max |got - ref64| <= 8 max|emu32 - ref64| + 2^-20 (|ref64| + 1),  rms(got - ref64) <= 3 rms(emu32 - ref64) + 2^-22 (rms|ref64| + 1);
precision 2 is held per entry to the bound of include/ssp.h.  tests/test_gmm_instances_host.py checks the yardstick itself.  Every test
prints what it measured as a `gmm_accuracy {json}` line (pytest -s); profiles/gmm_accuracy.md is made of those lines."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from speech_signal_processing_amd import api
    return api


def record(**kw):
    print("gmm_accuracy " + json.dumps({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in kw.items()}))


def scorer_of(api, c, w=None, mus=None):
    ctx = api.default_context()
    sc = api.GmmScorer(ctx, c["w"] if w is None else w, c["mus"] if mus is None else mus, c["cov"], has_ubm=c["ubm"])
    return sc, api.Segments.from_lengths(ctx, c["lens"])


def run_both(sc, seg, c, precision):
    """the un-fused launch (loglik=True: the [M x F] matrix, per-utterance means by the reduce kernel) and the fused one, as host arrays"""
    un = {k: np.asarray(v) for k, v in sc.score(c["X"], seg, loglik=True, precision=precision).items()}
    fu = {k: np.asarray(v) for k, v in sc.score(c["X"], seg, precision=precision).items()}
    assert un["loglik"].shape == c["ref_ll"].shape and un["scores"].shape == fu["scores"].shape == c["ref_sc"].shape
    return un, fu


def check_empty_and_fused_mean(c, un, fu, what):
    lens = np.asarray(c["lens"])
    for r, launch in ((un, "un-fused"), (fu, "fused")):
        assert np.isnan(r["scores"][lens == 0]).all(), (what, launch, "an empty utterance's row is not NaN")
        assert (r["argmax"][lens == 0] == 0).all(), (what, launch, "an empty utterance's arg-max is not 0")
        assert np.isfinite(r["scores"][lens > 0]).all(), (what, launch)
    # the fused scores are float64 piece sums of the same per-frame values: the float32 rounding of a float64 mean
    mean32 = G.utt_means(un["loglik"], c["lens"], np.float32)[lens > 0]
    assert (np.abs(fu["scores"][lens > 0] - mean32) <= np.spacing(np.abs(mean32))).all(), (what, "fused scores against the mean of loglik")


def check_precision0(c, un, fu, what, instance):
    """every loglik and scores entry by the comparison; returns nothing, prints the ratios"""
    r_ll = G.compare(un["loglik"], c["ref_ll"], c["emu_ll"], "%s loglik" % what)
    r_un = G.compare(un["scores"], c["ref_sc"], c["emu_sc"], "%s un-fused scores" % what)
    r_fu = G.compare(fu["scores"], c["ref_sc"], c["emu_sc"], "%s fused scores" % what)
    check_empty_and_fused_mean(c, un, fu, what)
    for launch, r in (("un-fused loglik", r_ll), ("un-fused scores", r_un), ("fused scores", r_fu)):
        record(case=c["name"], K=c["K"], D=c["D"], precision=0, instance=instance, launch=launch, max_ratio=r["max_ratio"],
               rms_ratio=r["rms_ratio"], max_vs_emu=r["max_vs_emu"], rms_vs_emu=r["rms_vs_emu"], max_err=float("%.3e" % r["max_err"]),
               emu_max_err=float("%.3e" % r["emu_max_err"]))
    return r_ll


def check_precision2(c, un, fu, what, instance):
    bound = G.bf16x3_bound(c["w"], c["mus"], c["cov"], c["X"], c["ref_ll"])
    sbound = G.utt_means(bound, c["lens"])
    b_ll = G.compare_bound(un["loglik"], c["ref_ll"], bound, "%s loglik" % what)
    b_un = G.compare_bound(un["scores"], c["ref_sc"], sbound, "%s un-fused scores" % what)
    b_fu = G.compare_bound(fu["scores"], c["ref_sc"], sbound, "%s fused scores" % what)
    check_empty_and_fused_mean(c, un, fu, what)
    fin = np.isfinite(c["ref_ll"])
    err = np.abs(un["loglik"] - c["ref_ll"])[fin]
    eerr = np.abs(c["emu_ll"] - c["ref_ll"])[fin]
    record(case=c["name"], K=c["K"], D=c["D"], precision=2, instance=instance, launch="un-fused loglik | un-fused scores | fused scores",
           error_over_bound=[float("%.4g" % b) for b in (b_ll, b_un, b_fu)], max_err=float("%.3e" % err.max()),
           max_vs_emu=float(err.max() / max(eerr.max(), 1e-300)))


# ------------------------------------------------------------------------------------------------- the instance sweep
@pytest.mark.parametrize("D", G.SWEEP_D)
def test_instance_sweep(api, D):
    c = G.sweep_case(D)
    nq, nk = G.pick_nq(D), G.pick_nk(D)
    inst0 = "fp32 NQ=%d CT=%d" % (nq, 2 if nq <= 16 else 1)
    sc, seg = scorer_of(api, c)
    nz = np.asarray(c["lens"]) > 0
    un0, fu0 = run_both(sc, seg, c, 0)
    print("instance list: D=%d K=%d M=%d ubm=%d: %s un-fused, %s fused (granule %d)" % (D, c["K"], c["M"], c["ubm"], inst0, inst0,
                                                                                       G.piece_granule(D, False)))
    check_precision0(c, un0, fu0, "D=%d precision 0" % D, inst0)
    assert np.array_equal(un0["argmax"], c["ref_am"]) and np.array_equal(fu0["argmax"], c["ref_am"]), (D, un0["argmax"], fu0["argmax"])
    if nk:
        inst2 = "bf16x3 NK=%d CT=2" % nk
        un2, fu2 = run_both(sc, seg, c, 2)
        print("instance list: D=%d K=%d M=%d ubm=%d: %s un-fused, %s fused (granule 64, %d row tiles)"
              % (D, c["K"], c["M"], c["ubm"], inst2, inst2, c["M"] * ((c["K"] + 31) // 32)))
        check_precision2(c, un2, fu2, "D=%d precision 2" % D, inst2)
        assert np.array_equal(un2["argmax"], c["ref_am"]) and np.array_equal(fu2["argmax"], c["ref_am"]), (D, un2["argmax"], fu2["argmax"])
        # precision 1: the bf16x3 pass with the close calls scored again in fp32 — the arg-max is precision 0's
        r1 = sc.score(c["X"], seg, precision=1)
        assert np.array_equal(np.asarray(r1["argmax"]), fu0["argmax"]), D
        sb = G.utt_means(G.bf16x3_bound(c["w"], c["mus"], c["cov"], c["X"], c["ref_ll"]), c["lens"])
        G.compare_bound(np.asarray(r1["scores"]), c["ref_sc"], np.maximum(sb, G.entry_tolerance(c["ref_sc"], c["emu_sc"])), "D=%d precision 1" % D)
    else:
        for precision in (1, 2, 3):
            for loglik in (False, True):
                with pytest.raises(NotImplementedError, match="D <= 64"):
                    sc.score(c["X"], seg, loglik=loglik, precision=precision)
        after = {k: np.asarray(v) for k, v in sc.score(c["X"], seg, precision=0).items()}   # a refused call leaves nothing behind
        assert np.array_equal(after["scores"][nz], fu0["scores"][nz]) and np.array_equal(after["argmax"], fu0["argmax"])


def test_D_128_is_refused_at_pack(api):
    rng = np.random.default_rng(128)
    w, mus, cov = G._draw_models(rng, 4, 128, 2, 0.3)
    with pytest.raises(NotImplementedError, match="127"):
        api.GmmScorer(api.default_context(), w, mus, cov, has_ubm=False)


def test_a_mean_entry_off_by_a_hundredth_of_a_sigma_fails_the_comparison(api):
    """the teeth of the comparison, on the card: the GPU scores the K = 64, D = 39 sweep case with ONE mean entry of ONE mixture of ONE
    model moved by 0.01 sigma, the oracle and emu32 the unshifted case"""
    c = G.sweep_case(39)
    sc, seg = scorer_of(api, c, mus=G.shifted_models(c, 0.01))
    un, _ = run_both(sc, seg, c, 0)
    with pytest.raises(AssertionError, match="x its limit"):
        G.compare(un["loglik"], c["ref_ll"], c["emu_ll"], "shifted")
    # the other two models are untouched by it and still pass
    keep = [i for i in range(c["M"]) if i != 1]
    G.compare(un["loglik"][keep], c["ref_ll"][keep], c["emu_ll"][keep], "the unshifted models")


# ------------------------------------------------------------------------------------------------- off the easy case
HARD = [(kind, K, D) for (K, D) in G.HARD_SHAPES for kind in G.HARD_KINDS] + [("late_dominant", 70, 39), ("late_dominant", 70, 13)]


@pytest.mark.parametrize("kind,K,D", HARD, ids=["%s_K%d_D%d" % h for h in HARD])
def test_off_the_easy_case(api, kind, K, D):
    c = G.late_dominant_case(D) if kind == "late_dominant" else G.hard_case(kind, K, D)
    sc, seg = scorer_of(api, c)
    un0, fu0 = run_both(sc, seg, c, 0)
    assert np.isfinite(un0["loglik"]).all(), (kind, K, D, "precision 0 is not finite")
    r = check_precision0(c, un0, fu0, "%s precision 0" % c["name"], "fp32 NQ=%d" % G.pick_nq(D))
    un2, fu2 = run_both(sc, seg, c, 2)
    assert np.isfinite(un2["loglik"]).all(), (kind, K, D, "precision 2 is not finite")
    check_precision2(c, un2, fu2, "%s precision 2" % c["name"], "bf16x3 NK=%d" % G.pick_nk(D))
    if "ratio" in c:
        record(table="mu_over_sigma", ratio=c["ratio"], K=K, D=D, max_abs_ll=float("%.4g" % np.abs(c["ref_ll"]).max()),
               gpu_max_err=float("%.3e" % r["max_err"]), emu_max_err=float("%.3e" % r["emu_max_err"]),
               gpu_rel=float("%.3e" % (r["max_err"] / np.abs(c["ref_ll"]).max())))


# ------------------------------------------------------------------------------------------------- zero weights
@pytest.mark.parametrize("name", sorted(G.ZERO_PATTERNS))
def test_zero_weights(api, name):
    """a mixture with weight 0 contributes nothing (sklearn and the oracle: log 0 = -inf inside a log-sum-exp): the model's
    log-likelihoods are the oracle's finite values at every precision, fused and un-fused, and the models without zeros do not change"""
    c, w0 = G.zero_weight_case(name)
    sc, seg = scorer_of(api, c)
    sc_before, _ = scorer_of(api, c, w=w0)
    nz = np.asarray(c["lens"]) > 0
    others = [0, 2]
    res = {}
    for precision in (0, 2):
        un, fu = run_both(sc, seg, c, precision)
        un_b, fu_b = run_both(sc_before, seg, c, precision)
        what = "%s precision %d" % (c["name"], precision)
        assert np.isfinite(un["loglik"]).all(), (what, "NaN or infinite log-likelihood", int((~np.isfinite(un["loglik"])).sum()))
        (check_precision0 if precision == 0 else check_precision2)(c, un, fu, what, "bf16x3 NK=%d" % G.pick_nk(c["D"]) if precision else
                                                                   "fp32 NQ=%d" % G.pick_nq(c["D"]))
        assert np.array_equal(un["loglik"][others], un_b["loglik"][others]), (what, "a model without zeros changed")
        assert np.array_equal(un["scores"][nz][:, others], un_b["scores"][nz][:, others]), what
        assert np.array_equal(fu["scores"][nz][:, others], fu_b["scores"][nz][:, others]), what
        res[precision] = (un, fu, un_b, fu_b)
    sbound = np.maximum(G.utt_means(G.bf16x3_bound(c["w"], c["mus"], c["cov"], c["X"], c["ref_ll"]), c["lens"]),
                        G.entry_tolerance(c["ref_sc"], c["emu_sc"]))
    for precision in (1, 3):
        what = "%s precision %d" % (c["name"], precision)
        # with loglik the call answers as precision 2 (include/ssp.h): the same bits
        un = {k: np.asarray(v) for k, v in sc.score(c["X"], seg, loglik=True, precision=precision).items()}
        assert np.array_equal(un["loglik"], res[2][0]["loglik"]) and np.array_equal(un["scores"][nz], res[2][0]["scores"][nz]), what
        # fused: every entry is the bf16x3 value or, where the utterance was a close call and the model a candidate, the fp32 one
        fu = {k: np.asarray(v) for k, v in sc.score(c["X"], seg, precision=precision).items()}
        fu_b = {k: np.asarray(v) for k, v in sc_before.score(c["X"], seg, precision=precision).items()}
        assert np.isfinite(fu["scores"][nz]).all() and np.isnan(fu["scores"][~nz]).all(), what
        G.compare_bound(fu["scores"], c["ref_sc"], sbound, what)
        f2, f0 = res[2][1]["scores"][nz], res[0][1]["scores"][nz]          # fused, with the zeros
        f2b, f0b = res[2][3]["scores"][nz], res[0][3]["scores"][nz]      # fused, before the zeros (the other models: the same bits)
        assert ((fu["scores"][nz] == f2) | (fu["scores"][nz] == f0)).all(), what
        assert ((fu_b["scores"][nz] == f2b) | (fu_b["scores"][nz] == f0b)).all(), what
        if precision == 1:   # the proven band: the arg-max is precision 0's
            assert np.array_equal(fu["argmax"], res[0][1]["argmax"]), (what, "arg-max differs from precision 0's")


def test_pack_refuses_weights_that_are_not_weights(api):
    """a negative or NaN weight, a model whose weights are all zero: SSP_ERR_INVALID before anything is uploaded"""
    c, _ = G.zero_weight_case("one_in_the_middle_K64")
    ctx = api.default_context()
    for bad, at in ((-0.25, (1, 5)), (np.nan, (2, 63)), (-0.0 - 1e-300, (0, 0))):
        w = c["w"].copy()
        w[at] = bad
        with pytest.raises(ValueError, match=r"model %d\b" % at[0]):
            api.GmmScorer(ctx, w, c["mus"], c["cov"], has_ubm=True)
    w = c["w"].copy()
    w[2] = 0.0
    with pytest.raises(ValueError, match=r"model 2\b"):
        api.GmmScorer(ctx, w, c["mus"], c["cov"], has_ubm=True)
    # the context is as good as before: the unchanged models pack and score
    sc, seg = scorer_of(api, c)
    r = sc.score(c["X"], seg, precision=0)
    assert np.array_equal(np.asarray(r["argmax"])[np.asarray(c["lens"]) == 0], [0, 0, 0])
