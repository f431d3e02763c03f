"""The yardsticks of tests/test_gmm_instances_gpu.py, checked without a GPU (tests/gmm_cases.py): emu32 — the float32 restatement of the
scoring kernel's formula that the GPU results are measured against — stays finite and inside a rigorous forward bound on every case; the
sweep's feature widths reach every compiled instance on both edges of its range; every sweep utterance is decided by more than the
comparison can be off; and the comparison has teeth: a model that is wrong by a hundredth of a standard deviation in ONE mean entry of
ONE mixture fails it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_cases as G  # noqa: E402


def all_cases():
    for D in G.SWEEP_D:
        yield G.sweep_case(D)
    for K, D in G.HARD_SHAPES:
        for kind in G.HARD_KINDS:
            yield G.hard_case(kind, K, D)
    for D in (39, 13):
        yield G.late_dominant_case(D)
    for name in G.ZERO_PATTERNS:
        yield G.zero_weight_case(name)[0]


def test_emu32_is_finite_and_inside_its_forward_bound_on_every_case():
    worst = 0.0
    for c in all_cases():
        assert np.isfinite(c["ref_ll"]).all(), c["name"]
        assert np.isfinite(c["emu_ll"]).all(), c["name"]
        bound = G.emu32_forward_bound(c["w"], c["mus"], c["cov"], c["X"], c["ref_ll"])
        used = float((np.abs(c["emu_ll"] - c["ref_ll"]) / bound).max())
        worst = max(worst, used)
        assert used <= 1.0, (c["name"], "emu32 uses %.3f of its forward bound" % used)
        # the oracle's two entry points agree: gmm_score is the mean of gmm_score_samples
        sc = G.ref64_scores(c["w"], c["mus"], c["cov"], c["X"], c["lens"])
        nz = np.asarray(c["lens"]) > 0
        assert np.isnan(sc[~nz]).all() and np.isnan(c["ref_sc"][~nz]).all()
        # (to float64 noise of the expanded quadratic form, whose BLAS summation order depends on the number of rows)
        assert np.allclose(sc[nz], c["ref_sc"][nz], rtol=1e-9, atol=0)
    print("emu32 uses at most %.3f of its forward bound" % worst)


def test_the_sweep_reaches_every_instance_on_both_edges_of_its_range():
    """pick_nq / the NK table restated from csrc/gmm.hip; the issue's table of ranges: NQ 4 <= 15, 7 <= 27, 10 <= 39, 16 <= 63, 24 <= 95,
    32 <= 127; NK 1 <= 8, 2 <= 16, 3 <= 24, 4 <= 32, 5 <= 40, 6 <= 48, 8 <= 64"""
    nq_hi = {4: 15, 7: 27, 10: 39, 16: 63, 24: 95, 32: 127}
    nk_hi = {1: 8, 2: 16, 3: 24, 4: 32, 5: 40, 6: 48, 8: 64}
    for table, pick, top in ((nq_hi, G.pick_nq, 127), (nk_hi, G.pick_nk, 64)):
        lo = 1
        for inst in sorted(table):
            hi = table[inst]
            assert all(pick(D) == inst for D in range(lo, hi + 1)), (inst, lo, hi)
            ds = [D for D in G.SWEEP_D if pick(D) == inst]
            assert len(ds) >= 2 and min(ds) == lo and max(ds) == hi, (inst, ds, lo, hi)
            lo = hi + 1
        assert lo == top + 1
    assert G.pick_nq(128) == -1 and G.pick_nk(65) == 0
    assert G.piece_granule(63, False) == 64 and G.piece_granule(64, False) == 32 and G.piece_granule(64, True) == 64
    # the zero k-step of NK 8 (D 49 .. 56: 2 D <= 112 of 128 columns) is in the sweep
    assert {49, 56} <= set(G.SWEEP_D)
    # every K of the rotation, both M, and an odd number of row tiles under the bf16 kernel's groups of two
    shapes = [G.sweep_shape(D) for D in G.SWEEP_D]
    assert {s[0] for s in shapes} == set(G.SWEEP_K) and {s[1:] for s in shapes} == {(3, True), (2, False)}
    assert any(M * ((K + 31) // 32) % 2 == 1 for (K, M, _), D in zip(shapes, G.SWEEP_D) if D <= 64)
    assert G.sweep_shape(39) == (64, 3, True)


@pytest.mark.parametrize("D", G.SWEEP_D)
def test_every_sweep_utterance_is_decided_and_the_true_speaker_wins(D):
    c = G.sweep_case(D)
    ok, left_out = G.construction_ok(c)
    assert ok and left_out == 0.0, (D, c["seed"], left_out)
    nz = np.asarray(c["lens"]) > 0
    assert np.array_equal(c["ref_am"][nz], c["speaker"][nz])
    # every model has parameters of its own
    for a in (c["w"], c["mus"], c["cov"]):
        if c["K"] > 1 or a.ndim == 3:
            assert all(not np.array_equal(a[i], a[j]) for i in range(c["M"]) for j in range(i))


def test_the_comparison_passes_emu32_in_another_order_and_fails_a_hundredth_of_a_sigma():
    c = G.sweep_case(39)
    assert (c["K"], c["D"]) == (64, 39)
    # a second float32 evaluation of the same formula (the terms summed in reverse order) passes, with room
    aug = np.concatenate([c["X"], c["X"] * c["X"], np.ones((len(c["X"]), 1), np.float32)], axis=1)
    alt = np.empty_like(c["emu_ll"])
    for m in range(c["M"]):
        W = G.pack_w(c["w"][m], c["mus"][m], c["cov"][m]).astype(np.float32)
        acc = np.zeros((len(c["X"]), c["K"]), np.float32)
        for j in reversed(range(2 * c["D"] + 1)):
            acc = acc + aug[:, j:j + 1] * W[None, :, j]
        mx = acc.max(axis=1, keepdims=True)
        alt[m] = (mx[:, 0] + np.log2(np.exp2(acc - mx).sum(axis=1, dtype=np.float32))) * G.LN2_F32
    r = G.compare(alt, c["ref_ll"], c["emu_ll"], "reverse order")
    print("reverse-order float32 evaluation:", r)
    assert r["max_ratio"] < 0.5 and r["rms_ratio"] < 0.7
    # the mutation
    mus = G.shifted_models(c, 0.01)
    bad_ll = G.emu32_loglik(c["w"], mus, c["cov"], c["X"])
    moved = np.abs(G.ref64_loglik(c["w"], mus, c["cov"], c["X"]) - c["ref_ll"])
    assert (moved > 4 * G.entry_tolerance(c["ref_ll"], c["emu_ll"])).any()
    with pytest.raises(AssertionError, match="x its limit"):
        G.compare(bad_ll, c["ref_ll"], c["emu_ll"], "shifted per-frame")
