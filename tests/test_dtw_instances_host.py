"""The yardstick of tests/test_dtw_instances_gpu.py checked on the CPU (tests/dtw_cases.py): the float32 restatement stays inside the
derived band against float64 at every instance's largest shape, the exact inputs are exact, the batched sweep is the oracle's, the
non-finite table is what the float64 oracle answers, and pick_w restates the dispatch of ssp_dtw_distances on both sides of every
threshold.  (The names of the compiled instances are checked in tests/test_dtw_instances_isa.py, which needs the compiler.)"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_cases as K  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

# one pair per instance at its largest shape (longest query x 64 W columns; W = 32 also beyond one super-block), at dim 1, 3 and 13
LARGEST = [(1, 130, 64 * w) for w in K.W_DIM1] + [(3, 130, 64 * w) for w in K.W_DIMN] + [(13, 130, 256), (1, 70, 6145), (3, 70, 6145)]


@pytest.mark.parametrize("dim,r,c", LARGEST, ids=["dim%d_%dx%d" % s for s in LARGEST])
def test_emu32_stays_inside_the_band_and_exact_inputs_are_exact(dim, r, c):
    x, y = K.gaussian(r, dim, 1), K.gaussian(c, dim, 2)
    ref, emu = K.ref64(x, y), K.emu32(x, y)
    b = K.band(r, c, dim, ref)
    ratio = abs(float(emu) - ref) / b
    print("dtw_band dim=%d r=%d c=%d ref=%.6g emu32 error / band = %.4f" % (dim, r, c, ref, ratio))
    assert emu.dtype == np.float32 and ref > 0 and ratio <= 1.0, (dim, r, c, ratio)
    xe, ye = K.exact(r, dim, 1), K.exact(c, dim, 2)
    ref, emu = K.ref64(xe, ye), K.emu32(xe, ye)
    assert ref == float(emu) and ref == int(ref) and 0 < ref < 2 ** 24, (dim, r, c, ref, emu)
    if dim > 1:
        assert ref % 5 == 0 and np.count_nonzero(xe[:, 2:]) == 0


def test_the_batched_sweep_is_the_oracles():
    """ref64_matrix / emu32_matrix pad a query's templates to one shape: the same bits as the pair by itself"""
    for dim in (1, 3, 13):
        Q = [K.gaussian(n, dim, 10 + n) for n in (1, 7, 40)]
        T = [K.gaussian(n, dim, 20 + n) for n in (1, 5, 66, 31)]
        ref, emu = K.ref64_matrix(Q, T), K.emu32_matrix(Q, T)
        assert ref.dtype == np.float64 and emu.dtype == np.float32
        for a, q in enumerate(Q):
            for b, t in enumerate(T):
                assert ref[a, b] == O.dtw_distance(q, t) == K.ref64(q, t), (dim, a, b)
                assert emu[a, b] == K.emu32(q, t), (dim, a, b)
                assert K.ref64(q, t, True) == O.dtw_distance(q, t) / (len(q) + len(t))
    # one hand-made pair: x = (0, 2), y = (0, 1, 2) -> costs [[0, 1, 2], [2, 1, 0]], the path 0 + 1 + 0
    assert K.ref64([0, 2], [0, 1, 2]) == 1.0 and K.emu32([0, 2], [0, 1, 2]) == np.float32(1.0)
    assert K.ref64([[0, 0], [3, 4]], [[0, 0], [0, 0], [3, 4]]) == 0.0
    assert K.ref64([[3, 4]], [[0, 0], [6, 8]]) == 10.0


@pytest.mark.parametrize("dim", (1, 3))
def test_non_finite_table_is_what_float64_answers(dim):
    """NaN anywhere -> NaN; an infinity on one side -> +inf; the same infinity in the same coordinate on both sides -> NaN (inf - inf);
    opposite infinities -> +inf.  The place of the bad element does not matter — the property the kernels' minima did not have."""
    q, t, cases = K.nonfinite_pairs(dim)
    assert np.isfinite(K.ref64(q, t))
    assert len(cases) == 10
    for name, qq, tt, want in cases:
        assert K.same_float(K.ref64(qq, tt), want), (dim, name, K.ref64(qq, tt), want)
        assert K.same_float(K.ref64(qq, tt, True), want), (dim, name)
        assert not (np.isfinite(qq).all() and np.isfinite(tt).all()), name
    # a long template: the bad element in its first super-block and in its second
    for at in (1000, 2048):
        _, _, long_cases = K.nonfinite_pairs(dim, r=9, c=2049, t_rows={"first": at, "mid": at, "last": at})
        for name, qq, tt, want in long_cases:
            assert K.same_float(K.ref64(qq, tt), want), (dim, at, name)
    # at dim > 1 the infinities must share the coordinate to cancel
    if dim > 1:
        assert K.ref64(K.put(q, "mid", K.INF, coord=0), K.put(t, "mid", K.INF, coord=2)) == np.inf
    # numpy's arg-min picks a NaN: a polluted template wins whatever the place of the NaN (the reference's classify)
    assert np.array([1.0, np.nan, 0.5]).argmin() == 1


def test_pick_w_on_both_sides_of_every_threshold():
    assert K.INSTANCES == [("dtw1_kernel", w) for w in (4, 8, 12, 16, 20, 24, 32)] + [("dtw_kernel", w) for w in (4, 8, 16, 32)]
    limits1 = {4: 256, 8: 512, 12: 768, 16: 1024, 20: 1280, 24: 1536}
    limitsn = {4: 256, 8: 512, 16: 1024}
    for dim, limits in ((1, limits1), (3, limitsn), (13, limitsn)):
        ws = K.widths(dim)
        assert K.pick_w(dim, 0) == 4 and K.pick_w(dim, 1) == 4
        for k, w in enumerate(ws[:-1]):
            assert K.pick_w(dim, limits[w]) == w and K.pick_w(dim, limits[w] - 1) == w and K.pick_w(dim, limits[w] + 1) == ws[k + 1], (dim, w)
            assert K.lo_of(dim, ws[k + 1]) == limits[w] + 1
        for c in (2048, 2049, 4096, 6145, 10 ** 6):
            assert K.pick_w(dim, c) == 32
        for w in ws:
            lens = K.template_lens(dim, w)
            assert K.pick_w(dim, max(lens)) == w and lens[-1] == 64 * w == max(lens) and lens[-2] == 64 * w - 1
            low = [lens[k] for k in K.low_edge_templates(dim, w)]
            assert max(low) == K.lo_of(dim, w) and K.pick_w(dim, max(low)) == w, (dim, w, low)
            assert w == 4 or K.pick_w(dim, max(low) - 1) != w


def test_fuzz_tool_restates_the_band():
    """tools/fuzz_scoring.py carries the band as one line of its own (it imports nothing from tests/): the same numbers as K.band"""
    src = open(os.path.join(K.ROOT, "tools", "fuzz_scoring.py")).read()
    m = re.search(r"^dtw_band = (lambda r, c, dim, ref: .*)$", src, re.M)
    assert m and "rtol=1e-4, atol=1e-4), (case, \"dtw\"" not in src
    f = eval(m.group(1), {})
    for r, c, dim, ref in ((1, 1, 1, 0.5), (130, 2048, 1, 1437.67), (70, 6145, 3, -10015.0), (9, 7, 13, 3.0), (5, 5, 2, 0.0)):
        assert f(r, c, dim, ref) == K.band(r, c, dim, ref), (r, c, dim, ref)


def test_pick_w_restates_the_host_code():
    """the two ladders of ssp_dtw_distances as they stand in csrc/dtw.hip, read from the source"""
    src = open(os.path.join(K.ROOT, "speech_signal_processing_amd", "csrc", "dtw.hip")).read()
    ladders = re.findall(r"W = ((?:need <= \d+ \? \d+ : )+)32;", src)
    assert len(ladders) == 2, ladders
    got = sorted(tuple(int(a) for a, b in re.findall(r"need <= (\d+) \? (\d+)", lad) if a == b) for lad in ladders)
    assert got == sorted([K.W_DIM1[:-1], K.W_DIMN[:-1]]), got
    assert "(max_c + 63) / 64" in src
