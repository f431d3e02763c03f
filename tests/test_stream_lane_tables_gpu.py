"""What the fixed-geometry instances of the wave-stream MFCC kernel read instead of recomputing (csrc/mfcc_stream_kernel.hpp, SSP_S_WTAB /
SSP_S_LADDR): the regression weights of the interior (transposed) time step come from a 39-entry table in LDS that every wave fills at
kernel start, and the lane parts of the DCT operand address, the ring store and the sample DMA offset stay in registers across the quad
loop.  Neither is arithmetic: the default launch must agree bit for bit with the run-time-geometry instance of the same kernel
(SSP_MFCC_STREAM_RUNTIME_GEO=1), which still forms every weight and every address where it is used.

The table is read by the steps whose 24-frame window lies strictly inside the utterance, so the shapes are chosen by how many such steps a
chunk has.  Which steps are interior is computed here from the kernel's own condition on the chunks the work table cuts (chunks_of mirrors
build_work_table's rule for this kernel in csrc/mfcc_plan.hip), never written down as numbers.  Order 1 unscaled has no fixed-geometry
instance and compares the run-time-geometry instance with itself, as in tests/test_stream_noops_gpu.py."""
import numpy as np
import pytest

from conftest import synth_audio

pytestmark = pytest.mark.gpu

FS, WIN, HOP = 16000, 400, 160
SWITCH = "SSP_MFCC_STREAM_RUNTIME_GEO"
ORDERS = [0, 1, 2]


def n_samples(frames):
    return WIN + HOP * (frames - 1)


def ceil_div(a, b):
    return -(-a // b)


def chunks_of(frames, num_cu):
    """(utterance, t0, n, pad) of every chunk the wave-stream kernel walks for a batch of these frame counts: whole utterances up to 512
    frames when the batch fills the machine (12 waves per CU), else cuts of a multiple of 16 frames, at least 32; cuts of a machine-filling
    batch start 12 frames further back than the 4-frame halo, and the utterances claimed last are cut in two"""
    total, want = sum(frames), num_cu * 12
    ch = min(max(max(frames), 1), 512)
    small = ceil_div(total, ch) < want
    if small:
        ch = min(ch, max(32, ceil_div(ceil_div(total, want), 16) * 16))
    tail_from = len(frames) - want if len(frames) >= 4 * want else len(frames)
    out = []
    for u, T in enumerate(frames):
        chu = min(ch, ceil_div((T + 1) // 2, 16) * 16) if (u >= tail_from and T >= 64) else ch
        for t0 in range(0, T, chu):
            out.append((u, t0, min(chu, T - t0), 0 if (small or t0 == 0) else 12))
    return out


def steps_of(T, t0, n, pad, order):
    """(ta, b, interior) of every time step of a chunk: the kernel's halo, step count and `interior` condition"""
    h = 4 if order > 0 else 0
    ta = max(t0 - (h + pad if order > 0 else 0), 0)
    e = t0 + n - ta
    return [(ta, b, ta + 16 * b - 8 >= 1 and ta + 16 * b + 16 <= T - 2) for b in range((e + 4 + 15) >> 4)]


def interior_counts(frames, num_cu, order):
    """per utterance: how many of its steps take the transposed form"""
    cnt = [0] * len(frames)
    for u, t0, n, pad in chunks_of(frames, num_cu):
        cnt[u] += sum(1 for _, _, inner in steps_of(frames[u], t0, n, pad, order) if inner)
    return cnt


@pytest.fixture(scope="module")
def ssp():
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import api
    return pkg, api


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_stream(api, tables, signals, ctx=None):
    ctx = ctx or api.default_context(torch_stream=False)
    plan = api.MfccPlan(ctx, tables)
    seg = api.Segments.from_lengths(ctx, [len(s) for s in signals])
    fseg = plan.frame_segments(seg)
    out = plan.run(np.concatenate(signals).astype(np.float32), seg, fseg, variant=3)
    return [np.array(out[fseg.offsets[i]:fseg.offsets[i + 1]]) for i in range(len(signals))]


def both(api, tables, signals, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    fixed = run_stream(api, tables, signals)
    monkeypatch.setenv(SWITCH, "1")
    runtime = run_stream(api, tables, signals)
    monkeypatch.delenv(SWITCH, raising=False)
    return fixed, runtime


def assert_same_bits(fixed, runtime, frames, order):
    for u, n in enumerate(frames):
        assert fixed[u].shape == (n, 13 * (1 + order)), (u, fixed[u].shape)
        assert np.isfinite(fixed[u]).all(), u
        assert np.array_equal(fixed[u], runtime[u]), "utterance %d (%d frames)" % (u, n)


SHORT = [1, 5, 23, 41, 42, 57, 58]  # around the lengths with no interior step and with exactly one
LONG = 298                          # the bench's utterance
CUT = 530                           # longer than the 512 frames a wave walks at most


def first_length_with(k, num_cu, order):
    """the shortest lone utterance with k interior steps"""
    return next(T for T in range(1, 1024) if interior_counts([T], num_cu, order)[0] >= k)


@pytest.fixture(scope="module")
def signals():
    cache = {}

    def get(frames):
        if frames not in cache:
            cache[frames] = synth_audio(frames, n_samples(frames), FS)
        return cache[frames]
    return get


@pytest.mark.parametrize("order", ORDERS)
def test_short_utterances(ssp, signals, num_cu, monkeypatch, order):
    pkg, api = ssp
    cnt = interior_counts(SHORT, num_cu, max(order, 1))
    assert 0 in cnt and 1 in cnt, cnt
    assert all(interior_counts([T], num_cu, max(order, 1))[0] == 0 for T in SHORT[:3])
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order), [signals(T) for T in SHORT], monkeypatch)
    assert_same_bits(fixed, runtime, SHORT, order)


@pytest.mark.parametrize("order", ORDERS)
def test_first_and_second_interior_step(ssp, signals, num_cu, monkeypatch, order):
    """the lengths at which a lone utterance gets its first and its second interior step, and one frame less"""
    pkg, api = ssp
    o = max(order, 1)
    t1, t2 = first_length_with(1, num_cu, o), first_length_with(2, num_cu, o)
    frames = [t1 - 1, t1, t2 - 1, t2]
    assert [interior_counts([T], num_cu, o)[0] for T in frames] == [0, 1, 1, 2]
    for T in frames:  # (one at a time: in a batch the cuts could differ)
        fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order), [signals(T)], monkeypatch)
        assert_same_bits(fixed, runtime, [T], order)


@pytest.mark.parametrize("order", ORDERS)
def test_bench_utterance(ssp, signals, num_cu, monkeypatch, order):
    pkg, api = ssp
    n_all = sum(len(steps_of(LONG, t0, n, pad, max(order, 1))) for _, t0, n, pad in chunks_of([LONG], num_cu))
    n_in = interior_counts([LONG], num_cu, max(order, 1))[0]
    assert 0 < n_in < n_all, (n_in, n_all)
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order), [signals(LONG)], monkeypatch)
    assert_same_bits(fixed, runtime, [LONG], order)


@pytest.mark.parametrize("order", ORDERS)
def test_cut_utterance(ssp, signals, num_cu, monkeypatch, order):
    """an utterance of more than 512 frames: chunks that start inside it, with halos, and interior steps at ta != 0"""
    pkg, api = ssp
    if order > 0:
        assert any(ta != 0 and inner for _, t0, n, pad in chunks_of([CUT], num_cu) for ta, _, inner in steps_of(CUT, t0, n, pad, order))
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order), [signals(CUT)], monkeypatch)
    assert_same_bits(fixed, runtime, [CUT], order)


@pytest.mark.parametrize("order", ORDERS)
def test_ragged_batch_equals_single_utterances(ssp, signals, num_cu, monkeypatch, order):
    """all of the above in one call: the table path of one utterance does not depend on its neighbours in the batch"""
    pkg, api = ssp
    frames = SHORT + [LONG, CUT]
    # (a batch this small is cut by the same rule as each utterance alone: the bits of an utterance must then be the same)
    assert [c[1:] for c in chunks_of(frames, num_cu) if c[0] == len(frames) - 1] == [c[1:] for c in chunks_of([CUT], num_cu)]
    tables = pkg.preset_sidekit(fs=FS, delta_order=order)
    fixed, runtime = both(api, tables, [signals(T) for T in frames], monkeypatch)
    assert_same_bits(fixed, runtime, frames, order)
    monkeypatch.delenv(SWITCH, raising=False)
    for u, T in enumerate(frames):
        alone = run_stream(api, tables, [signals(T)])[0]
        assert np.array_equal(fixed[u], alone), "utterance %d (%d frames) alone" % (u, T)


@pytest.mark.parametrize("order", ORDERS)
def test_whole_utterance_chunks(ssp, num_cu, monkeypatch, order):
    """a machine-filling batch of 1-s utterances: one chunk per utterance, ta = 0, every wave of a full grid fills and reads its table"""
    pkg, api = ssp
    T = (FS - WIN) // HOP + 1
    n_utt = num_cu * 12 + 128
    frames = [T] * n_utt
    chunks = chunks_of(frames, num_cu)
    assert len(chunks) == n_utt and all(t0 == 0 and n == T for _, t0, n, _ in chunks)
    assert sum(1 for _, _, inner in steps_of(T, 0, T, 0, max(order, 1)) if inner) >= 1
    base = [synth_audio(60 + u, FS, FS) for u in range(7)]
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order), [base[u % 7] for u in range(n_utt)], monkeypatch)
    assert_same_bits(fixed[:64] + fixed[-64:], runtime[:64] + runtime[-64:], [T] * 128, order)
    assert np.array_equal(np.concatenate(fixed), np.concatenate(runtime))
    for u in range(7, n_utt, 997):  # (the same signal gives the same rows wherever it sits)
        assert np.array_equal(fixed[u], fixed[u % 7]), u


@pytest.mark.parametrize("order", ORDERS)
def test_silent_stretch(ssp, num_cu, monkeypatch, order):
    """digital silence inside an utterance (ln 0 = -inf): the scan kernel flags the chunks and the third kernel walks them again, behind
    the first kernel that filled the table; what is finite has the same bits, what is not the same class"""
    pkg, api = ssp
    T = 130
    x = synth_audio(70, n_samples(T), FS).copy()
    x[8000:10400] = 0.0  # frames 50 .. 62 lie wholly inside it
    assert interior_counts([T], num_cu, max(order, 1))[0] >= 1
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order), [x, synth_audio(71, n_samples(T), FS)], monkeypatch)
    assert not np.isfinite(fixed[0]).all() and np.isfinite(fixed[0]).any() and np.isfinite(fixed[1]).all()
    for u in range(2):
        assert fixed[u].shape == (T, 13 * (1 + order))
        assert np.array_equal(np.isnan(fixed[u]), np.isnan(runtime[u])), u
        assert np.array_equal(np.isposinf(fixed[u]), np.isposinf(runtime[u])), u
        assert np.array_equal(np.isneginf(fixed[u]), np.isneginf(runtime[u])), u
        fin = np.isfinite(fixed[u])
        assert np.array_equal(fixed[u][fin], runtime[u][fin]), u


def test_plans_of_different_order_back_to_back(ssp, signals, monkeypatch):
    """two plans on ONE context, launched in turn: every launch fills its own table, nothing of the launch before is read"""
    pkg, api = ssp
    sigs = [signals(LONG), signals(58)]
    monkeypatch.setenv(SWITCH, "1")
    want = {o: run_stream(api, pkg.preset_sidekit(fs=FS, delta_order=o), sigs) for o in ORDERS}
    monkeypatch.delenv(SWITCH, raising=False)
    ctx = api.default_context(torch_stream=False)
    for o in (2, 1, 2, 0, 2):
        got = run_stream(api, pkg.preset_sidekit(fs=FS, delta_order=o), sigs, ctx=ctx)
        assert_same_bits(got, want[o], [LONG, 58], o)
