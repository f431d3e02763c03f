"""GPU tests of the voice activity detection (run with -m gpu on an MI355X): the feature and detector kernels, through the
reference-shaped VAD module and the batched surface, against the reference's own outputs (tests/golden/vad.npz) and, on randomised
ragged batches, against the float64 restatement tests/vad_oracle.py.

Tolerances are the project's own (tests/test_gpu_parity.py:4-7, north star 1e-4):
  power   : |gpu - ref| <= 1e-4 |ref| per frame
  entropy : |gpu - ref| <= 1e-4 max(1, max|ref|) per utterance
  gated zcr, NaN pattern, every decision : equal
Every fixture frame is compared (the fixture keeps its frames outside the 1e-4 band of every threshold).  In the randomised batches an
utterance with a frame inside that band is compared on features only, and at most 1 % of utterances may be such.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vad_oracle as VO  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def vad():
    from speech_signal_processing_amd import VAD, api
    return VAD, api


def _cases(g):
    return [str(c) for c in g["cases"]]


def check_features(got, ref, what, band_free=True):
    """got / ref: (zcr, power, entropy); returns the largest errors seen (power relative, entropy absolute)"""
    gz, gp, ge = (np.asarray(v, dtype=np.float64).reshape(-1) for v in got)
    rz, rp, re_ = (np.asarray(v, dtype=np.float64).reshape(-1) for v in ref)
    assert gz.shape == rz.shape and gp.shape == rp.shape and ge.shape == re_.shape, (what, gp.shape, rp.shape)
    if rp.size == 0:
        return 0.0, 0.0
    assert np.array_equal(np.isnan(gp), np.isnan(rp)) and np.array_equal(np.isnan(ge), np.isnan(re_)), what + ": NaN pattern differs"
    assert not np.isnan(gz).any(), what
    fin = ~np.isnan(rp)
    perr = np.abs(gp[fin] - rp[fin])
    rel = float((perr / np.maximum(np.abs(rp[fin]), 1e-300)).max()) if fin.any() else 0.0
    assert (perr <= TOL * np.abs(rp[fin])).all(), "%s: power off by %.3e relative" % (what, rel)
    eerr = float(np.abs(ge[fin] - re_[fin]).max()) if fin.any() else 0.0
    assert eerr <= TOL * max(1.0, float(np.abs(re_[fin]).max()) if fin.any() else 1.0), "%s: entropy off by %.3e" % (what, eerr)
    if band_free:
        assert np.array_equal(gz, rz), "%s: gated zcr differs on %d frames" % (what, int((gz != rz).sum()))
    return rel, eerr


def test_reference_shaped_features_vs_reference(vad, golden):
    """enframe -> feature / ZCR / energy / spectrum_entropy as the reference is called, every frame of every case"""
    VAD, _ = vad
    g = golden("vad")
    worst = [0.0, 0.0]
    for c in _cases(g):
        frames = VAD.enframe(VO.normalise(g["x_" + c]))
        assert frames.shape == tuple(g["shape_" + c])
        zcr, power, ent = VAD.feature(frames)
        for v in (zcr, power, ent):
            assert v.shape == (frames.shape[1], 1) and v.dtype == np.float64
        rel, eerr = check_features((zcr, power, ent), (g["zcr_" + c], g["power_" + c], g["entropy_" + c]), "feature " + c)
        worst = [max(worst[0], rel), max(worst[1], eerr)]
        assert np.array_equal(VAD.energy(frames), power, equal_nan=True) and np.array_equal(VAD.spectrum_entropy(frames), ent, equal_nan=True)
        with np.errstate(invalid="ignore"):
            sg = np.sign(frames)
            raw = ((sg[:-1] * sg[1:]) < 0).sum(axis=0).astype(np.float64).reshape(-1, 1)
        assert np.array_equal(VAD.ZCR(frames), raw), c   # the bare count, not gated
    print("[observed] reference-shaped: power %.3e relative, entropy %.3e absolute" % tuple(worst))


def test_feature_batch_vs_reference(vad, golden):
    """the whole fixture as ONE ragged int16 batch (peak on the device), and as float32 of the same integers"""
    VAD, _ = vad
    g = golden("vad")
    names = _cases(g)
    for cast in (lambda x: x, lambda x: x.astype(np.float32)):
        out = VAD.feature_batch([cast(g["x_" + c]) for c in names])
        assert len(out) == len(names)
        worst = [0.0, 0.0]
        for c, got in zip(names, out):
            rel, eerr = check_features(got, (g["zcr_" + c], g["power_" + c], g["entropy_" + c]), "feature_batch " + c)
            worst = [max(worst[0], rel), max(worst[1], eerr)]
        print("[observed] feature_batch: power %.3e relative, entropy %.3e absolute" % tuple(worst))


def test_decisions_vs_reference(vad, golden):
    """VAD_detection on the fixture's own float64 features (both threshold sets), VAD_frequency, and both end to end from the int16 input"""
    VAD, _ = vad
    g = golden("vad")
    names = _cases(g)
    for c in names:
        for k, (gate, lo, hi) in enumerate(g["thresholds"]):
            res = VAD.VAD_detection(g["zcr_" + c], g["power_" + c], zcr_gate=gate, ampl=lo, amph=hi)
            assert res.shape == g["det%d_%s" % (k, c)].shape and res.dtype == np.float64
            assert np.array_equal(res, g["det%d_%s" % (k, c)]), (c, k)
        fr = VAD.VAD_frequency(g["entropy_" + c])
        assert fr.shape == g["freq_" + c].shape and np.array_equal(fr, g["freq_" + c]), c
    sigs = [g["x_" + c] for c in names]
    for k, (gate, lo, hi) in enumerate(g["thresholds"]):
        masks = VAD.detect_batch(sigs, zcr_gate=gate, ampl=lo, amph=hi)
        for c, m in zip(names, masks):
            assert m.dtype == np.uint8 and np.array_equal(m, g["det%d_%s" % (k, c)][:, 0].astype(np.uint8)), (c, k)
    for c, m in zip(names, VAD.detect_batch(sigs, method='frequency')):
        assert np.array_equal(m, g["freq_" + c][:, 0].astype(np.uint8)), c


def _bits(v):
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def test_same_bits_whatever_the_route(vad, golden):
    """int16 and float32 of the same integers; host and device pointers; an utterance in a batch and alone: the same float32 bits"""
    import torch
    _, api = vad
    g = golden("vad")
    ctx = api.default_context()
    sigs = [g["x_" + c] for c in _cases(g)] + VO.random_batch(3, 14)
    flat = np.concatenate(sigs)
    seg = api.Segments.from_lengths(ctx, [s.shape[0] for s in sigs])
    base = api.vad_features(ctx, flat, seg)
    fseg = base[3]
    assert [int(n) for n in np.diff(fseg.offsets)] == [VO.num_frames(s.shape[0]) for s in sigs]
    routes = {"float32 host": api.vad_features(ctx, flat.astype(np.float32), seg),
              "int16 device": api.vad_features(ctx, torch.from_numpy(flat).cuda(), seg),
              "float32 device": api.vad_features(ctx, torch.from_numpy(flat.astype(np.float32)).cuda(), seg)}
    for name, got in routes.items():
        for k in range(3):
            assert np.array_equal(_bits(got[k]), _bits(base[k])), (name, k)
    # step 256 (the framed-matrix calls' layout): int16 and float32 of the same integers, against the restatement's frames taken every 256
    s256 = (api.vad_features(ctx, flat, seg, step=256), api.vad_features(ctx, flat.astype(np.float32), seg, step=256))
    for k in range(3):
        assert np.array_equal(_bits(s256[0][k]), _bits(s256[1][k])), ("step 256", k)
    o256 = s256[0][3].offsets
    for u in (0, 1, 4, len(sigs) - 1):
        ref = VO.features(VO.enframe(VO.normalise(sigs[u]), step=256))
        check_features(tuple(v[o256[u]:o256[u + 1]] for v in s256[0][:3]), ref, "step 256, utterance %d" % u, band_free=False)
    o = fseg.offsets
    for u, s in enumerate(sigs):
        alone = api.vad_features(ctx, s, api.Segments.from_lengths(ctx, [s.shape[0]]))
        for k in range(3):
            assert np.array_equal(_bits(alone[k]), _bits(base[k])[o[u]:o[u + 1]]), (u, k)
    # the detector: host and device pointers, batch and alone
    mask, count = api.vad_detect(ctx, base[0], base[1], fseg)
    dmask, dcount = api.vad_detect(ctx, torch.from_numpy(base[0]).cuda(), torch.from_numpy(base[1]).cuda(), fseg)
    assert np.array_equal(mask, dmask.cpu().numpy()) and np.array_equal(count, dcount.cpu().numpy())
    assert count.dtype == np.int32 and [int(mask[o[u]:o[u + 1]].sum()) for u in range(len(sigs))] == count.tolist()
    for u in range(len(sigs)):
        m1, c1 = api.vad_detect(ctx, base[0][o[u]:o[u + 1]], base[1][o[u]:o[u + 1]], api.Segments.from_lengths(ctx, [int(o[u + 1] - o[u])]))
        assert np.array_equal(m1, mask[o[u]:o[u + 1]]) and int(c1[0]) == int(count[u]), u


def test_long_chunks_vs_reference_and_alone(vad, golden):
    """One call large enough that the library cuts LONG chunks — its chunk length is total frames / (12 x CUs) rounded up to 8 (8 below
    24 576 frames on 256 CUs, >= 24 here, several chunks per utterance) — so the eight-frame loop runs more than once per chunk: the next
    stage's DMA under the arithmetic, the int16 tail fix behind the first stage, multi-chunk utterances.  The fixture plus 200 utterances
    of 2 to 3 s, int16, most of odd length (every other utterance then STARTS on an odd sample), starting / ending in speech.  Features
    against vad.npz and the float64 restatement at the usual bounds; the same bits as float32 and as every utterance alone (cut in
    eights); decisions on every utterance without a frame inside a threshold's band."""
    VAD, api = vad
    g = golden("vad")
    names = _cases(g)
    rng = np.random.default_rng(21)
    sigs = [g["x_" + c] for c in names]
    for u in range(200):
        n = 2 * int(rng.integers(16000, 24000)) + (0 if u % 4 == 3 else 1)
        sigs.append(VO.random_signal(rng, n, start_in_speech=(u % 3 == 0), end_in_speech=(u % 3 == 1)))
    ctx = api.default_context()
    flat = np.concatenate(sigs)
    seg = api.Segments.from_lengths(ctx, [x.shape[0] for x in sigs])
    assert sum(int(seg.offsets[u]) & 1 for u in range(len(sigs))) > 50
    zcr, power, ent, fseg = api.vad_features(ctx, flat, seg)
    assert fseg.total > 2 * 24576 and max(np.diff(fseg.offsets)) > 64
    f32 = api.vad_features(ctx, flat.astype(np.float32), seg)
    for k, v in enumerate((zcr, power, ent)):
        assert np.array_equal(_bits(f32[k]), _bits(v)), k
    mask, _ = api.vad_detect(ctx, zcr, power, fseg)
    o = fseg.offsets
    worst, clean_n = [0.0, 0.0], 0
    for u, x in enumerate(sigs):
        got = tuple(v[o[u]:o[u + 1]] for v in (zcr, power, ent))
        if u < len(names):
            c = names[u]
            ref, clean = (g["zcr_" + c], g["power_" + c], g["entropy_" + c]), True
            ref_mask = g["det0_" + c][:, 0].astype(np.uint8)
        else:
            ref = VO.signal_features(x)
            p_band, e_band = VO.near_threshold(*ref)
            clean = not (p_band.any() or e_band.any())
            ref_mask = VO.detect(ref[0], ref[1])
        rel, eerr = check_features(got, ref, "long chunks, utterance %d (%d samples)" % (u, x.shape[0]), band_free=clean)
        worst = [max(worst[0], rel), max(worst[1], eerr)]
        if clean:
            clean_n += 1
            assert np.array_equal(mask[o[u]:o[u + 1]], ref_mask), u
        alone = api.vad_features(ctx, x, api.Segments.from_lengths(ctx, [x.shape[0]]))
        for k in range(3):
            assert np.array_equal(_bits(alone[k]), _bits(got[k])), (u, k)
    print("[observed] long chunks: power %.3e relative, entropy %.3e absolute, %d of %d utterances compared on decisions" % (
        worst[0], worst[1], clean_n, len(sigs)))
    assert clean_n >= 0.9 * len(sigs)


def test_longest_chunks_on_the_device(vad):
    """A batch that reaches the chunk cap (1024 frames: 3.4 M frames on 256 CUs, every utterance ONE chunk of 375 frames, 47 trips of the
    eight-frame loop) — the cut the throughput figures are measured with.  9 000 int16 utterances of 47 999 samples on the device (odd
    length: every other one starts on an odd sample), copies of 16 signals: every copy must carry the bits its signal gets alone, and
    those agree with the float64 restatement.  The same batch as float32."""
    import torch
    _, api = vad
    ctx = api.default_context()
    rng = np.random.default_rng(22)
    K, n, n_utt = 16, 47999, 9000
    base = [VO.random_signal(rng, n, start_in_speech=(k % 3 == 0), end_in_speech=(k % 3 == 1)) for k in range(K)]
    T = VO.num_frames(n)
    alone = []
    for k, x in enumerate(base):
        a = api.vad_features(ctx, x, api.Segments.from_lengths(ctx, [n]))
        ref = VO.signal_features(x)
        p_band, e_band = VO.near_threshold(*ref)
        check_features(a[:3], ref, "signal %d alone" % k, band_free=not (p_band.any() or e_band.any()))
        alone.append(np.stack([_bits(a[j]) for j in range(3)]))
    alone = torch.from_numpy(np.stack(alone).astype(np.int64)).cuda()          # (K, 3, T) bit patterns
    idx = torch.from_numpy(rng.integers(0, K, n_utt)).cuda()
    flat = torch.from_numpy(np.stack(base)).cuda()[idx].reshape(-1)
    seg = api.Segments.from_lengths(ctx, np.full(n_utt, n, dtype=np.int64))
    assert n_utt * T > 1024 * 12 * 256
    for x in (flat, flat.float()):
        out = api.vad_features(ctx, x, seg)
        torch.cuda.synchronize()
        for j in range(3):
            got = out[j].view(torch.int32).to(torch.int64).bitwise_and(0xFFFFFFFF).view(n_utt, T)
            bad = (got != alone[idx, j]).any(dim=1)
            assert not bool(bad.any()), "plane %d: %d of %d utterances differ from their signal alone" % (j, int(bad.sum()), n_utt)
        del out


@pytest.mark.parametrize("seed,n_utt,kind", VO.RANDOM_BATCHES)
def test_random_batches_vs_oracle(vad, seed, n_utt, kind):
    """ragged batches (lengths 0, 1, 127, 128, 129, ... and random ones; utterances that start or end in speech) against the float64
    restatement: features on every utterance; zcr and masks on every utterance without a frame inside the 1e-4 band of a threshold"""
    VAD, _ = vad
    sigs, normalize = VO.batch_of(seed, n_utt, kind)
    feats = VAD.feature_batch(sigs, normalize=normalize)
    masks = VAD.detect_batch(sigs, normalize=normalize)
    fmasks = VAD.detect_batch(sigs, method='frequency', normalize=normalize)
    excluded, worst, speech = 0, [0.0, 0.0], 0
    for u, x in enumerate(sigs):
        zcr, power, ent = VO.signal_features(x, normalize=normalize)
        p_band, e_band = VO.near_threshold(zcr, power, ent)
        clean = not (p_band.any() or e_band.any())
        excluded += not clean
        rel, eerr = check_features(feats[u], (zcr, power, ent), "%s utterance %d (%d samples)" % (kind, u, x.shape[0]), band_free=clean)
        worst = [max(worst[0], rel), max(worst[1], eerr)]
        assert masks[u].shape == (VO.num_frames(x.shape[0]),) == fmasks[u].shape
        if clean:
            ref = VO.detect(zcr, power)
            assert np.array_equal(masks[u], ref), "%s utterance %d: mask differs on %d frames" % (kind, u, int((masks[u] != ref).sum()))
            assert np.array_equal(fmasks[u], VO.detect_frequency(ent)), (kind, u)
            speech += int(ref.sum())
    print("[observed] %s: power %.3e relative, entropy %.3e absolute, %d of %d utterances excluded, %d speech frames" % (
        kind, worst[0], worst[1], excluded, len(sigs), speech))
    assert excluded <= 0.01 * len(sigs), excluded
    assert speech > 2000


def test_detector_edges(vad):
    """the stop at frame 0 (loud last frame, run reaching frame 0) against a hand-written expectation; runs that stay open; an utterance
    long enough for the detector's out-of-LDS word planes"""
    VAD, api = vad
    power = np.array([20.0] * 20 + [0.01] * 5 + [20.0] * 3)
    want = np.array([1.0] * 20 + [0.0] * 8).reshape(-1, 1)
    assert np.array_equal(VAD.VAD_detection(np.zeros_like(power), power), want)
    # a short run is not reset: frames 3..8 (6 loud) + gap + 12 loud -> one segment from 3 on, closed by the quiet frame behind it
    power = np.array([0.01] * 3 + [20.0] * 6 + [0.01] * 10 + [20.0] * 12 + [0.01] * 4)
    want = np.array([0.0] * 3 + [1.0] * 28 + [0.0] * 4).reshape(-1, 1)
    assert np.array_equal(VAD.VAD_detection(np.zeros_like(power), power), want)
    # active (not loud) frames around a run are taken in, through power or through zcr; a run open at the end is never flushed
    power = np.array([0.01, 0.5, 0.5] + [20.0] * 17 + [0.2, 0.2, 0.01] + [20.0] * 30)
    zcr = np.array([0.0] * 20 + [40.0, 10.0, 0.0] + [0.0] * 30)
    want = np.array([0.0] + [1.0] * 20 + [0.0] * 32).reshape(-1, 1)
    assert np.array_equal(VAD.VAD_detection(zcr, power), want)
    assert np.array_equal(VAD.VAD_detection(zcr, power), VO.detect(zcr, power).reshape(-1, 1).astype(np.float64))
    assert VAD.VAD_detection(np.zeros((0, 1)), np.zeros((0, 1))).shape == (0, 1)
    # 40 000 frames: random runs, compared with the restatement
    rng = np.random.default_rng(5)
    n = 40000
    power = np.full(n, 0.01)
    at = 0
    while at < n - 200:
        at += int(rng.integers(1, 120))
        m = int(rng.integers(1, 60))
        power[at:at + m] = 20.0
        power[at + m:at + m + int(rng.integers(0, 6))] = 0.5
        at += m
    zcr = np.where(rng.random(n) < 0.05, 40.0, 0.0)
    got = VAD.VAD_detection(zcr, power)[:, 0]
    ref = VO.detect(zcr, power)
    assert np.array_equal(got, ref) and 1000 < ref.sum() < n
    ctx = api.default_context()
    mask, count = api.vad_detect(ctx, np.concatenate([zcr, zcr[:500]]).astype(np.float32), np.concatenate([power, power[:500]]).astype(np.float32),
                                 api.Segments.from_lengths(ctx, [n, 0, 500]))
    assert np.array_equal(mask[:n], ref) and np.array_equal(mask[n:], VO.detect(zcr[:500], power[:500]))
    assert count.tolist() == [int(ref.sum()), 0, int(mask[n:].sum())]


def test_segments_and_remove_silence(vad, golden):
    """remove_silence keeps exactly the samples that a frame of the (reference's) mask covers"""
    VAD, _ = vad
    g = golden("vad")
    names = _cases(g)
    sigs = [g["x_" + c] for c in names]
    for k, (gate, lo, hi) in enumerate(g["thresholds"]):
        out = VAD.remove_silence(sigs, zcr_gate=gate, ampl=lo, amph=hi)
        for c, x, y in zip(names, sigs, out):
            _, keep = VO.speech_segments(g["det%d_%s" % (k, c)][:, 0], x.shape[0])
            assert y.dtype == x.dtype and np.array_equal(y, x[keep]), (c, k)
    assert sum(y.shape[0] for y in out) > 50000 and out[names.index("g")].shape == (0,)


def test_error_codes(vad):
    _, api = vad
    from speech_signal_processing_amd import _lib
    ctx = api.default_context()
    x = np.zeros(1000, dtype=np.float32)
    seg = api.Segments.from_lengths(ctx, [1000])
    with pytest.raises(NotImplementedError):
        api.vad_features(ctx, x, seg, step=100)
    with pytest.raises(NotImplementedError):
        api.vad_features(ctx, x, seg, frame_size=512, step=256)
    with pytest.raises(ValueError):
        api.vad_features(ctx, x, seg, frame_seg=api.vad_frame_segments(ctx, seg, 256), step=128)   # 4 frames in the table, 8 expected
    with pytest.raises(ValueError):
        api.vad_features(ctx, x, seg, frame_seg=api.Segments.from_lengths(ctx, [4, 4]))            # another count of utterances
    with pytest.raises(ValueError):
        api.vad_detect(ctx, x[:8], x[:8], api.Segments.from_lengths(ctx, [8]), mode=2)
    with pytest.raises(ValueError):
        api.vad_detect(ctx, x[:8], x[:8], api.Segments.from_lengths(ctx, [8]), min_len=0)
    lib = _lib.load()
    fseg = api.vad_frame_segments(ctx, seg)
    buf = np.zeros(8, dtype=np.float32)
    p = buf.ctypes.data
    assert lib.ssp_vad_features(ctx._h, None, 0, seg._h, fseg._h, 256, 128, 1, 0, p, p, p, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_features(ctx._h, x.ctypes.data, 0, seg._h, fseg._h, 256, 128, 1, 0, p, None, p, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_features(ctx._h, x.ctypes.data, 2, seg._h, fseg._h, 256, 128, 1, 0, p, p, p, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_features(ctx._h, x.ctypes.data, 0, seg._h, fseg._h, 256, 128, 1, 0, p, p, p, 7, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_features(ctx._h, x.ctypes.data, 0, seg._h, fseg._h, 256, 0, 1, 0, p, p, p, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_features(ctx._h, x.ctypes.data, 0, seg._h, fseg._h, 256, 128, 1, 6, p, p, p, 0, None) == _lib.SSP_ERR_INVALID   # unknown flag bits
    assert lib.ssp_vad_features(ctx._h, x.ctypes.data, 0, seg._h, fseg._h, 256, 64, 1, 0, p, p, p, 0, None) == _lib.SSP_ERR_UNSUPPORTED
    assert lib.ssp_vad_detect(ctx._h, None, p, fseg._h, 0, 35.0, 0.3, 12.0, 16, p, None, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_detect(ctx._h, p, p, fseg._h, 0, 35.0, 0.3, 12.0, 16, None, None, 0, None) == _lib.SSP_ERR_INVALID
    assert b"null" in lib.ssp_last_error()
    assert ctypes.c_int(lib.ssp_vad_detect(ctx._h, p, p, fseg._h, 0, 35.0, 0.3, 12.0, 16, p, None, 0, None)).value == _lib.SSP_OK   # counts are optional
