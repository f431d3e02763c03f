"""CPU-side tests of the voice activity detection: the float64 restatement (tests/vad_oracle.py) against the reference's own outputs
(tests/golden/vad.npz, made by tests/golden/make_golden_vad.py), the frame-count rule of the C-ABI, the host-side helpers, and that
nothing computes without a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vad_oracle as VO  # noqa: E402


def _cases(g):
    return [str(c) for c in g["cases"]]


def test_oracle_matches_reference_features(golden):
    """features of the float64 restatement vs the reference's, every frame of every case, <= 1e-11; NaN rows where the reference has them"""
    g = golden("vad")
    for c in _cases(g):
        x = g["x_" + c]
        assert VO.enframe(VO.normalise(x)).shape == tuple(g["shape_" + c]) == (256, VO.num_frames(x.shape[0])), c
        zcr, power, ent = VO.signal_features(x)
        for name, got in (("zcr", zcr), ("power", power), ("entropy", ent)):
            ref = g[name + "_" + c][:, 0]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (c, name)
            np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-11, equal_nan=True, err_msg="%s %s" % (c, name))
        assert np.array_equal(zcr[np.isfinite(zcr)], g["zcr_" + c][:, 0][np.isfinite(zcr)]), c   # counts: exactly
    assert np.isnan(g["power_g"]).all() and np.isnan(g["entropy_g"]).all() and (g["zcr_g"] == 0).all()


def test_oracle_matches_reference_decisions(golden):
    """VAD_detection (both threshold sets) and VAD_frequency on the reference's own features: exactly"""
    g = golden("vad")
    n_speech = 0
    for c in _cases(g):
        for k, (gate, lo, hi) in enumerate(g["thresholds"]):
            got = VO.detect(g["zcr_" + c], g["power_" + c], gate, lo, hi)
            assert np.array_equal(got, g["det%d_%s" % (k, c)][:, 0].astype(np.uint8)), (c, k)
            n_speech += int(got.sum())
        assert np.array_equal(VO.detect_frequency(g["entropy_" + c][:, 0]), g["freq_" + c][:, 0].astype(np.uint8)), c
    assert n_speech > 1000
    # the unreset-run quirk is in the fixture: case c's short burst and the long one behind it are ONE segment
    det = g["det0_c"][:, 0]
    edges = np.flatnonzero(np.diff(np.concatenate(([0], det, [0]))))
    assert len(edges) == 2 and edges[1] - edges[0] > 70, edges


def test_fixture_meets_its_conditions(golden):
    """what make_golden_vad.py asserts, checked again on the stored arrays: no frame inside a threshold's band, quiet last frames, no -32768"""
    g = golden("vad")
    for c in _cases(g):
        assert g["x_" + c].dtype == np.int16 and not (g["x_" + c] == -32768).any()
        zcr, power, ent = g["zcr_" + c][:, 0], g["power_" + c][:, 0], g["entropy_" + c][:, 0]
        for gate, lo, hi in g["thresholds"]:
            p, e = VO.near_threshold(zcr, power, ent, lo, hi)
            assert not p.any() and not e.any(), c
            assert not (power[-1] > lo or zcr[-1] > gate), c


def test_detect_stops_at_frame_zero():
    """the documented deviation: a run that reaches frame 0 starts there, whatever the last frame holds"""
    power = np.array([20.0] * 20 + [0.01] * 5 + [20.0] * 3)
    zcr = np.zeros_like(power)
    assert np.array_equal(VO.detect(zcr, power), np.array([1] * 20 + [0] * 8, dtype=np.uint8))


def test_random_generator_stays_under_the_exclusion_cap():
    """the randomised GPU test drops an utterance from the decision comparison when a frame lies within 1e-4 of a threshold and fails above
    1 % of utterances: the float64 oracle alone must stay well under that"""
    for seed, n_utt, kind in VO.RANDOM_BATCHES:
        sigs, normalize = VO.batch_of(seed, n_utt, kind)
        assert [s.shape[0] for s in sigs[:len(VO.RANDOM_LENGTHS)]] == list(VO.RANDOM_LENGTHS)
        excluded, speech, starts, ends = 0, 0, 0, 0
        for x in sigs:
            zcr, power, ent = VO.signal_features(x, normalize=normalize)
            p, e = VO.near_threshold(zcr, power, ent)
            excluded += bool(p.any() or e.any())
            m = VO.detect(zcr, power)
            speech += int(m.sum())
            if m.size:
                starts += int(m[0])
                ends += int(m[-1])
        assert excluded <= 0.005 * len(sigs), (seed, excluded)   # half the cap of the GPU test
        assert speech > 2000 and starts > 5 and ends > 0, (seed, speech, starts, ends)


def test_vad_num_frames_rule():
    from speech_signal_processing_amd import _lib, api
    got = [api.vad_num_frames(n) for n in (0, 1, 127, 128, 129, 48000, 48077)]
    assert got == [0, 1, 1, 1, 2, 375, 376]
    assert got == [VO.num_frames(n) for n in (0, 1, 127, 128, 129, 48000, 48077)]
    assert api.vad_num_frames(513, 256) == 3
    lib = _lib.load()
    out = ctypes.c_int64()
    assert lib.ssp_vad_num_frames(-1, 128, ctypes.byref(out)) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_num_frames(10, 0, ctypes.byref(out)) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_num_frames(10, 128, None) == _lib.SSP_ERR_INVALID


def test_bad_arguments_are_refused_before_any_gpu_work():
    """null handles answer SSP_ERR_INVALID without a device"""
    from speech_signal_processing_amd import _lib
    lib = _lib.load()
    assert lib.ssp_vad_features(None, None, 0, None, None, 256, 128, 1, 0, None, None, None, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_detect(None, None, None, None, 0, 35.0, 0.3, 12.0, 16, None, None, 0, None) == _lib.SSP_ERR_INVALID
    assert lib.ssp_vad_frame_segments(None, None, 128, None) == _lib.SSP_ERR_INVALID


def test_enframe_and_segments_on_the_host(golden):
    """VAD.enframe is the reference's matrix; speech_segments keeps exactly the samples a marked frame covers"""
    from speech_signal_processing_amd import VAD
    g = golden("vad")
    for c in _cases(g):
        x = g["x_" + c]
        fr = VAD.enframe(VO.normalise(x))
        assert fr.shape == tuple(g["shape_" + c]) and fr.dtype == np.float64
        assert np.array_equal(fr, VO.enframe(VO.normalise(x)), equal_nan=True)
        for key in ("det0_", "det1_", "freq_"):
            mask = g[key + c][:, 0]
            segs, keep = VO.speech_segments(mask, x.shape[0])
            assert VAD.speech_segments(mask, x.shape[0]) == segs, (c, key)
            assert sum(b - a for a, b in segs) == int(keep.sum())
    assert VAD.speech_segments(np.array([0, 1, 0, 1, 1, 0, 0, 1]), 1000) == [(128, 384 + 384), (896, 1000)]
    assert VAD.speech_segments(np.zeros(5), 600) == []


def test_wavdata_reads_normalises_and_frames(tmp_path, golden):
    """VAD.wavdata: the file's int16 samples over their peak, framed (host only)"""
    import wave
    from speech_signal_processing_amd import VAD
    x = golden("vad")["x_b"]
    path = str(tmp_path / "b.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(x.astype("<i2").tobytes())
    fr = VAD.wavdata(path)
    assert fr.shape == tuple(golden("vad")["shape_b"]) and np.array_equal(fr, VO.enframe(VO.normalise(x)))


def test_vad_module_fails_loudly_without_gpu():
    """No CPU fallback: without a device every computing call of the VAD module raises SspError"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speech_signal_processing_amd import VAD, _lib
    frames = np.zeros((256, 4))
    for call in (lambda: VAD.feature(frames), lambda: VAD.ZCR(frames), lambda: VAD.energy(frames), lambda: VAD.spectrum_entropy(frames),
                 lambda: VAD.VAD_detection(np.zeros((4, 1)), np.zeros((4, 1))), lambda: VAD.VAD_frequency(np.zeros((4, 1))),
                 lambda: VAD.feature_batch([np.zeros(1000, dtype=np.int16)]), lambda: VAD.detect_batch([np.zeros(1000, dtype=np.int16)]),
                 lambda: VAD.remove_silence([np.zeros(1000, dtype=np.int16)])):
        with pytest.raises(_lib.SspError):
            call()


def test_product_never_imports_the_test_oracle():
    pkg = os.path.join(ROOT, "speech_signal_processing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(tests|oracle|vad_oracle)\b", text, flags=re.M), os.path.join(dirpath, f)
                assert "vad_oracle" not in text, os.path.join(dirpath, f)
