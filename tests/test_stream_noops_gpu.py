"""What the fixed-geometry instances of the wave-stream MFCC kernel leave out (csrc/mfcc_stream_kernel.hpp, SSP_S_NOFLOOR / SSP_S_PUTSC /
SSP_S_AHEAD): the floor operations in front of the logarithm, the per-lane select of the pipelined loop's ring store, and the chain of
dependent loads at the start of a chunk — replaced by one 32-byte record per chunk that a wave claims and loads one chunk ahead.  None
of it is arithmetic, so the default launch must agree bit for bit with the run-time-geometry instance of the same kernel, which
SSP_MFCC_STREAM_RUNTIME_GEO=1 forces and which keeps the floor, the select and the chain.

Cases: delta orders 0, 1 and 2 unscaled and order 2 scaled (small batches scale with the stand-alone kernel; the 4 000-utterance batch
is machine filling, single chunk per utterance, and reaches the instance that scales in the kernel).  Order 1 unscaled has no
fixed-geometry instance (it does not compile without scratch) and compares the run-time-geometry instance with itself, as in
tests/test_stream_fixed_geometry_gpu.py; which instance a launch took is read off the library's SSP_DEBUG line in a child process."""
import dataclasses
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import synth_audio

pytestmark = pytest.mark.gpu

FS, WIN, HOP = 16000, 400, 160
SWITCH = "SSP_MFCC_STREAM_RUNTIME_GEO"
CASES = [(0, 0), (1, 0), (2, 0), (2, 1)]
FEAT_TOL = 1e-4  # the parity suite's bound against the float64 oracle (tests/test_gpu_parity.py: assert_feat_close)


def n_samples(frames):
    return WIN + HOP * (frames - 1)


@pytest.fixture(scope="module")
def ssp():
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import api
    return pkg, api


def run_stream(api, tables, signals, launches=1):
    ctx = api.default_context(torch_stream=False)
    plan = api.MfccPlan(ctx, tables)
    seg = api.Segments.from_lengths(ctx, [len(s) for s in signals])
    fseg = plan.frame_segments(seg)
    flat = np.concatenate(signals).astype(np.float32)
    outs = []
    for _ in range(launches):
        out = plan.run(flat, seg, fseg, variant=3)
        outs.append([np.array(out[fseg.offsets[i]:fseg.offsets[i + 1]]) for i in range(len(signals))])
    return outs[0] if launches == 1 else outs


def both(api, tables, signals, monkeypatch, launches=1):
    monkeypatch.delenv(SWITCH, raising=False)
    fixed = run_stream(api, tables, signals, launches)
    monkeypatch.setenv(SWITCH, "1")
    runtime = run_stream(api, tables, signals)
    monkeypatch.delenv(SWITCH, raising=False)
    return fixed, runtime


def assert_same_bits(fixed, runtime, frames, order):
    for u, n in enumerate(frames):
        assert fixed[u].shape == (n, 13 * (1 + order)), (u, fixed[u].shape)
        assert np.isfinite(fixed[u]).all(), u
        assert np.array_equal(fixed[u], runtime[u]), "utterance %d (%d frames)" % (u, n)


def assert_feat_close(got, ref, what):
    """tests/test_gpu_parity.py's comparison against the oracle, at its bound"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), what + ": non-finite pattern differs"
    g, r = got[fin], ref[fin]
    if r.size == 0:
        return
    err = np.abs(g - r).max()
    assert err <= FEAT_TOL * max(1.0, np.abs(r).max()), "%s: max abs err %.3e (ref max %.3e)" % (what, err, np.abs(r).max())
    rms = np.sqrt(np.mean(r * r))
    assert np.allclose(g, r, rtol=FEAT_TOL, atol=FEAT_TOL * max(rms, 1e-30)), "%s: max err %.3e rms %.3e" % (what, err, rms)


@pytest.fixture(scope="module")
def ragged():
    """a single partial quad, both sides of a quad and of a step boundary, the two bench lengths, and a 60-s utterance: a batch this
    small is cut into 32-frame chunks, so the long one is some 190 chunks with halos on both sides"""
    frames = [1, 3, 4, 5, 15, 16, 17, 97, 98, 298, (60 * FS - WIN) // HOP + 1]
    return frames, [synth_audio(u, n_samples(n), FS) for u, n in enumerate(frames[:-1])] + [synth_audio(10, 60 * FS, FS)]


@pytest.mark.parametrize("order,cmvn", CASES)
def test_ragged_frame_counts(ssp, ragged, monkeypatch, order, cmvn):
    pkg, api = ssp
    frames, sigs = ragged
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn), sigs, monkeypatch)
    assert_same_bits(fixed, runtime, frames, order)


@pytest.fixture(scope="module")
def grids():
    """one chunk; 41 chunks for a grid of 11 workgroups = 44 waves (at least three waves claim nothing, and every claim ahead of the
    others runs past the table); 4 000 chunks of 8 frames for the 3 072 waves of a full grid"""
    base = [synth_audio(20 + u, n_samples(30), FS) for u in range(5)]
    short = [synth_audio(30 + u, FS // 10, FS) for u in range(7)]
    return {"one": ([20], [synth_audio(19, n_samples(20), FS)]),
            "fewer": ([30] * 41, [base[u % 5] for u in range(41)]),
            "more": ([8] * 4000, [short[u % 7] for u in range(4000)])}


@pytest.mark.parametrize("which", ["one", "fewer", "more"])
@pytest.mark.parametrize("order,cmvn", CASES)
def test_chunk_counts_against_the_grid(ssp, grids, monkeypatch, order, cmvn, which):
    pkg, api = ssp
    frames, sigs = grids[which]
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn), sigs, monkeypatch)
    assert_same_bits(fixed, runtime, frames, order)


@pytest.mark.parametrize("order,cmvn", CASES)
def test_repeated_launch(ssp, grids, monkeypatch, order, cmvn):
    """the claim counter ends a launch past the number of chunks (one claim per wave); the next launch of the same plan starts from zero"""
    pkg, api = ssp
    frames, sigs = grids["fewer"]
    (first, second), runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn), sigs, monkeypatch, launches=2)
    assert_same_bits(first, runtime, frames, order)
    assert_same_bits(second, runtime, frames, order)


@pytest.fixture(scope="module")
def non_finite():
    zero = np.zeros(n_samples(40), dtype=np.float32)  # ln 0 = -inf in every filter of every frame
    nan = synth_audio(41, n_samples(98), FS).copy()
    nan[5000] = np.nan                                # frames 29 .. 31 hold it
    return [zero, nan, synth_audio(42, n_samples(40), FS)]


@pytest.mark.parametrize("order,cmvn", CASES)
def test_non_finite_inputs(ssp, non_finite, monkeypatch, order, cmvn):
    """without the max in front of the log a NaN band energy stays NaN (with it: max -> -inf, log -> NaN), and a zero one is -inf either
    way.  Against the oracle only unscaled: its scaling rejects infinities, as the reference's library does"""
    pkg, api = ssp
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn), non_finite, monkeypatch)
    assert not np.isfinite(fixed[0]).any() and not np.isfinite(fixed[1]).all()
    assert np.isfinite(fixed[2]).all()
    if not cmvn:
        assert np.isfinite(fixed[1]).any()
    for u in range(len(non_finite)):
        assert np.array_equal(np.isnan(fixed[u]), np.isnan(runtime[u])), u
        assert np.array_equal(np.isposinf(fixed[u]), np.isposinf(runtime[u])), u
        assert np.array_equal(np.isneginf(fixed[u]), np.isneginf(runtime[u])), u
        fin = np.isfinite(fixed[u])
        assert np.array_equal(fixed[u][fin], runtime[u][fin]), u
    if not cmvn:
        from oracle import ref_cpu as O
        cfg, w, fb, dct = O.sidekit_tables(fs=FS, delta_order=order)
        for u, x in enumerate(non_finite):
            assert_feat_close(fixed[u], O.mfcc_pipeline(x, cfg, w, fb, dct), "non-finite utt %d order %d" % (u, order))


EPS = 1e-8


def floored(pkg, order):
    tables = pkg.preset_sidekit(fs=FS, delta_order=order)
    return dataclasses.replace(tables, cfg=dataclasses.replace(tables.cfg, floor_mode=1, eps=EPS))


@pytest.mark.parametrize("order", [0, 1, 2])
def test_a_plan_with_a_floor_matches_the_oracle(ssp, order):
    """log(v + eps): the instance without the floor operations must not be taken (test_a_plan_with_a_floor_keeps_the_runtime_instance);
    a silent stretch tells the two apart by far more than the bound: ln eps against -inf"""
    pkg, api = ssp
    from oracle import ref_cpu as O
    silent = synth_audio(52, n_samples(98), FS).copy()
    silent[6000:8000] = 0.0  # frames 38 .. 47 are digitally silent
    sigs = [synth_audio(50, n_samples(98), FS), silent, synth_audio(51, n_samples(17), FS)]
    got = run_stream(api, floored(pkg, order), sigs)
    cfg, w, fb, dct = O.sidekit_tables(fs=FS, delta_order=order)
    cfg = dict(cfg, floor_mode=1, eps=EPS)
    for u, x in enumerate(sigs):
        assert np.isfinite(got[u]).all(), u
        assert_feat_close(got[u], O.mfcc_pipeline(x, cfg, w, fb, dct), "floor utt %d order %d" % (u, order))


CHILD = r"""
import dataclasses, os, sys
import numpy as np
sys.path.insert(0, %r)
from conftest import synth_audio
import speech_signal_processing_amd as pkg
from speech_signal_processing_amd import api
ctx = api.default_context(torch_stream=False)
sigs = [synth_audio(u, 400 + 160 * 97, 16000) for u in range(3)]
for order in (0, 1, 2):
    for floor in (0, 1):
        tables = pkg.preset_sidekit(fs=16000, delta_order=order)
        if floor:
            tables = dataclasses.replace(tables, cfg=dataclasses.replace(tables.cfg, floor_mode=1, eps=1e-8))
        plan = api.MfccPlan(ctx, tables)
        seg = api.Segments.from_lengths(ctx, [len(x) for x in sigs])
        fseg = plan.frame_segments(seg)
        sys.stderr.write("[case] order %%d floor %%d\n" %% (order, floor))
        sys.stderr.flush()
        plan.run(np.concatenate(sigs).astype(np.float32), seg, fseg, variant=3)
"""


@pytest.fixture(scope="module")
def debug_lines():
    """(order, floor) -> the geo figures of the first-kernel launches, from the library's SSP_DEBUG lines in a child process"""
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SSP_DEBUG="1", PYTHONPATH=os.pathsep.join([os.path.dirname(tests_dir), tests_dir]))
    env.pop(SWITCH, None)
    r = subprocess.run([sys.executable, "-c", CHILD % tests_dir], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"\[case\] order (\d) floor (\d)", line)
        if m:
            key = tuple(int(x) for x in m.groups())
            out[key] = []
        m = re.match(r"\[ssp\] mfcc stream: .* geo (\d) cm (\d)", line)
        if m and key is not None:
            out[key].append(int(m.group(1)))
    return out


@pytest.mark.parametrize("order", [0, 1, 2])
def test_a_plan_with_a_floor_keeps_the_runtime_instance(debug_lines, order):
    default_geo = {0: 1, 1: 0, 2: 3}[order]  # (order 1 without scaling: the instance that is not built)
    assert debug_lines[order, 0] and set(debug_lines[order, 0]) == {default_geo}, debug_lines[order, 0]
    assert debug_lines[order, 1] and set(debug_lines[order, 1]) == {0}, debug_lines[order, 1]
