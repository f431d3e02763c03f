"""The wave-stream MFCC kernel's fixed-geometry instances (window 400, hop 160, 24 filters, 13 cepstra: hop, stage layout, delta order
and row width are template constants) against the run-time-geometry instances of the same kernel, which SSP_MFCC_STREAM_RUNTIME_GEO=1
forces: the two run the same operations in the same order, so every utterance must come out bit for bit the same.

Which instance a launch takes is read off the library's SSP_DEBUG line in a child process (test_default_launch_takes_the_fixed_instance):
GEO = 1 + delta order, except delta order 1 without scaling, whose fixed-geometry instance does not compile without scratch and is
therefore not built — those plans keep the run-time-geometry instance, and their cases here compare it with itself.
The small batches below are always scaled by the stand-alone kernel (the plan scales in the stream kernel only when every utterance is
one chunk of a machine-filling batch), so their cmvn = 1 cases run the CM = 0 instances; the CM = 1 fixed-geometry instances are
reached by test_scaling_instances_in_a_machine_filling_batch."""
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
CASES = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]


def n_samples(frames):
    return WIN + HOP * (frames - 1)


@pytest.fixture(scope="module")
def ssp():
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import api
    return pkg, api


@pytest.fixture(scope="module")
def ragged():
    """one partial quad, both sides of a step boundary (12 / 28 mod 16), the two bench lengths and one utterance longer than a
    512-frame chunk (a second chunk with a halo; a batch this small is also cut into short chunks)"""
    frames = [1, 3, 4, 5, 11, 12, 13, 27, 28, 29, 98, 298, 530]
    return frames, [synth_audio(u, n_samples(n), FS) for u, n in enumerate(frames)]


@pytest.fixture(scope="module")
def out_of_range():
    return [synth_audio(50, 399, FS), synth_audio(51, 401, FS), synth_audio(52, n_samples(20), FS)]


@pytest.fixture(scope="module")
def silent():
    x = synth_audio(60, n_samples(98), FS).copy()
    x[6000:8000] = 0.0  # frames 38 .. 47 are digitally silent: ln 0 = -inf, the scan kernel flags the chunk, the walk kernel redoes it
    return [x, synth_audio(61, n_samples(40), FS)]


def run_stream(api, tables, signals):
    ctx = api.default_context(torch_stream=False)
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


@pytest.mark.parametrize("order,cmvn", CASES)
def test_ragged_lengths_and_a_multi_chunk_utterance(ssp, ragged, monkeypatch, order, cmvn):
    pkg, api = ssp
    frames, sigs = ragged
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn), sigs, monkeypatch)
    for u, n in enumerate(frames):
        assert fixed[u].shape == (n, 13 * (1 + order)), (u, fixed[u].shape)
        assert np.isfinite(fixed[u]).all(), u
        assert np.array_equal(fixed[u], runtime[u]), "utterance %d (%d frames)" % (u, n)


@pytest.mark.parametrize("order,cmvn", CASES)
def test_out_of_range_lengths(ssp, out_of_range, monkeypatch, order, cmvn):
    pkg, api = ssp
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn), out_of_range, monkeypatch)
    assert [len(f) for f in fixed] == [0, 1, 20]
    for u in range(len(out_of_range)):
        assert fixed[u].shape == runtime[u].shape
        assert np.array_equal(fixed[u], runtime[u]), u


@pytest.mark.parametrize("order,cmvn", CASES)
def test_misaligned_base(ssp, ragged, monkeypatch, order, cmvn):
    """the batch 1, 2 and 3 floats off the 16-byte grid (device pointers): the sample DMA needs dword-aligned addresses only"""
    import torch
    pkg, api = ssp
    sigs = ragged[1][6:]
    tables = pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn)
    flat = np.concatenate(sigs).astype(np.float32)
    res = {}
    for geo in (None, "1"):
        if geo is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, geo)
        ctx = api.default_context(torch_stream=True)
        plan = api.MfccPlan(ctx, tables)
        seg = api.Segments.from_lengths(ctx, [len(s) for s in sigs])
        fseg = plan.frame_segments(seg)
        for mis in (1, 2, 3):
            buf = torch.zeros(len(flat) + 8, device="cuda")
            buf[mis:mis + len(flat)] = torch.from_numpy(flat).cuda()
            res[geo, mis] = plan.run(buf[mis:mis + len(flat)], seg, fseg, variant=3).cpu().numpy()
    monkeypatch.delenv(SWITCH, raising=False)
    for mis in (1, 2, 3):
        assert res[None, mis].shape == (sum(ragged[0][6:]), 13 * (1 + order))
        assert np.array_equal(res[None, mis], res["1", mis]), mis
        assert np.array_equal(res[None, mis], res[None, 1]), mis


@pytest.mark.parametrize("order,cmvn", CASES)
def test_non_finite_path(ssp, silent, monkeypatch, order, cmvn):
    pkg, api = ssp
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=cmvn), silent, monkeypatch)
    assert not np.isfinite(fixed[0]).all()  # the silent stretch shows
    if not cmvn:  # (scaled, a column that holds -inf has no finite mean)
        assert np.isfinite(fixed[0]).any()
    assert np.isfinite(fixed[1]).all()
    for u in range(len(silent)):
        assert np.array_equal(np.isnan(fixed[u]), np.isnan(runtime[u])), u
        assert np.array_equal(np.isposinf(fixed[u]), np.isposinf(runtime[u])), u
        assert np.array_equal(np.isneginf(fixed[u]), np.isneginf(runtime[u])), u
        fin = np.isfinite(fixed[u])
        assert np.array_equal(fixed[u][fin], runtime[u][fin]), u


@pytest.fixture(scope="module")
def filling():
    """3400 one-second utterances, each a single 98-frame chunk: more chunks than the machine has waves to fill, so the plan lets the
    stream kernel scale the features itself (CM = 1)"""
    base = [synth_audio(100 + u, n_samples(98), FS) for u in range(7)]
    return [base[u % 7] for u in range(3400)]


@pytest.mark.parametrize("order", [0, 1, 2])
def test_scaling_instances_in_a_machine_filling_batch(ssp, filling, monkeypatch, order):
    pkg, api = ssp
    fixed, runtime = both(api, pkg.preset_sidekit(fs=FS, delta_order=order, cmvn=1), filling, monkeypatch)
    for u in list(range(0, 3400, 113)) + [3399]:
        assert fixed[u].shape == (98, 13 * (1 + order))
        assert np.isfinite(fixed[u]).all(), u
        assert np.abs(fixed[u].mean(axis=0)).max() < 1e-3, u  # scaled
        assert np.array_equal(fixed[u], runtime[u]), u


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r)
from conftest import synth_audio
import speech_signal_processing_amd as pkg
from speech_signal_processing_amd import api
ctx = api.default_context(torch_stream=False)
small = [synth_audio(u, 400 + 160 * 97, 16000) for u in range(3)]
big = [small[u %% 3] for u in range(3400)]
for order, cmvn, sigs in [(0, 0, small), (1, 0, small), (2, 0, small), (0, 1, big), (1, 1, big), (2, 1, big)]:
    for switch in (0, 1):
        if switch:
            os.environ["SSP_MFCC_STREAM_RUNTIME_GEO"] = "1"
        else:
            os.environ.pop("SSP_MFCC_STREAM_RUNTIME_GEO", None)
        plan = api.MfccPlan(ctx, pkg.preset_sidekit(fs=16000, delta_order=order, cmvn=cmvn))
        seg = api.Segments.from_lengths(ctx, [len(x) for x in sigs])
        fseg = plan.frame_segments(seg)
        sys.stderr.write("[case] order %%d cmvn %%d switch %%d\n" %% (order, cmvn, switch))
        sys.stderr.flush()
        plan.run(np.concatenate(sigs).astype(np.float32), seg, fseg, variant=3)
"""


@pytest.fixture(scope="module")
def debug_lines():
    """(order, cmvn, switch) -> the (geo, cm) pairs of the first-kernel launches, from the library's SSP_DEBUG lines in a child process"""
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SSP_DEBUG="1", PYTHONPATH=os.pathsep.join([os.path.dirname(tests_dir), tests_dir]))
    env.pop(SWITCH, None)
    r = subprocess.run([sys.executable, "-c", CHILD % tests_dir], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"\[case\] order (\d) cmvn (\d) switch (\d)", line)
        if m:
            key = tuple(int(x) for x in m.groups())
            out[key] = []
        m = re.match(r"\[ssp\] mfcc stream: .* geo (\d) cm (\d)", line)
        if m and key is not None:
            out[key].append((int(m.group(1)), int(m.group(2))))
    return out


@pytest.mark.parametrize("order", [0, 1, 2])
def test_default_launch_takes_the_fixed_instance(debug_lines, order):
    """without this, a dispatch that fell back to GEO = 0 would let every comparison above pass on one and the same kernel"""
    small_geo = {0: 1, 1: 0, 2: 3}[order]  # (order 1 without scaling: the instance that is not built)
    assert debug_lines[order, 0, 0] and set(debug_lines[order, 0, 0]) == {(small_geo, 0)}, debug_lines[order, 0, 0]
    assert debug_lines[order, 1, 0] and set(debug_lines[order, 1, 0]) == {(1 + order, 1)}, debug_lines[order, 1, 0]
    for cmvn in (0, 1):
        assert debug_lines[order, cmvn, 1] and set(debug_lines[order, cmvn, 1]) == {(0, cmvn)}, debug_lines[order, cmvn, 1]
