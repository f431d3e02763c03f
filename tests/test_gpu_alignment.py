"""GPU tests of every device-pointer entry point on arrays that are NOT 16-byte aligned (run with -m gpu on an MI355X).

include/ssp.h asks of a device array only the natural alignment of its element type; many kernels pick a 16-byte or a scalar code path
from the low four address bits ("Alignment of device arrays").  torch's allocator hands out 512-byte aligned blocks, so the
other tests never reach the second branch.  Here every array is a view at a chosen skew inside a guarded buffer (tests/skewed.py):

  1. the result is BIT-EQUAL (np.array_equal, NaN pattern included) to the same call on 16-byte aligned copies of the same arrays:
     every pair of branches differs only in how bytes are moved, never in the order of a sum;
  2. for one skew per case the result also meets the float64 oracle / restatement under the project's existing rules (features
     1e-4 max(1, max|ref|), scores 1e-4 relative, decisions exact), so that the file does not rest on the code under test alone;
  3. no guard byte around a skewed output (or input) changes;
  4. no guard value of an input shows up: finite results stay finite and the peak a normalised VAD call divided by is the signal's own.

Skewed inputs go through the public api with torch views; api allocates its own outputs (except MfccPlan.run(out=)), so skewed outputs
are called through the C-ABI (ctx._lib.ssp_*, where = SSP_DEVICE).  Skews: float32 / int32 4, 8, 12 bytes; int16 2, 6 (odd samples) and
8; uint8 1 and 3.  Arrays whose base decides a code path take every skew, the others 4 bytes.

ssp_dtw_distances with where = SSP_DEVICE has its skewed, guarded case in tests/test_dtw_instances_gpu.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_oracle as GO    # noqa: E402
import lstm_oracle as LO   # noqa: E402
import skewed as SK        # noqa: E402
import vad_oracle as VO    # noqa: E402
from conftest import synth_audio  # noqa: E402

pytestmark = pytest.mark.gpu

FEAT_TOL = 1e-4
DEVICE = 1
_BASE = {}     # aligned results, computed once per case and shared by its skews
_CACHE = {}    # packed models, plans, inputs


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def env():
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import api, _lib
    return pkg, api, _lib, api.default_context(torch_stream=True)


def assert_feat_close(got, ref, what=""):
    """the project's feature rule (tests/test_gpu_parity.py): max |got - ref| <= 1e-4 max(1, max |ref|), same non-finite pattern"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), what + ": non-finite pattern differs"
    if fin.any():
        err = float(np.abs(got[fin] - ref[fin]).max())
        print("[measured] %s: max abs err %.3e (ref max %.3e)" % (what, err, np.abs(ref[fin]).max()))
        assert err <= FEAT_TOL * max(1.0, np.abs(ref[fin]).max()), "%s: max abs err %.3e (ref max %.3e)" % (what, err, np.abs(ref[fin]).max())


class Arrays:
    """the device arrays of one call: inputs and outputs at their skews, every one guarded"""

    def __init__(self, skews):
        self.skews, self.tokens, self.outs = dict(skews), [], {}
        self.used = set()

    def skew(self, name):
        self.used.add(name)
        return self.skews.get(name, 0)

    def inp(self, name, values, dtype="float32", guard=None):
        values = np.asarray(values)
        arr, tok = SK.view(values.size, dtype, self.skew(name), values, "torch", guard)
        self.tokens.append((name, tok))
        return arr.view(values.shape)

    def out(self, name, shape, dtype="float32"):
        arr, tok = SK.view(int(np.prod(shape)), dtype, self.skew(name), None, "torch")
        self.tokens.append((name, tok))
        self.outs[name] = arr.view(tuple(shape))
        return self.outs[name]

    def skewed_outputs(self, names):
        return any(self.skews.get(n, 0) for n in names)

    def finish(self, extra=None):
        """wait, check every guard, hand the outputs back as numpy arrays"""
        import torch
        torch.cuda.synchronize()
        assert set(self.skews) <= self.used, "skews for arrays this call does not have: %s" % (set(self.skews) - self.used)
        for name, tok in self.tokens:
            SK.check_guards(tok, name)
        res = {k: v.cpu().numpy() for k, v in self.outs.items()}
        for k, v in (extra or {}).items():
            res[k] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        return res


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def same_bits(got, base, what):
    assert set(got) == set(base), (what, sorted(got), sorted(base))
    for k in sorted(base):
        assert got[k].dtype == base[k].dtype and got[k].shape == base[k].shape, (what, k)
        if not np.array_equal(got[k], base[k], equal_nan=got[k].dtype.kind == "f"):
            bad = np.flatnonzero(~((got[k] == base[k]) | ((got[k] != got[k]) & (base[k] != base[k]))).reshape(-1))
            raise AssertionError("%s: %s differs from the aligned call on %d of %d elements, the first at flat index %d (%r against %r)" % (
                what, k, bad.size, base[k].size, bad[0], got[k].reshape(-1)[bad[0]], base[k].reshape(-1)[bad[0]]))


def run_case(key, run, skews, what):
    """the skewed call against the aligned one (computed once per case)"""
    if key not in _BASE:
        _BASE[key] = run({})
    got = run(skews)
    same_bits(got, _BASE[key], what)
    return got


def ids(sets):
    return ["-".join("%s%d" % (k, v) for k, v in s.items()) or "aligned" for s in sets]


F32 = (4, 8, 12)
I16 = (2, 6, 8)


# ======================================================================================================================= MFCC
MFCC_LENS = [400, 404, 1044, 8000, 100004]    # 1 / 1 / 5 / 48 / 623 frames: the last is more than one 512-frame chunk


def _mfcc_setup(env, preset):
    pkg, api, _, ctx = env

    def make():
        from oracle import ref_cpu as O
        if preset in ("sk0", "sk2"):
            order = int(preset[2])
            tables, otab, fs, lens = pkg.preset_sidekit(delta_order=order), O.sidekit_tables(delta_order=order), 16000, MFCC_LENS
        elif preset == "librosa":
            tables, otab, fs, lens = pkg.preset_librosa(8000, 13), O.librosa_tables(8000, 13), 8000, [1025, 24000]
        elif preset == "inrepo":
            tables, otab, fs, lens = pkg.preset_inrepo(), O.inrepo_tables(8000, 512, 256), 8000, MFCC_LENS
        else:
            raise KeyError(preset)
        sigs = [synth_audio(u, n, fs) for u, n in enumerate(lens)]
        plan = api.MfccPlan(ctx, tables)
        seg = api.Segments.from_lengths(ctx, lens)
        return {"plan": plan, "seg": seg, "fseg": plan.frame_segments(seg), "sigs": sigs, "otab": otab}
    return cached(("mfcc", preset), make)


def _mfcc_run(env, preset, variant, i16):
    s = _mfcc_setup(env, preset)
    flat = np.concatenate(s["sigs"])
    if i16:
        flat = (flat * 20000).astype(np.int16)

    def run(skews):
        a = Arrays(skews)
        x = a.inp("x", flat, "int16" if i16 else "float32")
        out = a.out("out", (s["fseg"].total, s["plan"].d_out))
        back = s["plan"].run(x, s["seg"], s["fseg"], out=out, variant=variant)
        assert back.data_ptr() == out.data_ptr()
        return a.finish()
    return run, s, flat


def _mfcc_oracle(s, flat, got, what):
    from oracle import ref_cpu as O
    cfg, w, fb, dct = s["otab"]
    so, fo = s["seg"].offsets, s["fseg"].offsets
    for u in range(s["seg"].n):
        ref = O.mfcc_pipeline(flat[so[u]:so[u + 1]].astype(np.float32), cfg, w, fb, dct)
        assert_feat_close(got[fo[u]:fo[u + 1]], ref, "%s utterance %d" % (what, u))


MFCC_SKEWS = [{"x": 4}, {"out": 4}, {"x": 8, "out": 12}, {"x": 12, "out": 8}]


@pytest.mark.parametrize("skews", MFCC_SKEWS, ids=ids(MFCC_SKEWS))
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_mfcc_sidekit_input_and_output_skewed(env, variant, order, skews):
    """generic, workgroup and wave-stream kernels on the ragged batch: the workgroup kernel's head / 16-byte / tail store phases
    (mfcc_fast.hip) depend on the output base, the stream kernel's sample stage takes any dword-aligned start"""
    run, s, flat = _mfcc_run(env, "sk%d" % order, variant, False)
    what = "mfcc sidekit order %d variant %d %s" % (order, variant, skews)
    got = run_case(("mfcc", order, variant), run, skews, what)["out"]
    assert np.isfinite(got).all(), what
    if skews == MFCC_SKEWS[2]:
        _mfcc_oracle(s, flat, got, what)


I16_SKEWS = [{"x": 2}, {"x": 6}, {"x": 8}, {"x": 2, "out": 4}]


@pytest.mark.parametrize("skews", I16_SKEWS, ids=ids(I16_SKEWS))
@pytest.mark.parametrize("variant", [2, 3])
def test_mfcc_int16_input_on_odd_samples(env, variant, skews):
    """ssp_mfcc_run_i16 with the device array on an odd sample (2, 6) or dword- but not 16-byte aligned (8): widen_i16_kernel's scalar
    loop instead of its 16-byte read.  Bit-equal to the aligned int16 call and to the float32 call on the same integers."""
    run, s, flat = _mfcc_run(env, "sk2", variant, True)
    what = "mfcc int16 variant %d %s" % (variant, skews)
    got = run_case(("mfcc16", variant), run, skews, what)["out"]
    assert np.isfinite(got).all(), what
    if skews == I16_SKEWS[0]:
        a = Arrays({})
        xf = a.inp("x", flat.astype(np.float32))
        ref = s["plan"].run(xf, s["seg"], s["fseg"], variant=variant)
        assert np.array_equal(a.finish({"ref": ref})["ref"], got), what + ": int16 input differs from its float32 image"
        _mfcc_oracle(s, flat, got, what)


OTHER_SKEWS = [{"x": 4}, {"out": 4}, {"x": 8, "out": 12}]


@pytest.mark.parametrize("skews", OTHER_SKEWS, ids=ids(OTHER_SKEWS))
@pytest.mark.parametrize("preset,variant", [("librosa", 4), ("inrepo", 0)])
def test_mfcc_other_dialects_skewed(env, preset, variant, skews):
    """the 2048-point wave-stream kernel on the librosa preset (1025 and 24000 samples) and the in-repo 13-d dialect (auto)"""
    run, s, flat = _mfcc_run(env, preset, variant, False)
    what = "mfcc %s variant %d %s" % (preset, variant, skews)
    got = run_case(("mfcc", preset, variant), run, skews, what)["out"]
    assert np.isfinite(got).all(), what
    if skews == OTHER_SKEWS[2]:
        _mfcc_oracle(s, flat, got, what)


SCALED_SKEWS = [{"out": 4}, {"out": 8}, {"out": 12}, {"x": 4}]


@pytest.mark.parametrize("skews", SCALED_SKEWS, ids=ids(SCALED_SKEWS))
def test_mfcc_scaling_inside_the_stream_kernel_on_a_skewed_output(env, skews):
    """the 26-column per-utterance scaled instance (tests/test_gpu_parity.py test_scaling_instances_at_every_width's preset): a
    machine-filling batch of single-chunk utterances, so the wave that walks an utterance rewrites its own rows — 8 bytes per lane,
    since the column count is even — and a row base is 8-byte aligned only if the output base is (4 and 12: it is not)."""
    pkg, api, _, ctx = env
    from oracle import ref_cpu as O
    lens = [(1044, 400, 1200, 404, 880)[u % 5] for u in range(8000)]   # 5 / 1 / 6 / 1 / 4 frames, 27 200 frames in all

    def make():
        rng = np.random.default_rng(26)
        plan = api.MfccPlan(ctx, pkg.preset_sidekit(fs=16000, delta_order=1, cmvn=1))
        seg = api.Segments.from_lengths(ctx, lens)
        return plan, seg, plan.frame_segments(seg), (0.3 * rng.standard_normal(sum(lens))).astype(np.float32)
    plan, seg, fseg, flat = cached("mfcc26", make)
    assert plan.d_out == 26 and max(np.diff(fseg.offsets)) == 6

    def run(sk):
        a = Arrays(sk)
        x = a.inp("x", flat)
        out = a.out("out", (fseg.total, 26))
        plan.run(x, seg, fseg, out=out, variant=3)
        return a.finish()
    what = "mfcc 26-d scaled %s" % skews
    got = run_case("mfcc26", run, skews, what)["out"]
    assert np.isfinite(got).all(), what
    if skews == SCALED_SKEWS[0]:
        cfg, w, fb, dct = O.sidekit_tables(delta_order=1, cmvn=1)
        for u in (0, 1, 2, 4, 4002, 7999):
            ref = O.mfcc_pipeline(flat[seg.offsets[u]:seg.offsets[u + 1]], cfg, w, fb, dct)
            assert_feat_close(got[fseg.offsets[u]:fseg.offsets[u + 1]], ref, "%s utterance %d" % (what, u))


# ======================================================================================================================= VAD
VAD_LENS = [1, 127, 128, 129, 255, 300, 257, 1000, 20001]   # odd lengths put later utterances on odd samples; utterance 5 is silent
VAD_SILENT = 5


def _vad_signals(kind):
    def make():
        rng = np.random.default_rng(31)
        sigs = [VO.random_signal(rng, n) for n in VAD_LENS]
        sigs[0][:] = 77
        sigs[VAD_SILENT][:] = 0
        long = 131.0 * rng.standard_normal(VAD_LENS[-1])
        long[5000:11000] += VO.burst(rng, 6000, f0=150.0, amp=20000.0)   # 46 loud frames: a run the detector flushes
        sigs[-1] = np.round(long).astype(np.int16)
        assert max(int(np.abs(s.astype(np.int32)).max()) for s in sigs) < 32767   # (the int16 guard value is nobody's peak)
        if kind == "i16":
            return sigs
        if kind == "f32":
            return [s.astype(np.float32) for s in sigs]
        return [(s.astype(np.float32) / np.float32(32768.0)) * np.float32(2.0) for s in sigs]   # "unit": taken as they are
    return cached(("vadsig", kind), make)


def _vad_features_run(env, kind, normalize, step):
    _, api, _lib, ctx = env
    sigs = _vad_signals(kind)
    flat = np.concatenate(sigs)
    seg = cached("vadseg", lambda: api.Segments.from_lengths(ctx, VAD_LENS))
    fseg = cached(("vadfseg", step), lambda: api.vad_frame_segments(ctx, seg, step))
    names = ("zcr", "power", "entropy")

    def run(skews):
        a = Arrays(skews)
        # (float32 guards: a large finite value — the peak's fmaxf would drop a NaN, this one would become the peak)
        x = a.inp("x", flat, "int16" if kind == "i16" else "float32", None if kind == "i16" else SK.BIG)
        if a.skewed_outputs(names) or not skews:
            o = [a.out(n, (fseg.total,)) for n in names]
            _lib.check(ctx._lib.ssp_vad_features(ctx._h, p(x), 1 if kind == "i16" else 0, seg._h, fseg._h, 256, step, 1 if normalize else 0, 0,
                                                 p(o[0]), p(o[1]), p(o[2]), DEVICE, None))
            return a.finish()
        for n in names:
            a.skew(n)
        z, pw, en, _ = api.vad_features(ctx, x, seg, fseg, step=step, normalize=normalize)
        return a.finish({"zcr": z, "power": pw, "entropy": en})
    return run, sigs, fseg


def _vad_oracle_check(sigs, fseg, got, normalize, step, what):
    """tests/test_vad_gpu.py's rules: power 1e-4 relative, entropy 1e-4 max(1, max|ref|), NaN pattern equal, gated zcr equal outside
    the 1e-4 band of the 0.1 gate; and the peak the kernel divided by is the utterance's own"""
    o = fseg.offsets
    for u, s in enumerate(sigs):
        x = VO.normalise(s) if normalize else np.asarray(s, dtype=np.float64)
        rz, rp, re_ = VO.features(VO.enframe(x, step))
        gz, gp, ge = (got[k][o[u]:o[u + 1]].astype(np.float64) for k in ("zcr", "power", "entropy"))
        assert gp.shape == rp.shape, (what, u)
        assert np.array_equal(np.isnan(gp), np.isnan(rp)) and np.array_equal(np.isnan(ge), np.isnan(re_)), "%s utterance %d: NaN pattern" % (what, u)
        assert not np.isnan(gz).any()
        fin = ~np.isnan(rp)
        assert (np.abs(gp[fin] - rp[fin]) <= FEAT_TOL * np.abs(rp[fin])).all(), "%s utterance %d: power" % (what, u)
        if fin.any():
            assert np.abs(ge[fin] - re_[fin]).max() <= FEAT_TOL * max(1.0, np.abs(re_[fin]).max()), "%s utterance %d: entropy" % (what, u)
        clear = fin & ~(np.abs(rp - 0.1) <= VO.BAND * 0.1)
        assert np.array_equal(gz[clear], rz[clear]), "%s utterance %d: gated zcr" % (what, u)
        if normalize and fin.any():
            own = float(np.abs(np.asarray(s, dtype=np.float64)).max())
            raw = float((np.asarray(s[:256], dtype=np.float64) ** 2).sum())
            implied = np.sqrt(raw / gp[0])
            assert abs(implied - own) <= 1e-3 * own and abs(implied - 32767.0) > 1e-3 * 32767.0, "%s utterance %d: divided by %g, peak %g" % (what, u, implied, own)
    assert np.isnan(got["power"][o[VAD_SILENT]:o[VAD_SILENT + 1]]).all() == bool(normalize)


VAD_CASES = [("f32", s) for s in F32] + [("i16", s) for s in I16]


@pytest.mark.parametrize("step", [128, 256])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind,skew", VAD_CASES)
def test_vad_features_samples_skewed(env, kind, skew, normalize, step):
    """the sample array at every skew through api.vad_features.  normalize runs the peak kernel: its 16-byte groups on an aligned
    base, the scalar V = 1 instance on any other; the feature kernel moves an int16 utterance on an odd sample down to the dword
    below and zeroes the foreign sample.  One digitally silent utterance: NaN power / entropy with normalize, as the aligned call."""
    k = kind if (normalize or kind == "i16") else "unit"
    run, sigs, fseg = _vad_features_run(env, k, normalize, step)
    what = "vad features %s normalize %d step %d x skewed %d" % (k, normalize, step, skew)
    got = run_case(("vadf", k, normalize, step), run, {"x": skew}, what)
    if skew in (4, 2):
        _vad_oracle_check(sigs, fseg, got, normalize, step, what)


VAD_OUT_SKEWS = [{"zcr": 4, "power": 8, "entropy": 12}, {"x": 1, "zcr": 12, "power": 4, "entropy": 4}]


@pytest.mark.parametrize("skews", VAD_OUT_SKEWS, ids=ids(VAD_OUT_SKEWS))
@pytest.mark.parametrize("step", [128, 256])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_vad_features_outputs_skewed(env, kind, normalize, step, skews):
    """zcr_out, power_out and entropy_out skewed, through ssp_vad_features itself ("x": 1 stands for one element size: 4 / 2 bytes)"""
    k = kind if (normalize or kind == "i16") else "unit"
    skews = dict(skews)
    if "x" in skews:
        skews["x"] = 2 if kind == "i16" else 4
    run, sigs, fseg = _vad_features_run(env, k, normalize, step)
    what = "vad features %s normalize %d step %d %s" % (k, normalize, step, skews)
    got = run_case(("vadf", k, normalize, step), run, skews, what)
    if "x" not in skews:
        _vad_oracle_check(sigs, fseg, got, normalize, step, what)


DETECT_SKEWS = [{"mask": 1, "count": 4}, {"mask": 3}, {"zcr": 4, "plane": 4}, {"zcr": 8, "plane": 12, "mask": 3, "count": 4}]


@pytest.mark.parametrize("skews", DETECT_SKEWS, ids=ids(DETECT_SKEWS))
@pytest.mark.parametrize("mode", [0, 1])
def test_vad_detect_planes_mask_and_counts_skewed(env, mode, skews):
    """both detectors on the planes of the batch above (NaNs of the silent utterance included): mask_out on odd bytes, n_speech_out and
    the planes on dwords; decisions equal to the restatement's on the same float32 planes"""
    _, api, _lib, ctx = env
    run_f, sigs, fseg = _vad_features_run(env, "i16", True, 128)
    if ("vadf", "i16", True, 128) not in _BASE:
        _BASE[("vadf", "i16", True, 128)] = run_f({})
    planes = _BASE[("vadf", "i16", True, 128)]
    plane = planes["power"] if mode == 0 else planes["entropy"]
    gate, lo, hi, min_len = 35.0, 0.3, 12.0, 16
    thr = lo if mode == 0 else 0.4

    def run(sk):
        a = Arrays(sk)
        z = a.inp("zcr", planes["zcr"])
        q = a.inp("plane", plane)
        if a.skewed_outputs(("mask", "count")) or not sk:
            m, c = a.out("mask", (fseg.total,), "uint8"), a.out("count", (fseg.n,), "int32")
            _lib.check(ctx._lib.ssp_vad_detect(ctx._h, p(z) if mode == 0 else None, p(q), fseg._h, mode, gate, thr, hi, min_len, p(m), p(c), DEVICE, None))
            return a.finish()
        a.skew("mask"), a.skew("count")
        m, c = api.vad_detect(ctx, z if mode == 0 else None, q, fseg, mode=mode, zcr_gate=gate, ampl=thr, amph=hi, min_len=min_len)
        return a.finish({"mask": m, "count": c})
    what = "vad detect mode %d %s" % (mode, skews)
    got = run_case(("vadd", mode), run, skews, what)
    o = fseg.offsets
    marked = 0
    for u in range(fseg.n):
        zz, pp = planes["zcr"][o[u]:o[u + 1]], plane[o[u]:o[u + 1]]
        ref = VO.detect(zz, pp, gate, np.float32(lo), np.float32(hi), min_len) if mode == 0 else VO.detect_frequency(pp, np.float32(0.4))
        assert np.array_equal(got["mask"][o[u]:o[u + 1]], ref), (what, u)
        assert got["count"][u] == int(ref.sum()), (what, u)
        marked += int(ref.sum())
    assert 0 < marked < fseg.total   # (the batch exercises both decisions)


# ======================================================================================================================= GMM
GMM_LENS = [1, 70, 300]


def _gmm_setup(env, D):
    _, api, _, ctx = env

    def make():
        rng = np.random.default_rng(50 + D)
        K, M = 16, 5
        w = rng.dirichlet(5 * np.ones(K))
        mu = rng.standard_normal((K, D))
        cov = rng.uniform(0.5, 2.0, (K, D))
        mus = [mu] + [mu + 0.5 * rng.standard_normal((K, D)) for _ in range(M - 1)]
        feats = []
        for j, n in enumerate(GMM_LENS):
            comp = rng.choice(K, size=n, p=w)
            feats.append((mus[1 + j][comp] + np.sqrt(cov[comp]) * rng.standard_normal((n, D))).astype(np.float32))
        sc = api.GmmScorer(ctx, np.stack([w] * M), np.stack(mus), np.stack([cov] * M), has_ubm=True)
        return {"sc": sc, "seg": api.Segments.from_lengths(ctx, GMM_LENS), "X": np.vstack(feats), "feats": feats, "w": w, "mus": mus, "cov": cov}
    return cached(("gmm", D), make)


GMM_SKEWS = [{"feats": 4}, {"feats": 8}, {"feats": 12}, {"feats": 4, "loglik": 4, "scores": 8, "argmax": 12}, {"loglik": 12, "scores": 4, "argmax": 4}]


@pytest.mark.parametrize("skews", GMM_SKEWS, ids=ids(GMM_SKEWS))
@pytest.mark.parametrize("loglik", [True, False])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("D", [39, 40])
def test_gmm_score_features_and_outputs_skewed(env, D, precision, loglik, skews):
    """5 models with a UBM, K = 16, utterances of 1 / 70 / 300 frames.  stage_frames (gmm.hip) takes float4 or scalar staging of a
    workgroup's frames from the address of its first row: at D = 40 the feats base alone decides it.  With and without loglik_out
    (without: the per-utterance means are formed inside the scoring kernel)."""
    _, api, _lib, ctx = env
    from oracle import ref_cpu as O
    g = _gmm_setup(env, D)
    sc, seg = g["sc"], g["seg"]
    skews = {k: v for k, v in skews.items() if loglik or k != "loglik"}
    F, U, M = seg.total, seg.n, sc.n_models

    def run(sk):
        a = Arrays(sk)
        x = a.inp("feats", g["X"])
        names = ("loglik", "scores", "argmax") if loglik else ("scores", "argmax")
        if a.skewed_outputs(names) or not sk:
            ll = a.out("loglik", (M, F)) if loglik else None
            s_, am = a.out("scores", (U, M)), a.out("argmax", (U,), "int32")
            _lib.check(ctx._lib.ssp_gmm_score(sc._h, p(x), seg._h, p(ll), p(s_), p(am), DEVICE, precision, None))
            return a.finish()
        for n in names:
            a.skew(n)
        r = sc.score(x, seg, loglik=loglik, precision=precision)
        return a.finish({n: r[n] for n in names})
    what = "gmm score D %d precision %d loglik %d %s" % (D, precision, loglik, skews)
    got = run_case(("gmm", D, precision, loglik), run, skews, what)
    assert all(np.isfinite(v).all() for v in got.values()), what
    if skews.get("feats") == 4:
        ref = np.array([[O.gmm_score(g["w"], m, g["cov"], f) for m in g["mus"]] for f in g["feats"]])
        assert (np.abs(got["scores"] - ref) <= FEAT_TOL * np.abs(ref)).all(), (what, np.abs(got["scores"] - ref).max())
        assert np.array_equal(got["argmax"], (ref[:, 1:] - ref[:, :1]).argmax(1)), what
        if loglik:
            for m in range(M):
                np.testing.assert_allclose(got["loglik"][m], O.gmm_score_samples(g["w"], g["mus"][m], g["cov"], g["X"]), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("skew", F32)
def test_gmm_em_stats_device_frames_skewed(env, skew):
    """ssp_gmm_em_stats on a skewed device X (K = 16, D = 39, 500 frames); its outputs are host arrays"""
    _, api, _, ctx = env
    from oracle import ref_cpu as O
    rng = np.random.default_rng(61)
    K, D, n = 16, 39, 500
    mu = rng.standard_normal((K, D)) * 1.5
    X = (mu[rng.integers(0, K, n)] + rng.standard_normal((n, D))).astype(np.float32)
    w, cov = rng.dirichlet(5 * np.ones(K)), rng.uniform(0.5, 2.0, (K, D))

    def run(sk):
        a = Arrays(sk)
        st = api.gmm_em_stats(ctx, w, mu, cov, a.inp("X", X))
        return a.finish({"nk": st["nk"], "sx": st["sx"], "sxx": st["sxx"], "ll": np.array([st["loglik_sum"]])})
    got = run_case("em", run, {"X": skew}, "em stats X skewed %d" % skew)
    assert all(np.isfinite(v).all() for v in got.values())
    if skew == 4:
        nk, sx, sxx, ll = O.gmm_em_stats(w, mu, cov, X.astype(np.float64))
        assert abs(got["ll"][0] - ll) <= 2e-5 * abs(ll)   # (tests/test_gpu_parity.py test_gmm_em_stats_shapes' rules)
        assert np.allclose(got["nk"], nk, rtol=1e-4, atol=1e-4 * nk.max())
        assert np.allclose(got["sx"], sx, rtol=1e-4, atol=1e-4 * np.abs(sx).max())
        assert np.allclose(got["sxx"], sxx, rtol=1e-4, atol=1e-4 * np.abs(sxx).max())


# ======================================================================================================================= cosine, centroids
COS_SKEWS = [{"X": 4}, {"C": 4}, {"X": 8, "C": 12}, {"dist": 4, "argmin": 4, "min": 4}, {"dist": 8}, {"X": 12, "C": 8, "dist": 12}]
COS_CASES = [(128, 8, 0), (128, 7, 0), (33, 8, 0), (128, 8, 1), (128, 8, 2)]


@pytest.mark.parametrize("skews", COS_SKEWS, ids=ids(COS_SKEWS))
@pytest.mark.parametrize("d,S,precision", COS_CASES)
def test_cosine_identify_embeddings_centroids_and_distances_skewed(env, d, S, precision, skews):
    """N = 70.  The scoring kernels store dist_out element by element whatever the base (the 16-byte store of cosine.hip belongs to the
    kernel's GEMM mode, which ssp_dense_forward reaches: test_dense_forward_input_and_output_skewed); what a skew changes here is the
    address of every operand row.  precision 1 / 2 (bf16x3 sweep, cascade) give arg-min and minimum only, so the distance skew falls
    on min_out there."""
    _, api, _lib, ctx = env
    from oracle import ref_cpu as O
    N = 70
    rng = np.random.default_rng(7 * d + S)
    Cn = rng.standard_normal((S, d)).astype(np.float32)
    X = (Cn[rng.integers(0, S, N)] + 0.7 * rng.standard_normal((N, d))).astype(np.float32)
    dist = precision == 0
    if not dist:
        skews = {("min" if k == "dist" else k): v for k, v in skews.items()}
    names = ("dist", "argmin", "min") if dist else ("argmin", "min")

    def run(sk):
        a = Arrays(sk)
        x, c = a.inp("X", X), a.inp("C", Cn)
        if a.skewed_outputs(names) or not sk:
            dm = a.out("dist", (N, S)) if dist else None
            am, mv = a.out("argmin", (N,), "int32"), a.out("min", (N,))
            _lib.check(ctx._lib.ssp_cosine_identify2(ctx._h, p(x), N, d, p(c), S, p(dm), p(am), p(mv), DEVICE, precision, None))
            return a.finish()
        for n in names:
            a.skew(n)
        r = api.cosine_identify(ctx, x, c, dist=dist, precision=precision, counts=False)
        return a.finish({n: r[n] for n in names})
    what = "cosine d %d S %d precision %d %s" % (d, S, precision, skews)
    got = run_case(("cos", d, S, precision), run, skews, what)
    assert all(np.isfinite(v).all() for v in got.values()), what
    if skews in (COS_SKEWS[2], COS_SKEWS[3]) or skews == {"min": 4, "argmin": 4}:
        ref = O.cosine_matrix(X, Cn)
        assert np.array_equal(got["argmin"], ref.argmin(1)), what
        if dist:   # (tests/test_gpu_parity.py test_cosine_odd_shapes_vs_oracle's bound)
            np.testing.assert_allclose(got["dist"], ref, rtol=0, atol=3e-6)
        # precision 1 / 2: ssp.h's proven bounds on the minimum, as test_cosine_split_precision_argmin_equals_fp32_path_on_golden takes them
        np.testing.assert_allclose(got["min"], ref.min(1), rtol=0, atol=(3e-6, 2e-4, 4.1e-3)[precision])


def test_cosine_identify_plain_entry_point_skewed(env):
    """ssp_cosine_identify (no precision argument) with every array skewed: the same bits as ssp_cosine_identify2 at precision 0"""
    _, api, _lib, ctx = env
    N, d, S = 70, 128, 8
    rng = np.random.default_rng(3)
    Cn = rng.standard_normal((S, d)).astype(np.float32)
    X = (Cn[rng.integers(0, S, N)] + 0.7 * rng.standard_normal((N, d))).astype(np.float32)

    def run(sk, two=False):
        a = Arrays(sk)
        x, c = a.inp("X", X), a.inp("C", Cn)
        dm, am, mv = a.out("dist", (N, S)), a.out("argmin", (N,), "int32"), a.out("min", (N,))
        if two:
            _lib.check(ctx._lib.ssp_cosine_identify2(ctx._h, p(x), N, d, p(c), S, p(dm), p(am), p(mv), DEVICE, 0, None))
        else:
            _lib.check(ctx._lib.ssp_cosine_identify(ctx._h, p(x), N, d, p(c), S, p(dm), p(am), p(mv), DEVICE, None))
        return a.finish()
    got = run_case("cos1", run, {"X": 4, "C": 8, "dist": 12, "argmin": 4, "min": 8}, "ssp_cosine_identify")
    same_bits(got, run({}, two=True), "ssp_cosine_identify against ssp_cosine_identify2")


@pytest.mark.parametrize("skews", [{"X": 4}, {"X": 8, "labels": 4}, {"X": 12, "out": 4}], ids=ids([{"X": 4}, {"X": 8, "labels": 4}, {"X": 12, "out": 4}]))
@pytest.mark.parametrize("N,d,S", [(600, 8, 3), (2049, 33, 5)])
def test_centroids_rows_skewed(env, N, d, S, skews):
    _, api, _lib, ctx = env
    rng = np.random.default_rng(N + d)
    X = (rng.standard_normal((N, d)) * 2 + 0.5).astype(np.float32)
    lab = rng.integers(0, S, N).astype(np.int32)

    def run(sk):
        a = Arrays(sk)
        x, lb = a.inp("X", X), a.inp("labels", lab, "int32")
        if a.skewed_outputs(("out",)) or not sk:
            o = a.out("out", (S, d))
            _lib.check(ctx._lib.ssp_centroids(ctx._h, p(x), p(lb), N, d, S, p(o), DEVICE, None))
            return a.finish()
        a.skew("out")
        return a.finish({"out": api.centroids(ctx, x, lb, S)})
    got = run_case(("cen", N, d), run, skews, "centroids %s" % skews)["out"]
    if "out" in skews or skews == {"X": 4}:
        for s in range(S):   # (test_centroids_shapes_and_order's bound)
            np.testing.assert_allclose(got[s], X[lab == s].astype(np.float64).mean(axis=0), rtol=0, atol=1e-6)


# ======================================================================================================================= dense, packed network
DENSE_SKEWS = [{"X": 4}, {"Y": 4}, {"Y": 8}, {"Y": 12}, {"X": 8, "Y": 12, "Wt": 4, "bias": 4}]


@pytest.mark.parametrize("skews", DENSE_SKEWS, ids=ids(DENSE_SKEWS))
@pytest.mark.parametrize("N,d_in,units", [(77, 1274, 256), (77, 50, 10), (77, 50, 12), (77, 40, 32)])
def test_dense_forward_input_and_output_skewed(env, N, d_in, units, skews):
    """Two kernels store Y 16 bytes at a time when units is a multiple of 4 and the base is aligned, element by element otherwise:
    dense_kernel (d_in > 256: 1274 -> 256) and the register GEMM of cosine.hip (d_in <= 256: 50 -> 12 and 40 -> 32, where only the base
    decides; 50 -> 10 takes the element stores on every base)."""
    _, api, _lib, ctx = env
    from oracle import ref_cpu as O
    rng = np.random.default_rng(N + d_in)
    X = rng.standard_normal((N, d_in)).astype(np.float32)
    W = (rng.standard_normal((d_in, units)) / np.sqrt(d_in)).astype(np.float32)
    b = rng.standard_normal(units).astype(np.float32)

    def run(sk):
        a = Arrays(sk)
        x, wt, bb = a.inp("X", X), a.inp("Wt", np.ascontiguousarray(W.T)), a.inp("bias", b)
        if a.skewed_outputs(("Y",)) or not sk:
            y = a.out("Y", (N, units))
            _lib.check(ctx._lib.ssp_dense_forward(ctx._h, p(x), N, d_in, p(wt), p(bb), units, 1, p(y), DEVICE, None))
            return a.finish()
        a.skew("Y")
        return a.finish({"Y": api.dense_forward(ctx, x, wt, bb, relu=True)})
    what = "dense %d x %d -> %d %s" % (N, d_in, units, skews)
    got = run_case(("dense", d_in, units), run, skews, what)["Y"]
    assert np.isfinite(got).all(), what
    if "Wt" in skews:
        assert_feat_close(got, O.dense_net_forward(X, [(W, b, "relu")]), what)


DNN_SKEWS = [{"X": 4}, {"Y": 4}, {"Y": 8}, {"X": 12, "Y": 12}]


@pytest.mark.parametrize("skews", DNN_SKEWS, ids=ids(DNN_SKEWS))
def test_packed_network_forward_input_and_output_skewed(env, skews):
    """dims [40, 32, 16], N = 70: the chained kernel's 16-byte or scalar stores of Y (dnn_chain.hip)"""
    _, api, _lib, ctx = env
    from oracle import ref_cpu as O
    dims, N = [40, 32, 16], 70
    rng = np.random.default_rng(88)
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               (0.2 * rng.standard_normal(dims[i + 1])).astype(np.float32), "relu" if i == 0 else "linear") for i in range(2)]
    net = cached("dnn", lambda: api.DnnForward(ctx, [(np.ascontiguousarray(W.T), b, act == "relu") for W, b, act in layers]))

    def run(sk):
        a = Arrays(sk)
        x = a.inp("X", X)
        if a.skewed_outputs(("Y",)) or not sk:
            y = a.out("Y", (N, dims[-1]))
            _lib.check(ctx._lib.ssp_dnn_forward(net._h, p(x), N, p(y), DEVICE, None))
            return a.finish()
        a.skew("Y")
        return a.finish({"Y": net.forward(x)})
    got = run_case("dnn", run, skews, "dnn %s" % skews)["Y"]
    if len(skews) == 2:
        assert_feat_close(got, O.dense_net_forward(X, layers), "dnn %s" % skews)


# ======================================================================================================================= LSTM, GRU network
LSTM_SKEWS = [{"feats": 4}, {"h": 4}, {"h": 8}, {"feats": 8, "h": 12}]


@pytest.mark.parametrize("skews", LSTM_SKEWS, ids=ids(LSTM_SKEWS))
@pytest.mark.parametrize("H", [16, 128])
def test_lstm_forward_frames_and_last_state_skewed(env, H, skews):
    """D = 13 (rows of 52 bytes), 70 sequences of 1 / 5 / 98 frames; h_out rows are multiples of 16 bytes, so the base alone picks the
    16-byte or the scalar store of the last state (lstm.hip)"""
    _, api, _lib, ctx = env
    D, n_seq, act = 13, 70, "sigmoid"
    lens = [(1, 5, 98)[s % 3] for s in range(n_seq)]

    def make():
        rng = np.random.default_rng(300 + H)
        W, U, b = LO.keras_init(rng, D, H, 1.5)
        X = (3.0 * rng.standard_normal((sum(lens), D))).astype(np.float32)
        return W, U, b, X, api.LstmForward(ctx, W, U, b, act), api.Segments.from_lengths(ctx, lens)
    W, U, b, X, net, seg = cached(("lstm", H), make)

    def run(sk):
        a = Arrays(sk)
        x = a.inp("feats", X)
        if a.skewed_outputs(("h",)) or not sk:
            h = a.out("h", (n_seq, H))
            _lib.check(ctx._lib.ssp_lstm_forward(net._h, p(x), seg._h, p(h), DEVICE, None))
            return a.finish()
        a.skew("h")
        return a.finish({"h": net.forward(x, seg)})
    what = "lstm H %d %s" % (H, skews)
    got = run_case(("lstm", H), run, skews, what)["h"]
    assert np.isfinite(got).all(), what
    if len(skews) == 2:
        assert_feat_close(got, LO.forward_ragged(W, U, b, X, seg.offsets, act), what)


GRU_SKEWS = [{"X": 4}, {"seq": 4}, {"seq": 8}, {"seq": 12, "X": 8}, {"mean": 4}, {"seq": 4, "mean": 12}]


@pytest.mark.parametrize("skews", GRU_SKEWS, ids=ids(GRU_SKEWS))
@pytest.mark.parametrize("reset_after", [False, True])
def test_gru_forward_sequence_in_place_or_through_the_workspace(env, reset_after, skews):
    """(T, d_in, H, N) = (5, 7, 48, 37).  A 16-byte aligned seq_out is written in place; any other goes through the workspace and a
    device-to-device copy (gru.hip): bit-equality with the in-place route is the check on that route, ssp_gru_last_slab that it ran."""
    _, api, _lib, ctx = env
    T, d_in, H, N, act = 5, 7, 48, 37, "sigmoid"

    def make():
        rng = np.random.default_rng(500 + reset_after)
        W, U, b = GO.gru_init(rng, d_in, H, reset_after, 1.5)
        X = (3 * rng.standard_normal((N, T, d_in))).astype(np.float32)
        return W, U, b, X, api.GruForward(ctx, W, U, b, act, reset_after)
    W, U, b, X, net = cached(("gru", reset_after), make)

    def run(sk):
        a = Arrays(sk)
        x = a.inp("X", X)
        if a.skewed_outputs(("seq", "mean")) or not sk:
            seq, mean = a.out("seq", (N, T, H)), a.out("mean", (N, H))
            _lib.check(ctx._lib.ssp_gru_forward(net._h, p(x), N, T, p(seq), p(mean), DEVICE, None))
            assert net.last_slab == N
            return a.finish()
        a.skew("seq"), a.skew("mean")
        return a.finish({"seq": net.forward(x), "mean": net.forward(x, mean=True)})
    what = "gru reset_after %d %s" % (reset_after, skews)
    got = run_case(("gru", reset_after), run, skews, what)
    assert np.isfinite(got["seq"]).all() and np.isfinite(got["mean"]).all(), what
    if len(skews) == 2:
        ref = GO.gru(W, U, b, X, act, reset_after)
        assert_feat_close(got["seq"], ref, what + " sequence")
        assert_feat_close(got["mean"], GO.time_mean(ref), what + " mean")


CONV_SKEWS = [{"X": 4}, {"Y": 4}, {"X": 8, "K": 4, "bias": 4, "Y": 12}]


@pytest.mark.parametrize("skews", CONV_SKEWS, ids=ids(CONV_SKEWS))
def test_conv2d_same_skewed(env, skews):
    """(5, 3) input, 3 x 3 kernel, 16 filters, stride 2"""
    _, api, _lib, ctx = env
    rng = np.random.default_rng(16)
    N, T, D, k, F = 3, 5, 3, 3, 16
    X = (3 * rng.standard_normal((N, T, D))).astype(np.float32)
    K = GO.glorot(rng, (k, k, 1, F), k * k, k * k * F)
    bc = (0.1 * rng.standard_normal(F)).astype(np.float32)
    To, Do = api.conv2d_same_out_shape(T, D, (2, 2))

    def run(sk):
        a = Arrays(sk)
        x, kk, bb = a.inp("X", X), a.inp("K", K), a.inp("bias", bc)
        if a.skewed_outputs(("Y",)) or not sk:
            y = a.out("Y", (N, To, Do * F))
            _lib.check(ctx._lib.ssp_conv2d_same_forward(ctx._h, p(x), N, T, D, p(kk), p(bb), k, k, F, 2, 2, p(y), DEVICE, None))
            return a.finish()
        a.skew("Y")
        return a.finish({"Y": api.conv2d_same(ctx, x, kk, bb, (2, 2))})
    got = run_case("conv", run, skews, "conv %s" % skews)["Y"]
    if "K" in skews:
        assert_feat_close(got, GO.conv2d_same(X, K, bc, (2, 2)), "conv %s" % skews)


L2_SKEWS = [{"X": 4}, {"Y": 4}, {"X": 8, "Y": 12}]


@pytest.mark.parametrize("skews", L2_SKEWS, ids=ids(L2_SKEWS))
@pytest.mark.parametrize("d", [33, 512])
def test_l2_normalize_skewed(env, d, skews):
    _, api, _lib, ctx = env
    N = 37
    X = (2 * np.random.default_rng(d).standard_normal((N, d))).astype(np.float32)
    X[3] = 0   # an all-zero row stays zero

    def run(sk):
        a = Arrays(sk)
        x = a.inp("X", X)
        if a.skewed_outputs(("Y",)) or not sk:
            y = a.out("Y", (N, d))
            _lib.check(ctx._lib.ssp_l2_normalize(ctx._h, p(x), N, d, 1e-12, p(y), DEVICE, None))
            return a.finish()
        a.skew("Y")
        return a.finish({"Y": api.l2_normalize(ctx, x)})
    got = run_case(("l2", d), run, skews, "l2 d %d %s" % (d, skews))["Y"]
    if len(skews) == 2:
        assert_feat_close(got, GO.l2_normalize(X.astype(np.float64)), "l2 d %d" % d)


# ======================================================================================================================= stand-alone feature operations
OP_SKEWS = [{"in": 4}, {"out": 4}, {"in": 8, "out": 12}]


def _op_case(env, key, values, out_shape, raw, via_api, skews, oracle, tol_check=None):
    """one stand-alone operation: `in` through the api when only it is skewed, `out` through the C-ABI"""
    def run(sk):
        a = Arrays(sk)
        x = a.inp("in", values)
        if a.skewed_outputs(("out",)) or not sk:
            o = a.out("out", out_shape)
            raw(x, o)
            return a.finish()
        a.skew("out")
        return a.finish({"out": via_api(x)})
    what = "%s %s" % (key, skews)
    got = run_case(("op", key), run, skews, what)["out"]
    assert np.isfinite(got).all(), what
    if len(skews) == 2:
        (tol_check or assert_feat_close)(got, oracle(), what)


@pytest.mark.parametrize("skews", OP_SKEWS, ids=ids(OP_SKEWS))
def test_enframe_skewed(env, skews):
    """utils.processing.enframe at (400, 160) on 1000 samples: 7 frames, the last ones zero padded"""
    _, api, _lib, ctx = env
    from oracle import ref_cpu as O
    x = synth_audio(1, 1000, 16000)
    L, st = 400, 160
    w = np.ascontiguousarray(O.hamming_sym(L), dtype=np.float32)
    nf = -(-x.shape[0] // st)
    _op_case(env, "enframe", x, (L, nf),
             lambda xi, o: _lib.check(ctx._lib.ssp_enframe(ctx._h, p(xi), x.shape[0], L, st, w.ctypes.data, p(o), DEVICE, None)),
             lambda xi: api.enframe(ctx, xi, L, st, w), skews, lambda: O.enframe(x, L, st))


@pytest.mark.parametrize("skews", OP_SKEWS, ids=ids(OP_SKEWS))
def test_cepstrum_and_spectrum_abs_skewed(env, skews):
    """stMFCC on 50 spectra of 257 bins (40 filters, 13 cepstra, log10(. + 1e-8)) and |re + i im| / L on 50 rows of 2 x 257"""
    _, api, _lib, ctx = env
    from oracle import ref_cpu as O
    rng = np.random.default_rng(9)
    rows, nb, nfilt, nceps, eps = 50, 257, 40, 13, 1e-8
    Xs = np.abs(rng.standard_normal((rows, nb))).astype(np.float32)
    fb = np.abs(rng.standard_normal((nfilt, nb))).astype(np.float32) * (rng.random((nfilt, nb)) < 0.1)
    fb = np.ascontiguousarray(fb, dtype=np.float32)
    dct = np.ascontiguousarray(O.dct2_ortho_matrix(nfilt, nceps), dtype=np.float32)
    _op_case(env, "cepstrum", Xs, (rows, nceps),
             lambda xi, o: _lib.check(ctx._lib.ssp_cepstrum(ctx._h, p(xi), rows, nb, fb.ctypes.data, nfilt, dct.ctypes.data, nceps, 1, 1, eps, p(o), DEVICE, None)),
             lambda xi: api.cepstrum(ctx, xi, fb, dct, 1, 1, eps), skews,
             lambda: np.log10(Xs.astype(np.float64) @ fb.astype(np.float64).T + eps) @ dct.astype(np.float64).T)
    reim = rng.standard_normal((rows, 2 * nb)).astype(np.float32)
    _op_case(env, "spectrum_abs", reim, (rows, nb),
             lambda xi, o: _lib.check(ctx._lib.ssp_spectrum_abs(ctx._h, p(xi), rows, nb, 1.0 / 512, 1, p(o), DEVICE, None)),
             lambda xi: api.spectrum_abs(ctx, xi, nb, 1.0 / 512, 1), skews,
             lambda: np.hypot(reim[:, :nb].astype(np.float64), reim[:, nb:].astype(np.float64)) / 512)


@pytest.mark.parametrize("skews", OP_SKEWS, ids=ids(OP_SKEWS))
@pytest.mark.parametrize("dim", [13, 26])
def test_delta_and_cmvn_skewed(env, dim, skews):
    """ragged, with a 1-frame utterance (tests/test_gpu_parity.py test_delta_cmvn_ragged_batches' bounds)"""
    _, api, _lib, ctx = env
    from oracle import ref_cpu as O
    lens = [70, 1, 3, 200]
    offs = np.concatenate(([0], np.cumsum(lens)))
    X = (np.random.default_rng(dim).standard_normal((sum(lens), dim)) * 3 + 1).astype(np.float32)
    seg = cached("dseg", lambda: api.Segments.from_lengths(ctx, lens))

    def per_utt(fn):
        return np.vstack([fn(X[offs[u]:offs[u + 1]].astype(np.float64)) for u in range(len(lens))])

    def delta_check(got, ref, what):
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), what

    def cmvn_check(got, ref, what):
        assert np.abs(got - ref).max() <= 1e-4, what
    _op_case(env, "delta%d" % dim, X, X.shape,
             lambda xi, o: _lib.check(ctx._lib.ssp_delta(ctx._h, p(xi), seg._h, dim, 2, p(o), DEVICE, None)),
             lambda xi: api.delta_features(ctx, xi, seg, 2), skews, lambda: per_utt(lambda f: O.delta(f, 2)), delta_check)
    _op_case(env, "cmvn%d" % dim, X, X.shape,
             lambda xi, o: _lib.check(ctx._lib.ssp_cmvn(ctx._h, p(xi), seg._h, dim, p(o), DEVICE, None)),
             lambda xi: api.cmvn_features(ctx, xi, seg), skews, lambda: per_utt(O.scale), cmvn_check)


@pytest.mark.parametrize("skews", OP_SKEWS, ids=ids(OP_SKEWS))
def test_plp_post_skewed(env, skews):
    """the PLP back end on ln Bark-band energies of a ragged batch (98 / 1 / 3 / 30 frames; fewer than five frames: the RASTA head)"""
    pkg, api, _lib, ctx = env
    from oracle import ref_cpu as O
    fs, lens = 16000, [98, 1, 3, 30]
    nb = O.plp_num_bands(fs)
    offs = np.concatenate(([0], np.cumsum(lens)))
    cfg, w, fb, eye = O.sidekit_plp_tables(fs)
    logspec = np.vstack([O.mfcc_pipeline(synth_audio(u, 400 + 160 * (T - 1), fs), cfg, w, fb, eye) for u, T in enumerate(lens)]).astype(np.float32)
    assert logspec.shape == (sum(lens), nb)
    seg = cached("pseg", lambda: api.Segments.from_lengths(ctx, lens))
    _op_case(env, "plp_post", logspec, (sum(lens), 13),
             lambda xi, o: _lib.check(ctx._lib.ssp_plp_post(ctx._h, p(xi), seg._h, nb, fs / 2.0, 13, 1, 0.6, p(o), DEVICE, None)),
             lambda xi: api.plp_post(ctx, xi, seg, fs / 2.0), skews,
             lambda: np.vstack([O.plp_from_logspec(logspec[offs[u]:offs[u + 1]].astype(np.float64), fs) for u in range(len(lens))]))
