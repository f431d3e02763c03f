"""GPU tests of the stream ordering of every device-pointer entry point (run with -m gpu on an MI355X).

The other GPU tests give the library inputs at rest on torch's default stream, where three kinds of mistake cannot show: a missing
wait / signal pair around a call on a context that owns its stream, work the C side queues on a stream other than ctx->stream
(include/ssp.h: "all work is enqueued on" a borrowed stream), and a context that borrowed one torch stream used while another is
current.  Here every call is made while the producer of its inputs is still in flight on a side stream and its outputs are consumed on
that stream the moment the call returns (tests/stream_order.py holds the protocol and its proof that the producer WAS in flight), in
three configurations — owned, borrowed-current, borrowed-stale — and the result must equal, bit for bit, the same call on inputs at
rest.  The contract under test is api.Context._ordered's: a device-pointer call sees everything queued on torch's current stream at
the time of the call, and work queued on that stream after the call returns sees the call's results.

So that the file does not rest on the code under test alone, in one configuration (owned) the baseline of every case also meets the
float64 oracle / restatement under the project's existing rules (features 1e-4 max(1, max|ref|), scores 1e-4 relative, decisions
exact).  Shapes are those of tests/test_gpu_alignment.py.

test_harness_detects_a_consumer_that_does_not_wait is the negative control: no library, a consumer on a second stream that does not
wait — it must see the poison.  If it fails, the HARNESS is wrong (it could not detect any race) and nothing else in this file means
anything.

What the cases detect was checked on an MI355X by running the file once with _ordered turned into a plain ``yield``: all 47 owned and
all 47 borrowed-stale cases and the four d_vector tests failed, the 47 borrowed-current cases and the control passed (they need no
ordering from Python).  Counted race by race: 58 of 59 owned, 63 of 64 borrowed-stale and 3 of 5 host-route races differed.  The ones that
cannot differ are listed at ``CANNOT_FAIL_WITHOUT_ORDERING`` below with the reason.  On the parent's api.py (ordering only for a context
that owns its stream) every borrowed-stale case and the four d_vector tests failed and everything else passed.

Context.allgather / allreduce_sum_ are covered: a world of one is initialised in-process (ctx.comm_init(0, 1, uid), as
tests/test_gpu_multirank.py does).  ssp_dtw_distances on device pointers has its race in tests/test_dtw_instances_gpu.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_oracle as GO             # noqa: E402
import lstm_oracle as LO            # noqa: E402
import stream_order as SO           # noqa: E402
import test_gpu_alignment as GA     # noqa: E402  (shapes, signals and the oracle rules; none of its guarded buffers)
import vad_oracle as VO             # noqa: E402
from conftest import synth_audio    # noqa: E402

pytestmark = pytest.mark.gpu

# Races that equal the baseline even with no ordering at all, and why:
#   the numpy routes of LstmNet — the library stages host arrays on its own stream and waits for it on the host before it returns: no
#   torch stream takes part, the check is the returned array alone;
#   allreduce_sum_ in a world of one — the identity, in place: whenever it runs, the buffer ends up holding what the producer wrote
#   (allgather, into a fresh output, does differ).
CANNOT_FAIL_WITHOUT_ORDERING = ("LstmNet.predict (numpy)", "LstmNet.predict_ragged (numpy)", "allreduce_sum_")


@pytest.fixture(scope="module", params=SO.MODES)
def cfg(request):
    c = SO.Config(request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stale():
    """the configuration the d_vector networks live in: they take api.default_context(torch_stream=True) themselves"""
    c = SO.Config("borrowed-stale")
    yield c
    c.close()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def f32(shape):
    return (tuple(shape), "float32")


# ======================================================================================================================= the harness
def test_harness_detects_a_consumer_that_does_not_wait():
    saw_poison, _ = SO.negative_control()
    assert saw_poison, "HARNESS ERROR: a consumer that does not wait for the producer read the produced values — no race can be detected"


# ======================================================================================================================= MFCC
def _mfcc_setup(cfg, preset):
    def make():
        import speech_signal_processing_amd as pkg
        from oracle import ref_cpu as O
        if preset == "sk2":
            tables, otab, fs, lens = pkg.preset_sidekit(delta_order=2), O.sidekit_tables(delta_order=2), 16000, GA.MFCC_LENS
        elif preset == "librosa":
            tables, otab, fs, lens = pkg.preset_librosa(8000, 13), O.librosa_tables(8000, 13), 8000, [1025, 24000]
        else:
            tables, otab, fs, lens = pkg.preset_inrepo(), O.inrepo_tables(8000, 512, 256), 8000, GA.MFCC_LENS
        plan = cfg.api.MfccPlan(cfg.ctx, tables)
        seg = cfg.api.Segments.from_lengths(cfg.ctx, lens)
        return {"plan": plan, "seg": seg, "fseg": plan.frame_segments(seg), "otab": otab,
                "flat": np.concatenate([synth_audio(u, n, fs) for u, n in enumerate(lens)])}
    return cfg.cached(("mfcc", preset), make)


# (preset, variant, int16 PCM, caller's output): generic, workgroup and wave-stream kernels; the librosa dialect's 2048-point stream
# kernel with its two-pass top_db clamp (an atomic maximum between the passes); the in-repo dialect on `auto` into an output api allocates
MFCC_CASES = [("sk2", 1, False, True), ("sk2", 2, False, True), ("sk2", 3, False, True), ("sk2", 2, True, True), ("sk2", 3, True, True),
              ("librosa", 4, False, True), ("inrepo", 0, False, False)]


@pytest.mark.parametrize("preset,variant,i16,own_out", MFCC_CASES)
def test_mfcc_run(cfg, preset, variant, i16, own_out):
    """MfccPlan.run on the ragged batch of the alignment tests (1 / 1 / 5 / 48 / 623 frames).  No route waits on the host: the chunk
    table of a (segments, variant) pair is uploaded once — by the baseline here — and device int16 input is widened slice by slice on
    the ctx stream."""
    s = _mfcc_setup(cfg, preset)
    flat = (s["flat"] * 20000).astype(np.int16) if i16 else s["flat"]
    plan, seg, fseg = s["plan"], s["seg"], s["fseg"]

    def call(d, o):
        return {"out": plan.run(d["x"], seg, fseg, out=o.get("out"), variant=variant)}
    what = "mfcc %s variant %d%s" % (preset, variant, " int16" if i16 else "")
    base = cfg.race(what, {"x": flat}, call, outs={"out": f32((fseg.total, plan.d_out))} if own_out else None)["out"]
    assert np.isfinite(base).all(), what
    if cfg.mode == "owned":
        GA._mfcc_oracle(s, flat, base, what)


# ======================================================================================================================= stand-alone operations
def test_enframe_cepstrum_spectrum_abs(cfg):
    """enframe and cepstrum stage their tables and wait for the copy before they queue the kernel (one host wait each)"""
    from oracle import ref_cpu as O
    api, ctx = cfg.api, cfg.ctx
    x = synth_audio(1, 1000, 16000)
    L, st = 400, 160
    w = np.ascontiguousarray(O.hamming_sym(L), dtype=np.float32)
    got = cfg.race("enframe", {"x": x}, lambda d, o: {"out": api.enframe(ctx, d["x"], L, st, w)}, waits=True)["out"]
    rng = np.random.default_rng(9)
    rows, nb, nfilt, nceps, eps = 50, 257, 40, 13, 1e-8
    Xs = np.abs(rng.standard_normal((rows, nb))).astype(np.float32)
    fb = np.ascontiguousarray(np.abs(rng.standard_normal((nfilt, nb))).astype(np.float32) * (rng.random((nfilt, nb)) < 0.1), dtype=np.float32)
    dct = np.ascontiguousarray(O.dct2_ortho_matrix(nfilt, nceps), dtype=np.float32)
    cep = cfg.race("cepstrum", {"X": Xs}, lambda d, o: {"out": api.cepstrum(ctx, d["X"], fb, dct, 1, 1, eps)}, waits=True)["out"]
    reim = rng.standard_normal((rows, 2 * nb)).astype(np.float32)
    mag = cfg.race("spectrum_abs", {"reim": reim}, lambda d, o: {"out": api.spectrum_abs(ctx, d["reim"], nb, 1.0 / 512, 1)})["out"]
    if cfg.mode == "owned":
        GA.assert_feat_close(got, O.enframe(x, L, st), "enframe")
        GA.assert_feat_close(cep, np.log10(Xs.astype(np.float64) @ fb.astype(np.float64).T + eps) @ dct.astype(np.float64).T, "cepstrum")
        GA.assert_feat_close(mag, np.hypot(reim[:, :nb].astype(np.float64), reim[:, nb:].astype(np.float64)) / 512, "spectrum_abs")


@pytest.mark.parametrize("dim", [13, 26])
def test_delta_and_cmvn(cfg, dim):
    """ragged, with a 1-frame utterance (tests/test_gpu_parity.py test_delta_cmvn_ragged_batches' bounds)"""
    from oracle import ref_cpu as O
    api, ctx = cfg.api, cfg.ctx
    lens = [70, 1, 3, 200]
    offs = np.concatenate(([0], np.cumsum(lens)))
    X = (np.random.default_rng(dim).standard_normal((sum(lens), dim)) * 3 + 1).astype(np.float32)
    seg = cfg.cached("dseg", lambda: api.Segments.from_lengths(ctx, lens))
    dl = cfg.race("delta %d" % dim, {"X": X}, lambda d, o: {"out": api.delta_features(ctx, d["X"], seg, 2)})["out"]
    cm = cfg.race("cmvn %d" % dim, {"X": X}, lambda d, o: {"out": api.cmvn_features(ctx, d["X"], seg)})["out"]
    if cfg.mode == "owned":
        def per_utt(fn):
            return np.vstack([fn(X[offs[u]:offs[u + 1]].astype(np.float64)) for u in range(len(lens))])
        ref = per_utt(lambda f: O.delta(f, 2))
        assert np.abs(dl - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
        assert np.abs(cm - per_utt(O.scale)).max() <= 1e-4


def test_plp_post(cfg):
    """the PLP back end on a ragged batch (98 / 1 / 3 / 30 frames); its tables are staged per call: one host wait before the kernels"""
    from oracle import ref_cpu as O
    api, ctx = cfg.api, cfg.ctx
    fs, lens = 16000, [98, 1, 3, 30]
    nb = O.plp_num_bands(fs)
    offs = np.concatenate(([0], np.cumsum(lens)))
    tcfg, w, fb, eye = O.sidekit_plp_tables(fs)
    logspec = GA.cached("plp logspec", lambda: np.vstack(
        [O.mfcc_pipeline(synth_audio(u, 400 + 160 * (T - 1), fs), tcfg, w, fb, eye) for u, T in enumerate(lens)]).astype(np.float32))
    seg = cfg.cached("pseg", lambda: api.Segments.from_lengths(ctx, lens))
    got = cfg.race("plp_post", {"x": logspec}, lambda d, o: {"out": api.plp_post(ctx, d["x"], seg, fs / 2.0)}, waits=True)["out"]
    assert np.isfinite(got).all()
    if cfg.mode == "owned":
        GA.assert_feat_close(got, np.vstack([O.plp_from_logspec(logspec[offs[u]:offs[u + 1]].astype(np.float64), fs) for u in range(len(lens))]), "plp_post")


# ======================================================================================================================= VAD
def _vad_segments(cfg, step):
    seg = cfg.cached("vadseg", lambda: cfg.api.Segments.from_lengths(cfg.ctx, GA.VAD_LENS))
    return seg, cfg.cached(("vadfseg", step), lambda: cfg.api.vad_frame_segments(cfg.ctx, seg, step))


@pytest.mark.parametrize("kind,normalize,step", [("i16", True, 128), ("f32", True, 128), ("unit", False, 128), ("i16", False, 256)])
def test_vad_features(cfg, kind, normalize, step):
    """with the normalised peak pre-pass (a memset and an atomic maximum in front of the feature kernel) and without; the call's chunk
    table is uploaded with one host wait before the kernels are queued"""
    api, ctx = cfg.api, cfg.ctx
    sigs = GA._vad_signals(kind)
    seg, fseg = _vad_segments(cfg, step)

    def call(d, o):
        z, pw, en, _ = api.vad_features(ctx, d["x"], seg, fseg, step=step, normalize=normalize)
        return {"zcr": z, "power": pw, "entropy": en}
    what = "vad features %s normalize %d step %d" % (kind, normalize, step)
    base = cfg.race(what, {"x": np.concatenate(sigs)}, call, waits=True)
    if cfg.mode == "owned":
        GA._vad_oracle_check(sigs, fseg, base, normalize, step, what)


@pytest.mark.parametrize("mode", [0, 1])
def test_vad_detect(cfg, mode):
    """both detectors on the planes of the int16 batch (the silent utterance's NaNs included): decisions equal to the restatement's"""
    api, ctx = cfg.api, cfg.ctx
    seg, fseg = _vad_segments(cfg, 128)

    def planes_of():
        z, pw, en, _ = api.vad_features(ctx, np.concatenate(GA._vad_signals("i16")), seg, fseg, step=128, normalize=True)
        return {"zcr": np.asarray(z), "power": np.asarray(pw), "entropy": np.asarray(en)}
    planes = cfg.cached("vadplanes", planes_of)
    plane = planes["power"] if mode == 0 else planes["entropy"]
    gate, lo, hi, min_len = 35.0, 0.3, 12.0, 16
    thr = lo if mode == 0 else 0.4

    def call(d, o):
        m, c = api.vad_detect(ctx, d["zcr"] if mode == 0 else None, d["plane"], fseg, mode=mode, zcr_gate=gate, ampl=thr, amph=hi, min_len=min_len)
        return {"mask": m, "count": c}
    inputs = {"zcr": planes["zcr"], "plane": plane} if mode == 0 else {"plane": plane}
    got = cfg.race("vad detect mode %d" % mode, inputs, call)
    o, marked = fseg.offsets, 0
    for u in range(fseg.n):
        zz, pp = planes["zcr"][o[u]:o[u + 1]], plane[o[u]:o[u + 1]]
        ref = VO.detect(zz, pp, gate, np.float32(lo), np.float32(hi), min_len) if mode == 0 else VO.detect_frequency(pp, np.float32(0.4))
        assert np.array_equal(got["mask"][o[u]:o[u + 1]], ref) and got["count"][u] == int(ref.sum()), (mode, u)
        marked += int(ref.sum())
    assert 0 < marked < fseg.total   # (a poisoned plane marks nothing in mode 0 and everything in mode 1: neither is the answer)


# ======================================================================================================================= GMM
GMM_U = 1100    # (precision 4 decides on the host from 1024 utterances on)


def _gmm_setup(cfg):
    """test_gmm_bf16x3_close_calls_are_rescored_in_fp32's models (K = 64, D = 39, 12 speakers, two of them identical and two 1e-6 apart:
    close calls that precision 1 / 3 / 4 score again) on 1100 utterances of 5 .. 59 frames"""
    def data():
        rng = np.random.default_rng(41)
        K, D, S = 64, 39, 12
        w = rng.dirichlet(5 * np.ones(K))
        mu = rng.standard_normal((K, D))
        cov = rng.uniform(0.5, 2.0, (K, D))
        mus = [mu] + [mu + 0.05 * rng.standard_normal((K, D)) for _ in range(S)]
        mus[5] = mus[4].copy()
        mus[9] = mus[8] + 1e-6 * rng.standard_normal((K, D))
        lens = rng.integers(5, 60, GMM_U)
        feats = [(mus[1 + u % S][rng.choice(K, size=n, p=w)] + np.sqrt(cov[rng.choice(K, size=n)]) * rng.standard_normal((n, D))).astype(np.float32)
                 for u, n in enumerate(lens)]
        return {"w": w, "mus": mus, "cov": cov, "lens": lens, "feats": feats, "X": np.vstack(feats), "S": S}
    g = GA.cached("stream order gmm", data)

    def make():
        M = g["S"] + 1
        return (cfg.api.GmmScorer(cfg.ctx, np.stack([g["w"]] * M), np.stack(g["mus"]), np.stack([g["cov"]] * M), has_ubm=True),
                cfg.api.Segments.from_lengths(cfg.ctx, g["lens"]))
    return (g,) + cfg.cached("gmm", make)


@pytest.mark.parametrize("loglik", [False, True])
@pytest.mark.parametrize("precision", [0, 1, 2, 3, 4])
def test_gmm_score(cfg, precision, loglik):
    """precisions 1 and 3 read the close-call count on the host mid-call and score those utterances again; 4 does the same on this batch
    (1100 utterances: it decides late, from the full lists).  With loglik the [models x frames] matrix is scored in one pass at the
    asked precision and nothing is scored twice: no host wait at any precision (4 then runs as 0)."""
    g, sc, seg = _gmm_setup(cfg)
    names = ("loglik", "scores", "argmax") if loglik else ("scores", "argmax")

    def call(d, o):
        r = sc.score(d["feats"], seg, loglik=loglik, precision=precision)
        return {n: r[n] for n in names}
    what = "gmm score precision %d loglik %d" % (precision, loglik)
    base = cfg.race(what, {"feats": g["X"]}, call, waits=precision in (1, 3, 4) and not loglik)
    if precision in (1, 3) and not loglik:
        assert 0 < sc.last_rescored < GMM_U, what
    if precision == 4 and not loglik:
        assert sc.last_auto["precision_used"] in (0, 1), what
    if cfg.mode == "owned":
        from oracle import ref_cpu as O
        some = list(range(0, GMM_U, 37))
        ref = np.array([[O.gmm_score(g["w"], m, g["cov"], g["feats"][u]) for m in g["mus"]] for u in some])
        assert (np.abs(base["scores"][some] - ref) <= 1e-4 * np.abs(ref)).all(), (what, np.abs(base["scores"][some] - ref).max())
        if loglik:
            F = int(seg.offsets[40])
            np.testing.assert_allclose(base["loglik"][3, :F], O.gmm_score_samples(g["w"], g["mus"][3], g["cov"], g["X"][:F]), rtol=1e-4, atol=1e-4)


def test_gmm_em_stats_and_batch(cfg):
    """device frames; the sums come back to host arrays (one host wait per call).  K = 16, D = 39, 500 frames; the batch form on three
    models over overlapping row ranges gives each model the single call's bits"""
    from oracle import ref_cpu as O
    api, ctx = cfg.api, cfg.ctx
    rng = np.random.default_rng(61)
    K, D, n = 16, 39, 500
    mu = rng.standard_normal((K, D)) * 1.5
    X = (mu[rng.integers(0, K, n)] + rng.standard_normal((n, D))).astype(np.float32)
    w, cov = rng.dirichlet(5 * np.ones(K)), rng.uniform(0.5, 2.0, (K, D))

    def one(d, o):
        st = api.gmm_em_stats(ctx, w, mu, cov, d["X"])
        return {"nk": st["nk"], "sx": st["sx"], "sxx": st["sxx"], "ll": np.array([st["loglik_sum"]])}
    got = cfg.race("em stats", {"X": X}, one, waits=True)
    off, cnt = np.array([0, 100, 37]), np.array([500, 400, 203])
    mus = np.stack([mu, mu + 0.1, mu - 0.1])

    def batch(d, o):
        st = api.gmm_em_stats_batch(ctx, np.stack([w] * 3), mus, np.stack([cov] * 3), d["X"], off, cnt)
        return {"nk": st["nk"], "sx": st["sx"], "sxx": st["sxx"], "ll": st["loglik_sum"]}
    gb = cfg.race("em stats batch", {"X": X}, batch, waits=True)
    assert all(np.array_equal(gb[k][0], got[k] if k != "ll" else got[k][0]) for k in got)
    if cfg.mode == "owned":
        for m in range(3):   # (tests/test_gpu_parity.py test_gmm_em_stats_shapes' rules)
            nk, sx, sxx, ll = O.gmm_em_stats(w, mus[m], cov, X[off[m]:off[m] + cnt[m]].astype(np.float64))
            assert abs(gb["ll"][m] - ll) <= 2e-5 * abs(ll)
            assert np.allclose(gb["nk"][m], nk, rtol=1e-4, atol=1e-4 * nk.max())
            assert np.allclose(gb["sx"][m], sx, rtol=1e-4, atol=1e-4 * np.abs(sx).max())
            assert np.allclose(gb["sxx"][m], sxx, rtol=1e-4, atol=1e-4 * np.abs(sxx).max())


# ======================================================================================================================= centroids, cosine
@pytest.mark.parametrize("N,d,S", [(600, 8, 3), (2049, 33, 5)])
def test_centroids(cfg, N, d, S):
    """the labels index the output: their poison is a wrong but in-range labelling (every label moved on by one)"""
    rng = np.random.default_rng(N + d)
    X = (rng.standard_normal((N, d)) * 2 + 0.5).astype(np.float32)
    lab = rng.integers(0, S, N).astype(np.int32)
    got = cfg.race("centroids %d x %d" % (N, d), {"X": X, "labels": lab}, lambda dv, o: {"out": cfg.api.centroids(cfg.ctx, dv["X"], dv["labels"], S)},
                   poison={"labels": ((lab + 1) % S).astype(np.int32)})["out"]
    if cfg.mode == "owned":
        for s in range(S):   # (test_centroids_shapes_and_order's bound)
            np.testing.assert_allclose(got[s], X[lab == s].astype(np.float64).mean(axis=0), rtol=0, atol=1e-6)


def _cosine_data(N, d, S):
    rng = np.random.default_rng(7 * d + S + N)
    Cn = rng.standard_normal((S, d)).astype(np.float32)
    return (Cn[rng.integers(0, S, N)] + 0.7 * rng.standard_normal((N, d))).astype(np.float32), Cn


# ((N, d, S), precision, dist, counts, waits): the split-precision sweeps re-score from a device-side list and return without a host wait
# unless the diagnostics are asked for (counts); auto runs as precision 0 on a small problem, and on the large one — the smallest at
# which cosine.hip prices a pilot: N >= 8192 and N d (7.8e-13 + 1.62e-14 S) >= 0.25e-3 — reads the pilot's counts on the host mid-call
SMALL, PILOT = (70, 128, 8), (16384, 256, 4000)
COS_CASES = [(SMALL, 0, True, False, False), (SMALL, 0, False, False, False), (SMALL, 1, False, False, False), (SMALL, 2, False, False, False),
             (SMALL, 1, False, True, True), (SMALL, "auto", True, False, False), (PILOT, "auto", False, False, True)]


@pytest.mark.parametrize("shape,precision,dist,counts,waits", COS_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_cosine_identify(cfg, shape, precision, dist, counts, waits):
    from oracle import ref_cpu as O
    N, d, S = shape
    X, Cn = GA.cached(("stream order cosine", shape), lambda: _cosine_data(N, d, S))
    names = ("dist", "argmin", "min") if dist else ("argmin", "min")

    def call(dv, o):
        r = cfg.api.cosine_identify(cfg.ctx, dv["X"], dv["C"], dist=dist, precision=precision, counts=counts)
        if shape == PILOT:
            assert r["auto"]["pilot_rows"] > 0, r["auto"]
        return {n: r[n] for n in names}
    what = "cosine %s precision %s dist %d counts %d" % (shape, precision, dist, counts)
    got = cfg.race(what, {"X": X, "C": Cn}, call, waits=waits)
    if cfg.mode == "owned":
        rows = slice(0, min(N, 256))   # (the oracle on the first rows: the large case's full matrix is 16384 x 4000 float64)
        ref = O.cosine_matrix(X[rows], Cn)
        assert np.array_equal(got["argmin"][rows], ref.argmin(1)), what
        if dist:   # (tests/test_gpu_parity.py test_cosine_odd_shapes_vs_oracle's bound)
            np.testing.assert_allclose(got["dist"][rows], ref, rtol=0, atol=3e-6)
        # include/ssp.h's proven bounds on the minimum at precisions 0 / 1 / 2 (auto: the loosest of the paths it may take)
        np.testing.assert_allclose(got["min"][rows], ref.min(1), rtol=0, atol={0: 3e-6, 1: 2e-4, 2: 4.1e-3, "auto": 4.1e-3}[precision])


def test_cosine_identify_plain_entry_point(cfg):
    """ssp_cosine_identify (no precision argument) through the C-ABI on outputs the caller owns, inside the ordering api gives every
    device-pointer call: the bits of ssp_cosine_identify2 at precision 0"""
    ctx, _lib = cfg.ctx, cfg._lib
    N, d, S = 70, 128, 8
    X, Cn = _cosine_data(N, d, S)

    def plain(dv, o):
        with ctx._ordered(_lib.DEVICE):
            _lib.check(ctx._lib.ssp_cosine_identify(ctx._h, p(dv["X"]), N, d, p(dv["C"]), S, p(o["dist"]), p(o["argmin"]), p(o["min"]), _lib.DEVICE, None))
        return dict(o)
    got = cfg.race("ssp_cosine_identify", {"X": X, "C": Cn}, plain, outs={"dist": f32((N, S)), "argmin": ((N,), "int32"), "min": f32((N,))})
    two = cfg.api.cosine_identify(ctx, X, Cn, dist=True, precision=0, counts=False)
    SO.same_bits(got, {k: np.asarray(two[k]) for k in got}, "ssp_cosine_identify against ssp_cosine_identify2")


# ======================================================================================================================= dense, packed network
@pytest.mark.parametrize("N,d_in,units", [(77, 1274, 256), (77, 50, 12)])
def test_dense_forward(cfg, N, d_in, units):
    """dense_kernel (d_in > 256) and the register GEMM of cosine.hip (d_in <= 256); X, the weights and the bias all arrive late"""
    from oracle import ref_cpu as O
    rng = np.random.default_rng(N + d_in)
    X = rng.standard_normal((N, d_in)).astype(np.float32)
    W = (rng.standard_normal((d_in, units)) / np.sqrt(d_in)).astype(np.float32)
    b = rng.standard_normal(units).astype(np.float32)
    got = cfg.race("dense %d -> %d" % (d_in, units), {"X": X, "Wt": np.ascontiguousarray(W.T), "bias": b},
                   lambda d, o: {"Y": cfg.api.dense_forward(cfg.ctx, d["X"], d["Wt"], d["bias"], relu=True)})["Y"]
    if cfg.mode == "owned":
        GA.assert_feat_close(got, O.dense_net_forward(X, [(W, b, "relu")]), "dense %d -> %d" % (d_in, units))


def _dnn_layers():
    rng = np.random.default_rng(88)
    dims, N = [40, 32, 16], 70
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               (0.2 * rng.standard_normal(dims[i + 1])).astype(np.float32), "relu" if i == 0 else "linear") for i in range(2)]
    return X, layers


def test_packed_network_forward(cfg):
    """DnnForward.forward, dims [40, 32, 16], N = 70 (dnn_chain.hip)"""
    from oracle import ref_cpu as O
    X, layers = _dnn_layers()
    net = cfg.cached("dnn", lambda: cfg.api.DnnForward(cfg.ctx, [(np.ascontiguousarray(W.T), b, act == "relu") for W, b, act in layers]))
    got = cfg.race("dnn forward", {"X": X}, lambda d, o: {"Y": net.forward(d["X"])})["Y"]
    if cfg.mode == "owned":
        GA.assert_feat_close(got, O.dense_net_forward(X, layers), "dnn forward")


# ======================================================================================================================= LSTM, GRU, conv, l2
def _lstm_case(H):
    def make():
        rng = np.random.default_rng(300 + H)
        D, lens = 13, [(1, 5, 98)[s % 3] for s in range(70)]
        W, U, b = LO.keras_init(rng, D, H, 1.5)
        return W, U, b, (3.0 * rng.standard_normal((sum(lens), D))).astype(np.float32), lens
    return GA.cached(("stream order lstm", H), make)


@pytest.mark.parametrize("H", [16, 128])
def test_lstm_forward_ragged(cfg, H):
    """LstmForward.forward on 70 sequences of 1 / 5 / 98 frames, D = 13"""
    W, U, b, X, lens = _lstm_case(H)
    net, seg = cfg.cached(("lstm", H), lambda: (cfg.api.LstmForward(cfg.ctx, W, U, b, "sigmoid"), cfg.api.Segments.from_lengths(cfg.ctx, lens)))
    got = cfg.race("lstm H %d" % H, {"feats": X}, lambda d, o: {"h": net.forward(d["feats"], seg)})["h"]
    if cfg.mode == "owned":
        GA.assert_feat_close(got, LO.forward_ragged(W, U, b, X, seg.offsets, "sigmoid"), "lstm H %d" % H)


@pytest.mark.parametrize("reset_after", [False, True])
def test_gru_forward(cfg, reset_after):
    """(T, d_in, H, N) = (5, 7, 48, 37): the sequence, its mean over time, and the sequence once more with the workspace capped at ten
    chunks, so that the call runs as four slabs through the same scratch"""
    T, d_in, H, N, act = 5, 7, 48, 37, "sigmoid"

    def data():
        rng = np.random.default_rng(500 + reset_after)
        return GO.gru_init(rng, d_in, H, reset_after, 1.5) + ((3 * rng.standard_normal((N, T, d_in))).astype(np.float32),)
    W, U, b, X = GA.cached(("stream order gru", reset_after), data)
    net = cfg.cached(("gru", reset_after), lambda: cfg.api.GruForward(cfg.ctx, W, U, b, act, reset_after))
    net.set_workspace(1 << 30)
    seq = cfg.race("gru sequence reset_after %d" % reset_after, {"X": X}, lambda d, o: {"seq": net.forward(d["X"])})["seq"]
    assert net.last_slab == N
    mean = cfg.race("gru mean reset_after %d" % reset_after, {"X": X}, lambda d, o: {"mean": net.forward(d["X"], mean=True)})["mean"]
    net.set_workspace(4 * (T * 3 * H + T * H + 2 * H) * 10)
    slabs = cfg.race("gru sequence in slabs reset_after %d" % reset_after, {"X": X}, lambda d, o: {"seq": net.forward(d["X"])})["seq"]
    assert 0 < net.last_slab < N, net.last_slab
    net.set_workspace(1 << 30)
    assert np.array_equal(slabs, seq)
    if cfg.mode == "owned":
        ref = GO.gru(W, U, b, X, act, reset_after)
        GA.assert_feat_close(seq, ref, "gru sequence")
        GA.assert_feat_close(mean, GO.time_mean(ref), "gru mean")


def test_conv2d_same_and_l2_normalize(cfg):
    """(5, 3) input, 3 x 3 kernel, 16 filters, stride 2 — input, kernel and bias all late; l2_normalize at d = 33 and 512 with a zero row"""
    api, ctx = cfg.api, cfg.ctx
    rng = np.random.default_rng(16)
    N, T, D, k, F = 3, 5, 3, 3, 16
    X = (3 * rng.standard_normal((N, T, D))).astype(np.float32)
    K = GO.glorot(rng, (k, k, 1, F), k * k, k * k * F)
    bc = (0.1 * rng.standard_normal(F)).astype(np.float32)
    got = cfg.race("conv2d_same", {"X": X, "K": K, "bias": bc}, lambda d, o: {"Y": api.conv2d_same(ctx, d["X"], d["K"], d["bias"], (2, 2))})["Y"]
    if cfg.mode == "owned":
        GA.assert_feat_close(got, GO.conv2d_same(X, K, bc, (2, 2)), "conv2d_same")
    for d in (33, 512):
        Z = (2 * np.random.default_rng(d).standard_normal((37, d))).astype(np.float32)
        Z[3] = 0
        y = cfg.race("l2_normalize d %d" % d, {"X": Z}, lambda dv, o: {"Y": api.l2_normalize(ctx, dv["X"])})["Y"]
        if cfg.mode == "owned":
            GA.assert_feat_close(y, GO.l2_normalize(Z.astype(np.float64)), "l2 d %d" % d)


# ======================================================================================================================= collectives
def test_allgather_and_allreduce_in_a_world_of_one(cfg):
    """Context.allgather / allreduce_sum_ through RCCL with one rank: both are the identity, queued on the ctx stream"""
    ctx = cfg.ctx
    x = np.arange(12 * 50, dtype=np.float32).reshape(12, 50) + 0.5
    ctx.comm_init(0, 1, cfg.api.Context.comm_unique_id())
    try:
        got = cfg.race("allgather", {"x": x}, lambda d, o: {"out": ctx.allgather(d["x"])})["out"]
        red = cfg.race(CANNOT_FAIL_WITHOUT_ORDERING[2], {"t": x.reshape(-1)}, lambda d, o: {"t": ctx.allreduce_sum_(d["t"])})["t"]
    finally:
        cfg.torch.cuda.synchronize()
        ctx.comm_destroy()
    assert np.array_equal(got, x) and np.array_equal(red, x.reshape(-1))


# ======================================================================================================================= the d_vector networks
# They take api.default_context(torch_stream=True) themselves — the context that borrowed torch's default stream — and are called here
# while S is current: with device tensors through the racing pattern, with numpy arrays (their own .cuda() in and .cpu() out on S) with
# the library's stream kept busy.

def test_dense_net_predict_under_another_stream(stale):
    from oracle import ref_cpu as O
    from speech_signal_processing_amd import d_vector
    X, layers = _dnn_layers()
    net = stale.cached("DenseNet", lambda: d_vector.DenseNet(layers))
    assert net._ctx is stale.ctx
    dev = stale.race("DenseNet.predict (tensor)", {"X": X}, lambda d, o: {"Y": net.predict(d["X"])})["Y"]
    base, got = stale.race_host("DenseNet.predict (numpy)", lambda: net.predict(X), [X.shape[0] * 16])
    assert np.array_equal(got, base) and np.array_equal(base, dev)
    GA.assert_feat_close(dev, O.dense_net_forward(X, layers), "DenseNet.predict")


def test_lstm_net_predict_and_ragged_under_another_stream(stale):
    from speech_signal_processing_amd import d_vector
    W, U, b, X, lens = _lstm_case(128)
    net = stale.cached("LstmNet", lambda: d_vector.LstmNet(W, U, b, recurrent_activation="sigmoid"))
    fseg = stale.cached("LstmNet fseg", lambda: stale.api.Segments.from_lengths(net._ctx, lens))
    N, T = 20, 9
    Xe = np.ascontiguousarray(X[:N * T].reshape(N, T, 13))
    # ((N, T, D) input: the call builds its segment table first — one upload and host wait on the library's stream)
    dev = stale.race("LstmNet.predict (tensor)", {"X": Xe}, lambda d, o: {"h": net.predict(d["X"])}, waits=True)["h"]
    rag = stale.race("LstmNet.predict_ragged (tensor)", {"X": X}, lambda d, o: {"h": net.predict_ragged(d["X"], fseg)})["h"]
    base, got = stale.race_host(CANNOT_FAIL_WITHOUT_ORDERING[0], lambda: net.predict(Xe), [])
    assert np.array_equal(got, base) and np.array_equal(base, dev)
    base, got = stale.race_host(CANNOT_FAIL_WITHOUT_ORDERING[1], lambda: net.predict_ragged(X, fseg), [])
    assert np.array_equal(got, base) and np.array_equal(base, rag)
    GA.assert_feat_close(dev, LO.forward_ragged(W, U, b, Xe.reshape(-1, 13), np.arange(N + 1) * T, "sigmoid"), "LstmNet.predict")
    GA.assert_feat_close(rag, LO.forward_ragged(W, U, b, X, fseg.offsets, "sigmoid"), "LstmNet.predict_ragged")


def test_conv_gru_net_predict_under_another_stream(stale):
    """the small network of tests/test_gru_gpu.py ((21, 14) input, 16 filters, 3 x GRU(48), E = 32) on 37 chunks, in one slab and with
    the workspace capped at ten chunks: conv, three GRU layers, dense and l2_normalize chained on the device, each slab copied into the
    result by torch on S"""
    from speech_signal_processing_amd import d_vector
    act, reset_after, N = "sigmoid", True, 37
    rng = np.random.default_rng(41)
    conv, grus, dense = GO.network_init(rng, 21, 14, 16, 48, 32, 3, reset_after, scale=2.0)
    X = (3 * rng.standard_normal((N, 21, 14))).astype(np.float32)
    net = stale.cached("ConvGruNet", lambda: d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after))
    _, per, _ = net._slab(21, 14)
    low = stale.cached("ConvGruNet low", lambda: d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after,
                                                                     workspace_bytes=per * 10))
    dev = stale.race("ConvGruNet.predict (tensor)", {"X": X}, lambda d, o: {"Y": net.predict(d["X"])})["Y"]
    slabs = stale.race("ConvGruNet.predict in slabs (tensor)", {"X": X}, lambda d, o: {"Y": low.predict(d["X"])})["Y"]
    assert low.last_slab == 10 and net.last_slab == N
    base, got = stale.race_host("ConvGruNet.predict (numpy)", lambda: net.predict(X), [N * 32])
    assert np.array_equal(got, base) and np.array_equal(base, dev) and np.array_equal(slabs, dev)
    base, got = stale.race_host("ConvGruNet.predict in slabs (numpy)", lambda: low.predict(X), [N * 32, 10 * 32])
    assert np.array_equal(got, base) and np.array_equal(base, dev)
    emb, _ = GO.network(conv, grus, dense, X, act, reset_after)
    GA.assert_feat_close(dev, emb, "ConvGruNet.predict")


def test_nn_model_eval_on_one_chunk_under_another_stream(stale):
    """nn_model.eval(chunk, spk_model=DenseNet): the decision rests on the embedding the network returns — an embedding read before the
    kernel wrote it is NaN, which the reference's scan never selects (the answer would be None)"""
    from speech_signal_processing_amd import d_vector
    X, layers = _dnn_layers()
    net = stale.cached("DenseNet", lambda: d_vector.DenseNet(layers))
    emb = net.predict(X[:3])
    m = d_vector.nn_model(store=None)
    m.d_vector = {"spk0": emb[0], "spk1": emb[1], "spk2": emb[2]}
    base, got = stale.race_host("nn_model.eval", lambda: m.eval(X[1], spk_model=net), [16])
    assert base == "spk1" and got == base
