"""GPU tests of the diarization block (run with -m gpu on an MI355X): ssp_pairwise_scores against the float64 restatement with its
contracts (symmetry, same bits every call, independence of the batch, the NaN-row rule, skewed device pointers), ssp_ahc_cluster EQUAL to
the float32 restatement on the matrix the device itself produced (LDS-resident and workspace-resident recordings in one ragged batch),
the end-to-end cases whose margin test_diarize_host.py asserts, the PLDA backend, Diarizer.run, and the error codes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diarize_oracle as DO      # noqa: E402
import plda_oracle as PO         # noqa: E402

pytestmark = pytest.mark.gpu

PAIR_COUNTS = (0, 1, 2, 31, 32, 33, 65, 100)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def env():
    import torch
    from speech_signal_processing_amd import api
    return torch, api, api.default_context(torch_stream=True)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# --------------------------------------------------------------------------------------------------------------------- pairwise
def _pair_case(q, form):
    def make():
        rng = np.random.RandomState(1000 + q)
        X = rng.randn(sum(PAIR_COUNTS), q).astype(np.float32)
        if form == "cosine":
            X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
            g = h = None
            c0 = 0.0
        else:
            psi = np.sort(rng.gamma(2.0, 2.0, q))[::-1]
            X = (X * np.sqrt(1.0 + psi)).astype(np.float32)
            g64, h64, c64 = DO.plda_coeffs(psi)
            g, h, c0 = g64.astype(np.float32), h64.astype(np.float32), float(np.float32(c64))
        ref = DO.pairwise(X, DO.offsets(PAIR_COUNTS), g, h, c0)
        return X, g, h, c0, ref
    return cached(("pair", q, form), make)


@pytest.mark.parametrize("form", ["cosine", "plda"])
@pytest.mark.parametrize("q", [1, 7, 64, 130, 512])
def test_pairwise_scores_ragged_batch(env, q, form):
    torch, api, ctx = env
    X, g, h, c0, ref = _pair_case(q, form)
    off, sq = DO.offsets(PAIR_COUNTS), DO.sq_offsets(PAIR_COUNTS)
    got_dev = api.pairwise_scores(ctx, dev(torch, X), PAIR_COUNTS, g, h, c0)
    got = got_dev.cpu().numpy()
    assert got.shape == (sq[-1],) and got.dtype == np.float32
    for r, (G, R) in enumerate(zip(DO.blocks(got, PAIR_COUNTS), DO.blocks(ref, PAIR_COUNTS))):
        if G.size == 0:
            continue
        err = float(np.abs(G - R).max())
        print("[measured] q=%d %s n=%d: max abs err %.3e, bound %.3e" % (q, form, G.shape[0], err, DO.parity_bound(R)))
        assert err <= DO.parity_bound(R), (q, form, r)
        assert np.array_equal(G, G.T), "block %d is not exactly symmetric" % r
    # the same call gives the same bits; the host route too
    assert np.array_equal(api.pairwise_scores(ctx, dev(torch, X), PAIR_COUNTS, g, h, c0).cpu().numpy(), got)
    assert np.array_equal(api.pairwise_scores(ctx, X, PAIR_COUNTS, g, h, c0), got)
    # a recording alone gives the bits it has in the batch
    for r in (3, 6, 7):
        alone = api.pairwise_scores(ctx, dev(torch, X[off[r]:off[r + 1]]), [PAIR_COUNTS[r]], g, h, c0).cpu().numpy()
        assert np.array_equal(alone, got[sq[r]:sq[r + 1]]), r
    # a leading pad: device pointers that are 4- but not 16-byte aligned, X and out
    pad = torch.empty(X.size + 1, dtype=torch.float32, device="cuda")
    pad[1:] = dev(torch, X).reshape(-1)
    out = torch.full((sq[-1] + 3,), float("nan"), device="cuda")
    api.pairwise_scores(ctx, pad[1:].view(X.shape), PAIR_COUNTS, g, h, c0, out=out[3:])
    assert np.array_equal(out[3:].cpu().numpy(), got) and bool(torch.isnan(out[:3]).all())


@pytest.mark.parametrize("form", ["cosine", "plda"])
def test_pairwise_scores_nan_row_rule(env, form):
    """a non-finite entry in row i: row i and column i of its block NaN, everything else as with that row zeroed"""
    torch, api, ctx = env
    X, g, h, c0, _ = _pair_case(130, form)
    off, sq = DO.offsets(PAIR_COUNTS), DO.sq_offsets(PAIR_COUNTS)
    bad, zero = X.copy(), X.copy()
    rows = {6: (off[6] + 40, np.nan), 7: (off[7] + 99, np.inf), 5: (off[5] + 0, -np.inf)}
    for r, (row, v) in rows.items():
        bad[row, 129 if r != 7 else 0] = v
        zero[row] = 0.0
    got = api.pairwise_scores(ctx, dev(torch, bad), PAIR_COUNTS, g, h, c0).cpu().numpy()
    want = api.pairwise_scores(ctx, dev(torch, zero), PAIR_COUNTS, g, h, c0).cpu().numpy()
    for r, (G, W) in enumerate(zip(DO.blocks(got, PAIR_COUNTS), DO.blocks(want, PAIR_COUNTS))):
        W = W.copy()
        if r in rows:
            i = rows[r][0] - off[r]
            W[i, :] = np.nan
            W[:, i] = np.nan
        assert np.array_equal(G, W, equal_nan=True), r


# -------------------------------------------------------------------------------------------------------------------------- AHC
def _ahc_batch(env):
    """the ragged batch: cosine scores the DEVICE produced, copied back (the restatement then clusters the very same float32 numbers)"""
    torch, api, ctx = env

    def make():
        X = np.concatenate([DO.cluster_case(n, 4, 32, 0.5, 100 + n)[0] for n in DO.AHC_COUNTS])
        S = api.pairwise_scores(ctx, dev(torch, X), DO.AHC_COUNTS)
        return S, S.cpu().numpy()
    return cached("ahc", make)


def _ahc_equal(got, want, what):
    got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items()}
    for k in ("labels", "n_clusters", "merge_pair"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    assert got["merge_score"].dtype == np.float32 and np.array_equal(got["merge_score"], want["merge_score"], equal_nan=True), what
    return got


@pytest.mark.parametrize("linkage", DO.LINKAGES)
def test_ahc_equals_the_float32_restatement(env, linkage):
    torch, api, ctx = env
    S_dev, S = _ahc_batch(env)
    got = api.ahc_cluster(ctx, S_dev, DO.AHC_COUNTS, linkage=linkage, threshold=0.5, merges=True)
    got = _ahc_equal(got, cached(("ahc-want", linkage), lambda: DO.ahc_batch(S, DO.AHC_COUNTS, linkage, 0.5)), linkage)
    # the host route, and without the merge outputs
    host = api.ahc_cluster(ctx, S, DO.AHC_COUNTS, linkage=linkage, threshold=0.5, merges=True)
    assert all(np.array_equal(host[k], got[k], equal_nan=(k == "merge_score")) for k in got)
    plain = api.ahc_cluster(ctx, S_dev, DO.AHC_COUNTS, linkage=linkage, threshold=0.5)
    assert set(plain) == {"labels", "n_clusters"} and np.array_equal(plain["labels"].cpu().numpy(), got["labels"])
    # a recording alone gives what it gives in the batch (LDS-resident and workspace-resident)
    off, sq = DO.offsets(DO.AHC_COUNTS), DO.sq_offsets(DO.AHC_COUNTS)
    for r in (3, 4, 5, 6):
        alone = api.ahc_cluster(ctx, S_dev[sq[r]:sq[r + 1]], [DO.AHC_COUNTS[r]], linkage=linkage, threshold=0.5, merges=True)
        for k in ("labels", "merge_pair", "merge_score"):
            assert np.array_equal(alone[k].cpu().numpy(), got[k][off[r]:off[r + 1]], equal_nan=True), (r, k)
        assert int(alone["n_clusters"][0]) == got["n_clusters"][r]


@pytest.mark.parametrize("linkage", DO.LINKAGES)
def test_ahc_stop_rules(env, linkage):
    torch, api, ctx = env
    S_dev, S = _ahc_batch(env)
    got = api.ahc_cluster(ctx, S_dev, DO.AHC_COUNTS, linkage=linkage, threshold=float("-inf"), min_clusters=3, merges=True)
    got = _ahc_equal(got, DO.ahc_batch(S, DO.AHC_COUNTS, linkage, -np.inf, 3), "min_clusters")
    assert got["n_clusters"].tolist() == [min(n, 3) for n in DO.AHC_COUNTS]
    ns = np.array([0, 5, 2, 0, 7, 1, 4], dtype=np.int32)       # 0: the threshold decides; 5 > n = 2: no merge
    got = api.ahc_cluster(ctx, S_dev, DO.AHC_COUNTS, linkage=linkage, threshold=0.5, n_speakers=ns, merges=True)
    got = _ahc_equal(got, DO.ahc_batch(S, DO.AHC_COUNTS, linkage, 0.5, 1, ns), "n_speakers")
    assert got["n_clusters"][[1, 2, 4, 5, 6]].tolist() == [2, 2, 7, 1, 4]


@pytest.mark.parametrize("linkage", DO.LINKAGES)
def test_ahc_tie_rule_on_quantised_scores(env, linkage):
    torch, api, ctx = env
    counts = (40, DO.N_LDS + 8)
    S = np.concatenate([DO.quantised_case(n, 7 + n).reshape(-1) for n in counts])
    for thr in (-np.inf, 0.25):
        got = api.ahc_cluster(ctx, dev(torch, S), counts, linkage=linkage, threshold=float(thr), merges=True)
        _ahc_equal(got, DO.ahc_batch(S, counts, linkage, thr), "quantised")


def test_ahc_one_nan_affects_its_recording_only(env):
    torch, api, ctx = env
    S_dev, S = _ahc_batch(env)
    sq, off = DO.sq_offsets(DO.AHC_COUNTS), DO.offsets(DO.AHC_COUNTS)
    bad = S.copy()
    bad[sq[3] + 7 * 65 + 30] = np.nan            # recording 3 (n = 65), entry [7][30]
    bad[sq[6] + 200 * 300 + 299] = np.inf        # recording 6 (n = 300, workspace-resident), entry [200][299]
    bad[sq[4] + 100 * DO.N_LDS + 5] = np.nan     # recording 4, entry [100][5]: below the diagonal, never read
    got = api.ahc_cluster(ctx, dev(torch, bad), DO.AHC_COUNTS, threshold=0.5, merges=True)
    got = _ahc_equal(got, DO.ahc_batch(bad, DO.AHC_COUNTS, "average", 0.5), "nan")
    clean = cached(("ahc-want", "average"), lambda: DO.ahc_batch(S, DO.AHC_COUNTS, "average", 0.5))
    for r in range(len(DO.AHC_COUNTS)):
        rows = slice(off[r], off[r + 1])
        if r in (3, 6):
            assert (got["labels"][rows] == -1).all() and got["n_clusters"][r] == -1
            assert (got["merge_pair"][rows] == -1).all() and np.isnan(got["merge_score"][rows]).all()
        else:
            assert np.array_equal(got["labels"][rows], clean["labels"][rows]) and np.array_equal(got["merge_pair"][rows], clean["merge_pair"][rows])


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("linkage", DO.LINKAGES)
def test_diarizer_recovers_the_true_partition(env, linkage):
    """cluster_case(n, 4, 32, 0.5, 100 + n) at threshold 0.5: test_diarize_host.py asserts the margin (accepted merges above 0.52, the
    first rejected below 0.48 in float64), 200 x the parity bound of the scores, so the device must find the case's own partition"""
    torch, api, ctx = env
    from speech_signal_processing_amd import diarize
    cases = [DO.cluster_case(n, 4, 32, 0.5, 100 + n) for n in DO.E2E_N]
    X = np.concatenate([c[0] for c in cases])
    d = diarize.Diarizer("cosine", linkage=linkage, threshold=0.5, ctx=ctx)
    for labels, cnt in (d.cluster(dev(torch, 3.0 * X), DO.E2E_N), d.cluster(3.0 * X, DO.E2E_N)):      # (unnormalised rows: the backend normalises)
        labels = labels.cpu().numpy() if hasattr(labels, "cpu") else labels
        cnt = cnt.cpu().numpy() if hasattr(cnt, "cpu") else cnt
        off = DO.offsets(DO.E2E_N)
        for r, (_, truth) in enumerate(cases):
            assert cnt[r] == 4 and DO.same_partition(labels[off[r]:off[r + 1]], truth), (linkage, DO.E2E_N[r])


def test_plda_backend_scores(env):
    """a small fitted model: the device's pair scores within the bound of plda_oracle's n = 1 log-likelihood ratio of the projected rows"""
    torch, api, ctx = env
    from speech_signal_processing_amd import diarize, plda
    rng = np.random.RandomState(5)
    q, S, per = 16, 12, 8
    spk = rng.randn(S, q) * 2.0
    X = (np.repeat(spk, per, axis=0) + rng.randn(S * per, q)).astype(np.float32)
    lab = np.repeat(np.arange(S), per)
    model = plda.Plda(n_iter=5, ctx=ctx).fit(X, lab)
    counts = (40, 0, 56)
    d = diarize.Diarizer(model, threshold=0.0, ctx=ctx)
    scores, seg = d.scores(X, counts)
    T = np.asarray(model.project(X), dtype=np.float64)
    off = DO.offsets(counts)
    for r, G in enumerate(DO.blocks(scores, counts)):
        if G.size == 0:
            continue
        t = T[off[r]:off[r + 1]]
        want = PO.llr_direct(model.psi_, t, np.ones(t.shape[0], dtype=np.int64), t)
        err = float(np.abs(G - want).max())
        print("[measured] plda backend n=%d: max abs err %.3e, bound %.3e" % (t.shape[0], err, DO.parity_bound(want)))
        assert err <= DO.parity_bound(want) and np.array_equal(G, G.T)
    labels, cnt = d.cluster(X, counts)
    want = DO.ahc_batch(scores, counts, "average", 0.0)
    assert np.array_equal(labels, want["labels"]) and np.array_equal(cnt[[0, 2]], want["n_clusters"][[0, 2]])


def test_diarizer_run(env):
    """two short synthetic signals and a deterministic embed: shapes, -1 off speech, labels equal to the pieces called by hand"""
    torch, api, ctx = env
    from speech_signal_processing_amd import VAD, diarize
    t = np.arange(4000)

    def tone(f, n):
        return 8000.0 * np.sin(2 * np.pi * f * t[:n] / 8000.0)
    sigs = [np.concatenate([np.zeros(2500), tone(200, 4000), np.zeros(3000), tone(900, 3500), np.zeros(2000)]).astype(np.int16),
            np.concatenate([np.zeros(1500), tone(900, 3000), np.zeros(3500), tone(200, 4000), np.zeros(1000)]).astype(np.int16)]

    def embed(chunks):
        """the share of sign changes among the samples that are not zero, and its complement: tones of different pitch point
        different ways, whatever silence a window takes in at the edge of a segment"""
        z = np.array([np.mean(np.diff(np.signbit(c[c != 0].astype(np.float64))) != 0) for c in chunks])
        return np.stack([z * 8.0, 1.0 - z * 8.0, np.full(len(chunks), 0.01)], axis=1).astype(np.float32)
    d = diarize.Diarizer("cosine", threshold=0.9, ctx=ctx)
    got = d.run(sigs, embed, win=800, hop=400, min_len=400)
    masks = VAD.detect_batch(sigs)
    wins = [diarize.windows(VAD.speech_segments(m, len(x)), 800, 400, 400) for m, x in zip(masks, sigs)]
    assert all(w.shape[0] >= 2 for w in wins)
    emb = embed([x[a:b] for x, w in zip(sigs, wins) for a, b in w])
    labels, cnt = d.cluster(emb, [w.shape[0] for w in wins])
    off = DO.offsets([w.shape[0] for w in wins])
    for i, (g, m, w) in enumerate(zip(got, masks, wins)):
        assert g.shape == (len(m),) and g.dtype == np.int32
        want = diarize.frame_labels(w, labels[off[i]:off[i + 1]], len(m), 128)
        assert np.array_equal(g, want)
        pos = np.arange(len(m)) * 128
        inside = ((pos[:, None] >= w[None, :, 0]) & (pos[:, None] < w[None, :, 1])).any(axis=1)
        assert (g[~inside] == -1).all() and (g[inside] >= 0).all() and (~inside).any() and inside.any()
        assert cnt[i] == 2 and set(g[inside].tolist()) == {0, 1}


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_error_codes_leave_the_context_usable(env):
    torch, api, ctx = env
    X = np.ones((4, 3), dtype=np.float32)
    S = np.zeros(16, dtype=np.float32)
    with pytest.raises(ValueError):
        api.pairwise_scores(ctx, np.ones((4, 0), dtype=np.float32), [4])                    # q < 1
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            api.pairwise_scores(ctx, X, [4], g=[1.0, bad, 1.0])
        with pytest.raises(ValueError):
            api.pairwise_scores(ctx, X, [4], h=[1.0, 1.0, bad])
    with pytest.raises(NotImplementedError):
        api.pairwise_scores(ctx, np.ones((2, 1025), dtype=np.float32), [2])                 # q > 1024
    with pytest.raises(NotImplementedError):
        api.pairwise_scores(ctx, np.ones((4097, 1), dtype=np.float32), [4097])              # n > 4096
    seg = api.Segments.from_lengths(ctx, [4])
    rc = ctx._lib.ssp_ahc_cluster
    from speech_signal_processing_amd import _lib
    lab, cnt = np.zeros(4, np.int32), np.zeros(1, np.int32)

    def ahc(linkage=0, thr=0.0, mc=1, ns=None):
        return rc(ctx._h, S.ctypes.data, seg._h, linkage, thr, mc, None if ns is None else ns.ctypes.data, lab.ctypes.data, cnt.ctypes.data,
                  None, None, _lib.HOST, None)
    assert ahc(linkage=3) == _lib.SSP_ERR_INVALID and ahc(linkage=-1) == _lib.SSP_ERR_INVALID
    assert ahc(thr=float("nan")) == _lib.SSP_ERR_INVALID
    assert ahc(mc=0) == _lib.SSP_ERR_INVALID
    assert ahc(ns=np.array([-1], dtype=np.int32)) == _lib.SSP_ERR_INVALID
    assert ahc(thr=float("inf")) == _lib.SSP_OK and cnt[0] == 4                            # +-inf are allowed
    assert ahc(thr=float("-inf")) == _lib.SSP_OK and cnt[0] == 1
    with pytest.raises(ValueError):
        api.ahc_cluster(ctx, S, [4], linkage="ward")
    big = api.Segments.from_lengths(ctx, [4097])
    assert rc(ctx._h, S.ctypes.data, big._h, 0, 0.0, 1, None, lab.ctypes.data, cnt.ctypes.data, None, None, _lib.HOST, None) == _lib.SSP_ERR_UNSUPPORTED
    # empty batches are no-ops
    assert api.pairwise_scores(ctx, np.zeros((0, 3), dtype=np.float32), []).shape == (0,)
    r = api.ahc_cluster(ctx, np.zeros(0, dtype=np.float32), [0, 0])
    assert r["labels"].shape == (0,) and r["n_clusters"].shape == (2,)
    # the context still works
    got = api.pairwise_scores(ctx, X, [4])
    assert np.array_equal(got, np.full(16, 3.0, dtype=np.float32))
    assert api.ahc_cluster(ctx, got, [4], threshold=0.0)["labels"].tolist() == [0, 0, 0, 0]
