"""GPU tests of the VAD threshold sweep (run with -m gpu on an MI355X): ssp_vad_sweep's integer counts against the reference's own
(tests/golden/vad_sweep.npz), against the detector kernel on the same device arrays, and against the float64 restatement
tests/vad_oracle.py; the search surface of the VAD module on top of it.  Every count is compared with ==.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skewed  # noqa: E402
import stream_order as SO  # noqa: E402
import vad_oracle as VO  # noqa: E402

pytestmark = pytest.mark.gpu

LIMIT = 131072   # frames per utterance (include/ssp.h)


@pytest.fixture(scope="module")
def env():
    import torch
    from speech_signal_processing_amd import VAD, api, _lib
    return torch, VAD, api, _lib, api.default_context()


def counts_of(mask, lab):
    m, y = np.asarray(mask).reshape(-1) != 0, np.asarray(lab).reshape(-1) != 0
    return [int((m & y).sum()), int((m & ~y).sum()), int((~m & y).sum())]


def oracle(z, p, lab, gates, ampls, amphs, min_len=16, mode=0):
    """(n_par, 3) of one utterance by the restatement, on the float32 numbers the device compares"""
    z, p = np.asarray(z, dtype=np.float32), np.asarray(p, dtype=np.float32)
    if mode == 1:
        return np.array([counts_of(VO.detect_frequency(p, np.float32(t)), lab) for t in ampls], dtype=np.int32).reshape(-1, 3)
    return np.array([counts_of(VO.detect(z, p, np.float32(g), np.float32(lo), np.float32(hi), min_len), lab)
                     for g, lo, hi in zip(gates, ampls, amphs)], dtype=np.int32).reshape(-1, 3)


def _planes(g, c):
    return tuple(g[k + c][:, 0].astype(np.float32) for k in ("zcr_", "power_", "entropy_")) + (g["ylab_" + c],)


# ---- 1. the reference's counts ---------------------------------------------------------------------------------------------------
def test_fixture_one_case_at_a_time(env, golden):
    _, VAD, api, _, ctx = env
    g = golden("vad_sweep")
    for c in (str(c) for c in g["cases"]):
        z, p, e, lab = _planes(g, c)
        seg = api.Segments.from_lengths(ctx, [z.shape[0]])
        got = api.vad_sweep(ctx, z, p, lab, seg, g["gates"], g["ampls"], g["amphs"])
        assert got.dtype == np.int32 and got.shape == (125, 1, 3)
        assert np.array_equal(got[:, 0, :], g["counts_" + c]), c
        got = api.vad_sweep(ctx, None, e, lab, seg, None, g["ethr"], None, mode=1)
        assert np.array_equal(got[:, 0, :], g["ecounts_" + c]), c
        f1, counts = VAD.sweep(g["zcr_" + c], g["power_" + c], lab, g["gates"], g["ampls"], g["amphs"])
        assert np.array_equal(counts, g["counts_" + c]) and f1.dtype == np.float64 and np.abs(f1 - g["f1_" + c]).max() <= 1e-15, c


def test_fixture_as_one_ragged_batch(env, golden):
    torch, _, api, _, ctx = env
    g = golden("vad_sweep")
    names = [str(c) for c in g["cases"]]
    pl = [_planes(g, c) for c in names]
    z, p, e, lab = (np.concatenate([q[k] for q in pl]) for k in range(4))
    seg = api.Segments.from_lengths(ctx, [q[0].shape[0] for q in pl])
    for dev in (False, True):
        arrs = [torch.from_numpy(v).cuda() for v in (z, p, e, lab)] if dev else [z, p, e, lab]
        got = api.vad_sweep(ctx, arrs[0], arrs[1], arrs[3], seg, g["gates"], g["ampls"], g["amphs"])
        got1 = api.vad_sweep(ctx, None, arrs[2], arrs[3], seg, None, g["ethr"], None, mode=1)
        if dev:
            assert got.is_cuda and got.dtype == torch.int32
            got, got1 = got.cpu().numpy(), got1.cpu().numpy()
        for u, c in enumerate(names):
            assert np.array_equal(got[:, u, :], g["counts_" + c]), (c, dev)
            assert np.array_equal(got1[:, u, :], g["ecounts_" + c]), (c, dev)


# ---- 2. the sweep against the detector kernel ------------------------------------------------------------------------------------
_RANDOM = {}


def random_batch(env):
    """40 ragged utterances' planes on the device, labels (any nonzero value = speech) and 130 triples, some outside optimize's box, one
    with NaNs; made once"""
    torch, _, api, _, ctx = env
    if not _RANDOM:
        sigs = VO.random_batch(21, 40)
        seg = api.Segments.from_lengths(ctx, [s.shape[0] for s in sigs])
        zcr, power, _, fseg = api.vad_features(ctx, torch.from_numpy(np.concatenate(sigs)).cuda(), seg)
        rng = np.random.default_rng(22)
        lab = (rng.random(fseg.total) < 0.45) * rng.integers(1, 256, fseg.total)
        o = fseg.offsets
        for u in range(0, fseg.n, 2):   # every other utterance: labels that follow the power, so that tp is not small
            lab[o[u]:o[u + 1]] = power[o[u]:o[u + 1]].cpu().numpy() > 1.0
        gates = np.concatenate([rng.uniform(20, 40, 120), rng.uniform(0, 80, 9), [np.nan]]).astype(np.float32)
        ampls = np.concatenate([rng.uniform(0.3, 4, 120), rng.uniform(0, 20, 9), [np.nan]]).astype(np.float32)
        amphs = np.concatenate([rng.uniform(5, 15, 120), rng.uniform(0, 20, 9), [8.0]]).astype(np.float32)
        _RANDOM.update(zcr=zcr, power=power, fseg=fseg, lab=lab.astype(np.uint8), gates=gates, ampls=ampls, amphs=amphs)
        _RANDOM["counts"] = api.vad_sweep(ctx, zcr, power, torch.from_numpy(_RANDOM["lab"]).cuda(), fseg, gates, ampls, amphs).cpu().numpy()
    return _RANDOM


def test_sweep_equals_detector_and_restatement(env):
    _, _, api, _, ctx = env
    r = random_batch(env)
    fseg, o, lab = r["fseg"], r["fseg"].offsets, r["lab"]
    z, p = r["zcr"].cpu().numpy(), r["power"].cpu().numpy()
    assert r["counts"].shape == (130, 40, 3) and (r["ampls"][120:129] >= r["amphs"][120:129]).any()
    for j, (g, lo, hi) in enumerate(zip(r["gates"], r["ampls"], r["amphs"])):
        mask, _ = api.vad_detect(ctx, r["zcr"], r["power"], fseg, 0, float(g), float(lo), float(hi), 16)
        mask = mask.cpu().numpy()
        want = np.array([counts_of(mask[o[u]:o[u + 1]], lab[o[u]:o[u + 1]]) for u in range(fseg.n)])
        assert np.array_equal(r["counts"][j], want), (j, g, lo, hi)
    for u in range(fseg.n):
        want = oracle(z[o[u]:o[u + 1]], p[o[u]:o[u + 1]], lab[o[u]:o[u + 1]], r["gates"], r["ampls"], r["amphs"])
        assert np.array_equal(r["counts"][:, u, :], want), u
    assert len({tuple(c) for c in r["counts"].sum(axis=1).tolist()}) > 10 and r["counts"][:, :, 0].sum() > 1000   # (the batch decides something)


# ---- 3. edges --------------------------------------------------------------------------------------------------------------------
def edge_pool():
    """(zcr, power, labels) of hand-made utterances: T = 1, 3, 63, 64, 65, 128, 129 and the state machine's corners at min_len 16"""
    rng = np.random.default_rng(31)
    pool = []

    def add(power, zcr=None):
        power = np.asarray(power, dtype=np.float32)
        zcr = np.zeros_like(power) if zcr is None else np.asarray(zcr, dtype=np.float32)
        pool.append((zcr, power, (rng.random(power.shape[0]) < 0.5).astype(np.uint8)))
    for T in (1, 3, 63, 64, 65, 128, 129):
        p = np.full(T, 0.01)
        p[:min(T, 20)] = 20.0            # a loud run from frame 0 (open to the end for T <= 20)
        if T > 40:
            p[T - 18:] = 20.0            # a run open at the last frame
        add(p)
    add([0.01] * 5 + [20.0] * 16 + [0.01] * 5 + [20.0] * 17 + [0.01] * 30)                   # runs of exactly min_len (stays open) and min_len + 1
    add([0.5] * 30 + [20.0] * 17 + [0.5] * 82)                                               # the walks reach frame 0 and T: everything marked
    add([0.5] * 64 + [20.0] * 64 + [0.7] + [20.0] * 63)                                      # word-aligned runs, the flush on a word border
    add([np.nan] * 70)                                                                       # all-NaN power
    add([0.01] * 3 + [6.0] * 20 + [0.2] * 4 + [0.01] * 40 + [20.0] * 41 + [0.01] * 21,       # active through zcr only, behind the first run
        [0.0] * 23 + [30.0] * 4 + [0.0] * 102)
    return pool


EDGE_TRIPLES = np.array([(35, 0.3, 12), (35, 0.3, 5), (20.5, 0.1, 0.6), (39.5, 4.0, 5.0), (25, 12, 12), (25, 15, 5), (35, 25, 19),   # ampl >= amph
                         (np.nan, 0.3, 12), (35, np.nan, 12), (35, 0.3, np.nan), (0, 0, 0), (35, 0.6, 0.65), (29.5, 0.45, 19.5)], dtype=np.float32)
_EDGE = {}


def edge_oracle(k, min_len):
    if (k, min_len) not in _EDGE:
        z, p, lab = _EDGE.setdefault("pool", edge_pool())[k]
        _EDGE[(k, min_len)] = oracle(z, p, lab, *EDGE_TRIPLES.T, min_len=min_len)
    return _EDGE[(k, min_len)]


@pytest.mark.parametrize("min_len", [1, 16, 40])
def test_edges_whole_pool(env, min_len):
    _, _, api, _, ctx = env
    pool = _EDGE.setdefault("pool", edge_pool())
    z, p, lab = (np.concatenate([q[k] for q in pool]) for k in range(3))
    seg = api.Segments.from_lengths(ctx, [q[0].shape[0] for q in pool])
    got = api.vad_sweep(ctx, z, p, lab, seg, *EDGE_TRIPLES.T, min_len=min_len)
    for u in range(len(pool)):
        assert np.array_equal(got[:, u, :], edge_oracle(u, min_len)), (u, min_len)
    if min_len == 16:   # hand-written, at (35, 0.3, 12): everything marked where both walks run out; nothing where the power is NaN;
        # the run of exactly min_len frames (5..20) stays open and the next one (26..42) closes it as one segment
        assert got[0, 8, :].tolist() == counts_of(np.ones(129), pool[8][2]) and got[:, 10, 0].sum() == 0 and got[:, 10, 1].sum() == 0
        mark = np.zeros(73)
        mark[5:43] = 1
        assert got[0, 7, :].tolist() == counts_of(mark, pool[7][2])
    assert (got[:, :, 0] + got[:, :, 1]).max() > 0


@pytest.mark.parametrize("n_utt", [1, 5])
@pytest.mark.parametrize("n_par", [1, 63, 64, 65, 257])
def test_edges_counts_of_triples_and_utterances(env, n_par, n_utt):
    torch, _, api, _, ctx = env
    pool = _EDGE.setdefault("pool", edge_pool())
    first = (n_par + 3 * n_utt) % len(pool)
    pick = [(first + 5 * k) % len(pool) for k in range(n_utt)]
    idx = (np.arange(n_par) * 7 + n_par) % len(EDGE_TRIPLES)
    tri = EDGE_TRIPLES[idx]
    z, p, lab = (torch.from_numpy(np.concatenate([pool[u][k] for u in pick])).cuda() for k in range(3))
    seg = api.Segments.from_lengths(ctx, [pool[u][0].shape[0] for u in pick])
    got = api.vad_sweep(ctx, z, p, lab, seg, *tri.T).cpu().numpy()
    assert got.shape == (n_par, n_utt, 3)
    for k, u in enumerate(pick):
        assert np.array_equal(got[:, k, :], edge_oracle(u, 16)[idx]), (n_par, n_utt, u)


# ---- 4. order --------------------------------------------------------------------------------------------------------------------
def test_permuted_and_duplicated_triples(env):
    torch, _, api, _, ctx = env
    r = random_batch(env)
    lab = torch.from_numpy(r["lab"]).cuda()
    perm = np.random.default_rng(41).permutation(130)
    got = api.vad_sweep(ctx, r["zcr"], r["power"], lab, r["fseg"], r["gates"][perm], r["ampls"][perm], r["amphs"][perm]).cpu().numpy()
    assert np.array_equal(got, r["counts"][perm])
    dup = np.repeat(np.arange(0, 130, 3), 3)[:-1]   # every third triple three times over (the last twice): equal neighbours in a workgroup
    got = api.vad_sweep(ctx, r["zcr"], r["power"], lab, r["fseg"], r["gates"][dup], r["ampls"][dup], r["amphs"][dup]).cpu().numpy()
    assert np.array_equal(got, r["counts"][dup])
    same_amph = api.vad_sweep(ctx, r["zcr"], r["power"], lab, r["fseg"], r["gates"][:9], r["ampls"][:9], 8.4).cpu().numpy()   # scalars broadcast
    want = api.vad_sweep(ctx, r["zcr"], r["power"], lab, r["fseg"], r["gates"][:9], r["ampls"][:9], np.full(9, 8.4)).cpu().numpy()
    assert same_amph.shape == (9, 40, 3) and np.array_equal(same_amph, want)


# ---- 5. lengths ------------------------------------------------------------------------------------------------------------------
def long_planes(n, seed):
    rng = np.random.default_rng(seed)
    power = np.full(n, 0.01, dtype=np.float32)
    at = 0
    while at < n - 200:
        at += int(rng.integers(1, 120))
        m = int(rng.integers(1, 60))
        power[at:at + m] = 20.0
        power[at + m:at + m + int(rng.integers(0, 6))] = 0.5
        at += m
    zcr = np.where(rng.random(n) < 0.05, 40.0, 0.0).astype(np.float32)
    lab = (np.convolve(power > 1.0, np.ones(9), mode="same") > 0).astype(np.uint8)
    return zcr, power, lab


@pytest.mark.parametrize("n,n_par", [(16385, 8), (40321, 3), (LIMIT, 2)])   # four, two and one wave per workgroup
def test_long_utterances(env, n, n_par):
    _, _, api, _, ctx = env
    z, p, lab = long_planes(n, 51)
    tri = np.array([(35, 0.3, 12), (30, 0.6, 12), (45, 0.3, 25), (35, 0.3, 0.4), (35, 25, 12), (20, 0.4, 19), (35, 0.3, 12), (np.nan, 0.45, 5)],
                   dtype=np.float32)[:n_par]
    lens = [n, 0, 500] if n < LIMIT else [n]
    seg = api.Segments.from_lengths(ctx, lens)
    zz, pp, ll = (np.concatenate([v, v[:sum(lens) - n]]) for v in (z, p, lab))
    got = api.vad_sweep(ctx, zz, pp, ll, seg, *tri.T)
    want = oracle(z, p, lab, *tri.T)
    assert np.array_equal(got[:, 0, :], want) and want[0, 0] > 100
    if len(lens) == 3:
        assert not got[:, 1, :].any() and np.array_equal(got[:, 2, :], oracle(z[:500], p[:500], lab[:500], *tri.T))
    got = api.vad_sweep(ctx, None, pp, ll, seg, None, [0.4, 15.0], None, mode=1)
    assert np.array_equal(got[:, 0, :], oracle(None, p, lab, None, [0.4, 15.0], None, mode=1))


def test_over_the_length_limit(env):
    _, _, api, _, ctx = env
    n = LIMIT + 1
    z = np.zeros(n + 5, dtype=np.float32)
    for mode in (0, 1):
        with pytest.raises(NotImplementedError) as ei:
            api.vad_sweep(ctx, z, z, z.astype(np.uint8), api.Segments.from_lengths(ctx, [5, n]), 35.0, 0.3, 12.0, mode=mode)
        assert str(LIMIT) in str(ei.value)
    with pytest.raises(ValueError):
        api.vad_sweep(ctx, z[:8], z[:8], z[:8], api.Segments.from_lengths(ctx, [8]), 35.0, 0.3, 12.0, min_len=0)
    with pytest.raises(ValueError):
        api.vad_sweep(ctx, z[:8], z[:8], z[:8], api.Segments.from_lengths(ctx, [8]), 35.0, np.zeros(0), 12.0)   # n_par 0
    assert api.vad_sweep(ctx, z[:0], z[:0], z[:0], api.Segments.from_lengths(ctx, []), 35.0, 0.3, 12.0).shape == (1, 0, 3)


# ---- 6. pointers and streams -----------------------------------------------------------------------------------------------------
SKEWS = [{"zcr": 4, "power": 12, "lab": 1, "counts": 4}, {"zcr": 8, "power": 4, "lab": 3, "counts": 12}, {"lab": 7, "counts": 8}]


@pytest.mark.parametrize("skews", SKEWS, ids=["-".join("%s%d" % kv for kv in s.items()) for s in SKEWS])
@pytest.mark.parametrize("mode", [0, 1])
def test_skewed_device_arrays(env, mode, skews):
    torch, _, api, _lib, ctx = env
    r = random_batch(env)
    fseg = r["fseg"]
    z, p = r["zcr"].cpu().numpy(), r["power"].cpu().numpy()
    gates, ampls, amphs = (np.ascontiguousarray(r[k][:37]) for k in ("gates", "ampls", "amphs"))
    want = r["counts"][:37] if mode == 0 else np.asarray(api.vad_sweep(ctx, None, p, r["lab"], fseg, None, ampls, None, mode=1))
    zv, zt = skewed.view(z.shape[0], "float32", skews.get("zcr", 0), fill=z)
    pv, pt = skewed.view(p.shape[0], "float32", skews.get("power", 0), fill=p)
    lv, lt = skewed.view(r["lab"].shape[0], "uint8", skews.get("lab", 0), fill=r["lab"])
    cv, ct = skewed.view(37 * fseg.n * 3, "int32", skews.get("counts", 0))
    torch.cuda.synchronize()
    with ctx._ordered(_lib.DEVICE):
        _lib.check(ctx._lib.ssp_vad_sweep(ctx._h, zv.data_ptr() if mode == 0 else None, pv.data_ptr(), lv.data_ptr(), fseg._h, mode, 37,
                                          gates.ctypes.data if mode == 0 else None, ampls.ctypes.data, amphs.ctypes.data if mode == 0 else None, 16,
                                          cv.data_ptr(), _lib.DEVICE, None))
    torch.cuda.synchronize()
    assert np.array_equal(cv.cpu().numpy().reshape(37, fseg.n, 3), want)
    for tok, what in ((zt, "zcr"), (pt, "power"), (lt, "labels"), (ct, "counts")):
        skewed.check_guards(tok, "vad sweep mode %d %s" % (mode, what))


@pytest.mark.parametrize("mode", SO.MODES)
def test_behind_pending_work_on_a_side_stream(env, mode):
    """the planes and labels arrive on a side stream while the call is made (tests/stream_order.py); the call waits on the host once,
    for the upload of its thresholds, so the producer may have finished when it returns"""
    _, _, api, _, _ = env
    r = random_batch(env)
    cfg = SO.Config(mode)
    try:
        fseg = api.Segments(cfg.ctx, r["fseg"].offsets)
        gates, ampls, amphs = r["gates"][:33], r["ampls"][:33], r["amphs"][:33]

        def call(d, o):
            return {"counts": api.vad_sweep(cfg.ctx, d["zcr"], d["power"], d["lab"], fseg, gates, ampls, amphs)}
        base = cfg.race("vad sweep", {"zcr": r["zcr"].cpu().numpy(), "power": r["power"].cpu().numpy(), "lab": r["lab"]}, call, waits=True)
        assert np.array_equal(base["counts"], r["counts"][:33])
        del fseg
    finally:
        cfg.close()


def test_host_and_device_arrays_give_equal_counts(env):
    torch, _, api, _, ctx = env
    r = random_batch(env)
    host = api.vad_sweep(ctx, r["zcr"].cpu().numpy(), r["power"].cpu().numpy(), r["lab"], r["fseg"], r["gates"], r["ampls"], r["amphs"])
    assert isinstance(host, np.ndarray) and np.array_equal(host, r["counts"])
    wide = api.vad_sweep(ctx, r["zcr"].cpu().numpy(), r["power"].cpu().numpy(), r["lab"].astype(np.int64) * 1000, r["fseg"], r["gates"], r["ampls"], r["amphs"])
    assert np.array_equal(wide, r["counts"])   # labels of any type: nonzero = speech
    counts, ms = api.vad_sweep(ctx, r["zcr"], r["power"], torch.from_numpy(r["lab"]).cuda(), r["fseg"], r["gates"], r["ampls"], r["amphs"], timing=True)
    assert np.array_equal(counts.cpu().numpy(), r["counts"]) and ms > 0


# ---- 7. the search surface -------------------------------------------------------------------------------------------------------
def test_optimize_on_a_graded_case(env, golden):
    _, VAD, _, _, _ = env
    g = golden("vad_sweep")
    x, ylab = g["x_h"], g["ylab_h"]
    X = VAD.enframe(x / np.max(np.abs(x.astype(np.float64))))
    zcr, power, _ = VAD.feature(X)
    coarse = VAD.optimize(X, ylab, refine=0)
    assert VAD.optimize.last["evaluations"] == 4096
    res = VAD.VAD_detection(zcr, power, **coarse)             # the coarse grid's own best, through the detector
    tp, fp, fn = counts_of(res, ylab)
    coarse_f1 = VAD.f1_counts(tp, fp, fn)
    assert coarse_f1 == VAD.optimize.last["target"] and VAD.optimize.last["counts"].tolist() == [tp, fp, fn]
    best = VAD.optimize(X, ylab)
    last = VAD.optimize.last
    assert sorted(best) == ["amph", "ampl", "zcr_gate"] and last["params"] == best and last["evaluations"] == 3 * 4096
    for k, (lo, hi) in VAD.BOUNDS.items():
        assert np.float32(lo) <= best[k] <= np.float32(hi), (k, best[k])
    f1, counts = VAD.sweep(zcr, power, ylab, best["zcr_gate"], best["ampl"], best["amph"])
    assert f1.shape == (1,) and f1[0] == last["target"] and counts[0].tolist() == last["counts"].tolist()
    assert last["target"] >= coarse_f1   # (the fixture's 125 triples are not points of the 16 x 16 x 16 grid: their best is printed only)
    print("[measured] optimize on case h: coarse F1 %.4f, refined %.4f at %r; best of the fixture's 125 triples %.4f" % (
        coarse_f1, last["target"], best, g["f1_h"].max()))


def test_optimize_batch_pools_the_counts(env, golden, capsys):
    _, VAD, _, _, _ = env
    g = golden("vad_sweep")
    names = ["h", "i", "c", "g"]
    sigs, labs = [g["x_" + c] for c in names], [g["y_" + c] for c in names]
    best = VAD.optimize_batch(sigs, labs, grid=(6, 5, 4), refine=1)
    last = VAD.optimize_batch.last
    assert capsys.readouterr().out == "" and last["evaluations"] == 240 and last["params"] == best
    total = np.zeros(3, dtype=np.int64)
    for (zcr, power, _), c in zip(VAD.feature_batch(sigs), names):
        ylab = VAD.label_frames(g["y_" + c])
        assert np.array_equal(ylab, g["ylab_" + c])
        _, counts = VAD.sweep(zcr, power, ylab, best["zcr_gate"], best["ampl"], best["amph"])
        total += counts[0]
    assert last["counts"].tolist() == total.tolist()
    assert last["target"] == VAD.f1_counts(*total) and last["target"] > 0
