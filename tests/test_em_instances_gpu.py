"""Every compiled kernel of the EM statistics (csrc/gmm_em.hip) against float64 on every route, under the one rule of tests/em_cases.py:
the single call on its default route and with SSP_EM_NO_FUSE / SSP_EM_NO_MFMA, the batched call over ranges of one buffer placed out of
order with gaps, the shared call with one parameter block; the width sweep, the hard kinds, and one model past the walker cap of every
path.  Beyond the rule: K <= 64 batched / shared = the single call's bits, K > 64 batched and single within the sum of their limits,
host = device features, a second call = the first, D = 64 works, D = 65 and batched D = 48 raise.
Run with -s for the `em_accuracy` lines (one per case and route, the largest ratios) that profiles/em_accuracy.md is written from.
Non-finite rows: tests/test_gmm_nonfinite_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_cases as E  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = E.case_ids()
REPORT = []          # (route, family, case, measure(...) results)
CALLS = [0]          # finite calls held to the rule


@pytest.fixture(scope="module")
def ssp():
    import torch
    from speech_signal_processing_amd import api
    return api, api.default_context(), torch.cuda.get_device_properties(0).multi_processor_count


def _same(a, b, m=None, mb=None):
    (ba, la), (bb, lb) = E.block_of(a, m), E.block_of(b, mb)
    return np.array_equal(ba, bb) and la == lb


def _hold(got, ev, L, what, bad, rows, m=None):
    """one result under the rule: measured, kept for the report, a miss collected (the test fails at its end with every miss)"""
    r = E.measure(got, ev, L, what, m)
    CALLS[0] += 1
    rows.append(r)
    if r["worst"] > 1.0:
        bad.append(r["message"])
    return r


def _report(route, c, rows, got_ref=()):
    worst = lambda k: max((r[k] or 0.0) for r in rows)  # noqa: E731
    REPORT.append((route, c["family"], c["name"], rows))
    print("em_accuracy %-30s %-16s calls %d  max %.3f  rms %.3f  loglik %.3f  mass %.3f  err/emu32 %.2f" % (
        c["name"], route, len(rows), worst("max_ratio"), worst("rms_ratio"), worst("ll_ratio"), worst("mass_ratio"), worst("max_vs_emu")))
    if c["family"].startswith("uncentred") and got_ref:
        rel = {"nk": 0.0, "sx": 0.0, "sxx": 0.0}
        lse = 0.0
        D = c["D"]
        for block, ll, ref in got_ref:
            own = ref["nk"] >= 1.0
            lse = max(lse, abs(ll - ref["ll"]) / ref["n"])
            if not own.any():
                continue
            r =np.abs(block - ref["block"])[own] / np.abs(ref["block"][own])
            rel["sx"], rel["sxx"], rel["nk"] = max(rel["sx"], r[:, :D].max()), max(rel["sxx"], r[:, D:2 * D].max()), max(rel["nk"], r[:, 2 * D].max())
            lse = max(lse, abs(ll - ref["ll"]) / ref["n"])
        print("em_uncentred %-30s %-16s rel err (mixtures with nk >= 1): nk %.2e  sx %.2e  sxx %.2e  |loglik_sum err| / n %.2e nat" % (
            c["name"], route, rel["nk"], rel["sx"], rel["sxx"], lse))


def _layout(rng, lens, gap=37):
    """rows of the models placed out of order, with gaps: (n_rows, row_off)"""
    off = np.zeros(len(lens), np.int64)
    pos = 11
    for m in rng.permutation(len(lens)):
        off[m] = pos
        pos += lens[m] + gap
    return pos + 5, off


def _buffer(c, seed=0):
    rng = np.random.default_rng(seed)
    n_rows, off = _layout(rng, c["lens"])
    X = (100.0 * rng.standard_normal((n_rows, c["D"]))).astype(np.float32)   # the gaps hold values that would show
    for m, f in enumerate(c["feats"]):
        X[off[m]:off[m] + len(f)] = f
    return X, off, np.array(c["lens"], np.int64)


@pytest.mark.parametrize("cid,spec", CASES, ids=[s[0] for s in CASES])
def test_single_call_every_route(ssp, cid, spec, monkeypatch):
    import torch
    api, ctx, num_cu = ssp
    c = E.build(spec)
    cap = E.walk_cap("single", c["K"], num_cu)
    bad = []
    for label, env in E.single_routes(c["K"], c["D"]):
        for name in ("SSP_EM_NO_FUSE", "SSP_EM_NO_MFMA"):
            monkeypatch.delenv(name, raising=False)
        for name in env:
            monkeypatch.setenv(name, "1")
        rows, got_ref = [], []
        for m in range(c["M"]):
            ev = E.ev_of(c, m)
            X = c["feats"][m]
            st = api.gmm_em_stats(ctx, c["w"][m], c["mus"][m], c["cov"][m], X)
            _hold(st, ev, E.acc_frames(len(X), cap), "%s single:%s model %d" % (cid, label, m), bad, rows)
            got_ref.append(E.block_of(st) + (ev["ref"],))
            assert _same(st, api.gmm_em_stats(ctx, c["w"][m], c["mus"][m], c["cov"][m], X)), (label, m, "a second call differs")
            assert _same(st, api.gmm_em_stats(ctx, c["w"][m], c["mus"][m], c["cov"][m], torch.from_numpy(X).cuda())), (label, m, "device features differ")
        _report("single:" + label, c, rows, got_ref)
    assert not bad, "\n".join(bad)


BATCHED = [s for s in CASES if (E.LATE_D if s[1][0] == "late" else s[1][-1]) <= E.MAX_D_MFMA]   # the batched entry points: D <= 47


@pytest.mark.parametrize("cid,spec", BATCHED, ids=[s[0] for s in BATCHED])
def test_batched_call(ssp, cid, spec):
    """every model its own parameters, the lengths of the case as ranges of one buffer out of order with gaps"""
    import torch
    api, ctx, num_cu = ssp
    c = E.build(spec)
    X, off, lens = _buffer(c)
    cap_b, cap_s = E.walk_cap("batch", c["K"], num_cu), E.walk_cap("single", c["K"], num_cu)
    st = api.gmm_em_stats_batch(ctx, c["w"], c["mus"], c["cov"], X, off, lens)
    bad, rows, got_ref = [], [], []
    for m in range(c["M"]):
        ev = E.ev_of(c, m)
        _hold(st, ev, E.acc_frames(lens[m], cap_b), "%s batch model %d" % (cid, m), bad, rows, m)
        got_ref.append(E.block_of(st, m) + (ev["ref"],))
        single = api.gmm_em_stats(ctx, c["w"][m], c["mus"][m], c["cov"][m], c["feats"][m])
        if c["K"] <= 64:
            assert _same(st, single, m), (m, "K <= 64: the batched call is not the single call's bits")
        else:
            E.agree(st, E.acc_frames(lens[m], cap_b), single, E.acc_frames(lens[m], cap_s), ev, "%s batch vs single, model %d" % (cid, m), m_a=m)
    _report("batch", c, rows, got_ref)
    for again in (api.gmm_em_stats_batch(ctx, c["w"], c["mus"], c["cov"], X, off, lens),
                  api.gmm_em_stats_batch(ctx, c["w"], c["mus"], c["cov"], torch.from_numpy(X).cuda(), off, lens)):
        assert all(_same(st, again, m, m) for m in range(c["M"]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cid,spec", BATCHED, ids=[s[0] for s in BATCHED])
def test_shared_call(ssp, cid, spec):
    """ONE parameter block (model 0's) over every range: the rule per range, the bits of the batched call with the block repeated, and
    for K <= 64 of the single call"""
    import torch
    api, ctx, num_cu = ssp
    c = E.build(spec)
    X, off, lens = _buffer(c, seed=1)
    cap_b = E.walk_cap("shared", c["K"], num_cu)
    st = api.gmm_em_stats_shared(ctx, c["w"][0], c["mus"][0], c["cov"][0], X, off, lens)
    bad, rows = [], []
    for m in range(c["M"]):
        _hold(st, E.ev_of(c, m, pm=0), E.acc_frames(lens[m], cap_b), "%s shared range %d" % (cid, m), bad, rows, m)
        if c["K"] <= 64:
            assert _same(st, api.gmm_em_stats(ctx, c["w"][0], c["mus"][0], c["cov"][0], c["feats"][m]), m), (m, "K <= 64: not the single call's bits")
    _report("shared", c, rows)
    rep = lambda a: np.repeat(a[:1], c["M"], axis=0)  # noqa: E731
    for again in (api.gmm_em_stats_batch(ctx, rep(c["w"]), rep(c["mus"]), rep(c["cov"]), X, off, lens),
                  api.gmm_em_stats_shared(ctx, c["w"][0], c["mus"][0], c["cov"][0], torch.from_numpy(X).cuda(), off, lens)):
        assert all(_same(st, again, m, m) for m in range(c["M"]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("entry,K,D", E.CAP_SHAPES, ids=["%s_K%d_D%d" % s for s in E.CAP_SHAPES])
def test_past_the_walker_cap(ssp, entry, K, D):
    """one model of 64 (cap + 3) + 17 frames: three walkers take a second tile — only then does the prefetch of tile + G read a tile —
    and the last tile is partial"""
    api, ctx, num_cu = ssp
    c = E.cap_case(entry, K, D, num_cu)
    ev = E.ev_of(c, 0)
    n = c["lens"][0]
    L = E.acc_frames(n, E.walk_cap(entry, K, num_cu))
    assert L == 128
    bad, rows = [], []
    if entry == "single":
        st = api.gmm_em_stats(ctx, c["w"][0], c["mus"][0], c["cov"][0], c["feats"][0])
        _hold(st, ev, L, c["name"], bad, rows)
    else:
        X = np.concatenate([np.full((11, D), 100.0, np.float32), c["feats"][0], np.full((7, D), 100.0, np.float32)])
        st = api.gmm_em_stats_batch(ctx, c["w"], c["mus"], c["cov"], X, [11], [n])
        _hold(st, ev, L, c["name"], bad, rows, 0)
        sh = api.gmm_em_stats_shared(ctx, c["w"][0], c["mus"][0], c["cov"][0], X, [11], [n])
        assert _same(st, sh, 0, 0)
    assert not rows[0]["rms_skipped"]
    _report(entry + ":cap", c, rows)
    assert not bad, "\n".join(bad)


def test_width_limits(ssp):
    """D = 64 is the widest single call (the sweep's last case runs it under the rule); D = 65, and D = 48 batched or shared, raise"""
    api, ctx, num_cu = ssp
    assert E.route_of("single", 128, 64) is not None and ("sweep_K128_D64", ("sweep", 128, 64)) in CASES
    one = lambda D: (np.ones(1), np.zeros((1, D)), np.ones((1, D)), np.zeros((10, D), np.float32))  # noqa: E731
    st = api.gmm_em_stats(ctx, *one(64))
    assert st["nk"][0] == 10.0 and np.isfinite(st["loglik_sum"])
    with pytest.raises(NotImplementedError):
        api.gmm_em_stats(ctx, *one(65))
    w, mu, cov, X = one(48)
    with pytest.raises(NotImplementedError):
        api.gmm_em_stats_batch(ctx, w[None], mu[None], cov[None], X, [0], [10])
    with pytest.raises(NotImplementedError):
        api.gmm_em_stats_shared(ctx, w, mu, cov, X, [0], [10])


def test_report():
    """the summary of the lines above, per route and case family (-s shows it); it holds nothing of its own"""
    table = {}
    for route, family, name, rows in REPORT:
        fam = "uncentred" if family.startswith("uncentred") else family
        t = table.setdefault((route, fam), dict(calls=0, max=0.0, rms=0.0, ll=0.0, mass=0.0, vs=0.0, at=""))
        t["calls"] += len(rows)
        for r in rows:
            if r["max_ratio"] > t["max"]:
                t["max"], t["at"] = r["max_ratio"], name
            t["rms"], t["ll"] = max(t["rms"], r["rms_ratio"] or 0.0), max(t["ll"], r["ll_ratio"])
            t["mass"], t["vs"] = max(t["mass"], r["mass_ratio"]), max(t["vs"], r["max_vs_emu"])
    for (route, fam), t in sorted(table.items()):
        print("em_summary %-16s %-14s calls %4d  max %.3f (%s)  rms %.3f  loglik %.3f  mass %.3f  err/emu32 %.2f" % (
            route, fam, t["calls"], t["max"], t["at"], t["rms"], t["ll"], t["mass"], t["vs"]))
    print("em_summary finite calls held to the rule: %d, largest ratio %.3f" % (
        CALLS[0], max([max(t["max"], t["rms"], t["ll"], t["mass"]) for t in table.values()] or [0.0])))
