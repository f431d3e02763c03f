"""The EM instance suite's own footing, on the CPU (tests/em_cases.py): the yardstick leaves a different legitimate float32 evaluation
room (emu32_alt at or below half of every limit on every case), the cases are what their builders say, the rule has teeth (six mutations
of emu32, each of which compare must refuse — one of them invisible to the older `1e-4 * max` rule), and the calls of the GPU file reach
every kernel csrc/gmm_em.hip compiles."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_cases as E  # noqa: E402

SPECS = E.all_specs()


def _L(c, m, entry=None):
    entry = entry or c.get("entry", "single")
    return E.acc_frames(c["lens"][m], E.walk_cap(entry, c["K"], c.get("num_cu", E.NUM_CU_DEFAULT)))


@pytest.mark.parametrize("cid,spec", SPECS, ids=[s[0] for s in SPECS])
def test_yardstick_leaves_room_and_cases_are_as_built(cid, spec):
    """emu32_alt <= 0.5 of every limit on every model of every case; the construction conditions of the hard kinds; one lost frame
    falls outside the loglik limit"""
    c = E.build(spec)
    assert c["name"] == cid
    for m in range(c["M"]):
        ev = E.ev_of(c, m)
        r = E.yardstick_ratios(c, m, c.get("entry", "single"), c.get("num_cu", E.NUM_CU_DEFAULT))
        assert r["worst"] <= 0.5, (cid, m, r["max_ratio"], r["rms_ratio"], r["ll_ratio"], r["mass_ratio"])
        assert r["rms_skipped"] == (int((ev["ref"]["nk"] >= 8).sum()) < 4)
        # a lost frame moves loglik_sum by its own lse: outside the limit for (nearly) every frame
        assert (np.abs(ev["ref"]["lse"]) > r["limits"]["ll"]).mean() >= 0.9, (cid, m)
    assert E.lone_frames_are_typical(c)
    if c["family"] == "cap":
        assert not E.yardstick_ratios(c, 0, c["entry"], c["num_cu"])["rms_skipped"]   # the rms rule is claimed for the long cases
        cap = E.walk_cap(c["entry"], c["K"], c["num_cu"])
        n_tiles = -(-c["lens"][0] // 64)
        assert n_tiles == cap + 4 and c["lens"][0] % 64 == 17 and _L(c, 0) == 128
    if c["family"].startswith("uncentred"):
        assert E.overlap_share(c) >= 0.05
        assert np.abs(np.abs(c["mus"]).mean(axis=(0, 1)) - c["ratio"]).max() < 1.0   # ONE offset, in every column
    if c["family"] == "identical":
        for m in range(c["M"]):
            nk = E.ev_of(c, m)["ref"]["nk"]
            assert np.abs(nk - c["lens"][m] / c["K"]).max() <= 1e-12 * c["lens"][m]
    if c["family"] == "late_dominant":
        assert E.late_gap(c) > 300.0
    if c["family"] == "skewed_w":
        assert (c["w"] > 0).all() and c["w"].min() < 1e-30


def _mutant(c, m, **kw):
    return E.emu32(c["w"][m], c["mus"][m], c["cov"][m], c["feats"][m], **kw)


def test_emu32_itself_passes():
    """the unmutated yardstick is inside its own rule (ratio 1 / 8 at most on the max rule)"""
    c = E.sweep_case(5, 33)
    for m in range(c["M"]):
        r = E.compare(E.ev_of(c, m)["emu"], E.ev_of(c, m), _L(c, m))
        assert r["max_ratio"] <= 0.125 + 1e-12


def test_mutation_last_frame_of_a_partial_tile_dropped():
    c = E.sweep_case(5, 33)
    for m in (3, 5):   # 65 and 209 frames: the last tile holds 1 and 17
        n = c["lens"][m]
        ev = E.ev_of(c, m)
        with pytest.raises(AssertionError):
            E.compare(_mutant(c, m, keep=np.arange(n - 1)), ev, _L(c, m))
        assert abs(ev["ref"]["lse"][n - 1]) > E.limits(ev, _L(c, m))["ll"]   # the loglik limit alone sees it


def test_mutation_second_tile_of_walker_0_dropped():
    c = E.cap_case("single", 5, 7)
    cap = E.walk_cap("single", 5)
    n = c["lens"][0]
    keep = np.concatenate([np.arange(0, 64 * cap), np.arange(64 * cap + 64, n)])   # tile `cap` is walker 0's second
    with pytest.raises(AssertionError):
        E.compare(_mutant(c, 0, keep=keep), E.ev_of(c, 0), _L(c, 0))
    E.compare(_mutant(c, 0, keep=np.arange(n)), E.ev_of(c, 0), _L(c, 0))


def test_mutation_padded_constant_zero():
    c = E.sweep_case(5, 2)
    for m in range(c["M"]):
        with pytest.raises(AssertionError):
            E.compare(_mutant(c, m, pad_const=0.0), E.ev_of(c, m), _L(c, m))


def test_mutation_small_mixture_mean_moved_and_the_old_rule_is_blind_to_it():
    """one mean entry of the least populated mixture with nk >= 1 moved by 0.05 sigma: the old `1e-4 * max` rule accepts, compare refuses"""
    c = E.small_mixture_case()
    ev = E.ev_of(c, 0)
    nk = ev["ref"]["nk"]
    k = int(np.where(nk >= 1.0, nk, np.inf).argmin())
    assert 1.0 <= nk[k] < 8.0 and nk.max() > 500.0
    mus = c["mus"].copy()
    mus[0, k, 0] += 0.05 * np.sqrt(c["cov"][0, k, 0])
    bad = E.emu32(c["w"][0], mus[0], c["cov"][0], c["feats"][0])
    assert E.old_rule_accepts(bad, ev)
    assert E.old_rule_accepts(ev["emu"], ev)
    with pytest.raises(AssertionError):
        E.compare(bad, ev, _L(c, 0))
    E.compare(ev["emu"], ev, _L(c, 0))


def test_mutation_halves_normalised_separately():
    c = E.sweep_case(64, 15)
    for m in range(c["M"]):
        with pytest.raises(AssertionError):
            E.compare(_mutant(c, m, sep_halves=True), E.ev_of(c, m), _L(c, m))


def test_mutation_x2_from_the_neighbouring_column():
    c = E.sweep_case(33, 7)
    for m in range(c["M"]):
        with pytest.raises(AssertionError):
            E.compare(_mutant(c, m, x2_shift=True), E.ev_of(c, m), _L(c, m))


def test_route_coverage():
    """the calls of the GPU file over its case list reach every entry of INSTANCES, and every single-call K > 64 and batched K > 64
    instance at NCT = 1 and 2 (the ones no older test runs) by name"""
    reached = set()
    for cid, spec in SPECS:
        kind = spec[0]
        K, D = (spec[2], spec[3]) if kind in ("hard", "cap") else ((70, E.LATE_D) if kind == "late" else (spec[1], spec[2]))
        fake = dict(family="cap" if kind == "cap" else "x", K=K, D=D, entry=spec[1] if kind == "cap" else None)
        for entry, label, env in E.calls_of(fake):
            route = E.route_of(entry, K, D, env)
            assert route is not None, (cid, entry, label)
            assert all(i in E.INSTANCES for i in route)
            reached.update(route)
    assert reached == set(E.INSTANCES), set(E.INSTANCES) - reached
    assert E.route_of("single", 65, 64) is not None and E.route_of("single", 5, 65) is None
    assert E.route_of("batch", 5, 48) is None and E.route_of("shared", 5, 48) is None


def test_walk_cap_restates_the_dispatch():
    assert E.walk_cap("single", 512, 256) == 512 and E.walk_cap("batch", 64, 256) == 512
    assert E.walk_cap("batch", 512, 256) == 64 and E.walk_cap("shared", 70, 256) == 256 and E.walk_cap("batch", 100000, 4) == 1
    assert E.acc_frames(1, 512) == 64 and E.acc_frames(64 * 512, 512) == 64 and E.acc_frames(64 * 512 + 1, 512) == 128


def test_fuzz_tool_restates_the_rule():
    """tools/fuzz_scoring.py carries the rule as a function of its own (it imports nothing from tests/): the same worst ratio as
    measure(), on a result inside the rule (emu32_alt) and on one outside it (a dropped frame), at both walker caps"""
    import re
    src = open(os.path.join(E.ROOT, "tools", "fuzz_scoring.py")).read()
    assert "em_cases" not in src.replace("tests/em_cases.py", "")
    m = re.search(r"# ---- em_rule begin\n(.*?)# ---- em_rule end", src, re.S)
    assert m
    ns = {"np": np, "O": E.O}
    exec(m.group(1), ns)
    for c, mm in ((E.sweep_case(5, 33), 5), (E.sweep_case(70, 15), 4), (E.cap_case("batch", 70, 15), 0)):
        ev, n = E.ev_of(c, mm), c["lens"][mm]
        args = (c["w"][mm], c["mus"][mm], c["cov"][mm], c["feats"][mm])
        for got in (E.alt_of(c, mm), E.emu32(*args, keep=np.arange(n - 1))):
            D = c["D"]
            b, ll = E.block_of(got)
            for cap in (E.walk_cap("single", c["K"]), E.walk_cap("batch", c["K"])):
                want = E.measure(got, ev, E.acc_frames(n, cap))["worst"]
                have = ns["em_rule"](*args, b[:, 2 * D], b[:, :D], b[:, D:2 * D], ll, cap)
                assert abs(have - want) <= 1e-9 * want, (c["name"], have, want)
