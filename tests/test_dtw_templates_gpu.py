"""Batched DTW templates (ssp_dtw_templates / api.dtw_templates / MFCC_DTW.generate_templates) against the per-speaker loop
(MFCC_DTW.generate_template, one ssp_dtw_path call per pair) bit for bit, and against the oracle's generate_template."""
import os

import numpy as np
import pytest

from conftest import synth_audio

pytestmark = pytest.mark.gpu

LENGTHS = [(130, 1100, 700, 1), (65,), (64, 64, 17), (1, 1), (300, 257, 300, 2, 299)]
DIM13 = (40, 33, 47, 5)


@pytest.fixture(scope="module")
def cases():
    """the fixed groups, the loop's templates and the batched call's, each computed once and left unchanged"""
    from oracle import ref_cpu as O
    from speech_signal_processing_amd import MFCC_DTW
    rng = np.random.default_rng(2024)
    groups = [[rng.standard_normal(n).astype(np.float32).astype(np.float64) for n in lens] for lens in LENGTHS]
    groups.append([O.MFCC(synth_audio(u, n, 8000), 8000, 512, 256).flatten() for u, n in ((0, 5000), (1, 9000), (2, 7000), (3, 6500))])
    g13 = [rng.standard_normal((n, 13)).astype(np.float32).astype(np.float64) for n in DIM13]
    c = {"groups": groups, "g13": g13}
    c["loop"] = [MFCC_DTW.generate_template(g) for g in groups]
    c["loop13"] = MFCC_DTW.generate_template(g13)
    c["batched"] = MFCC_DTW.generate_templates(groups)
    c["batched13"] = MFCC_DTW.generate_templates([g13])
    for v in c["loop"] + c["batched"] + c["batched13"] + [c["loop13"]]:
        v.setflags(write=False)
    return c


def _same(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b)


def test_bit_equal_to_the_per_speaker_loop(cases):
    assert len(cases["batched"]) == 6
    for g, (got, ref) in enumerate(zip(cases["batched"], cases["loop"])):
        assert _same(got, ref), g
    assert len(cases["batched13"]) == 1 and _same(cases["batched13"][0], cases["loop13"])
    assert cases["batched13"][0].shape == (47, 13)


def test_oracle_parity(cases):
    from oracle import ref_cpu as O
    for g, (got, grp) in enumerate(zip(cases["batched"] + cases["batched13"], cases["groups"] + [cases["g13"]])):
        ref = O.generate_template(grp)
        longest = max(grp, key=lambda s: s.shape[0])   # (the first of the longest)
        assert got.shape == ref.shape == longest.shape, g
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-5), (g, float(np.abs(got - ref).max()))


def test_result_does_not_depend_on_the_workspace_cap(cases):
    from speech_signal_processing_amd import MFCC_DTW, api
    one = MFCC_DTW.generate_templates(cases["groups"], workspace_bytes=1)   # every pair its own chunk, the cap raised per pair
    largest = 0
    for g in cases["groups"]:
        lens = [s.shape[0] for s in g]
        m = int(np.argmax(lens))   # the template: the first of the longest
        largest = max([largest] + [api._dtw_direction_bytes(n, lens[m]) for k, n in enumerate(lens) if k != m])
    assert largest == 700 * 1100
    two = MFCC_DTW.generate_templates(cases["groups"], workspace_bytes=2 * largest)
    for g, ref in enumerate(cases["batched"]):
        assert _same(one[g], ref) and _same(two[g], ref), g
    assert _same(MFCC_DTW.generate_templates([cases["g13"]], workspace_bytes=1)[0], cases["loop13"])


def test_order_of_groups_does_not_matter(cases):
    from speech_signal_processing_amd import MFCC_DTW
    rev = MFCC_DTW.generate_templates(cases["groups"][::-1])
    assert len(rev) == 6
    for got, ref in zip(rev, cases["batched"][::-1]):
        assert _same(got, ref)


def test_raw_abi(cases):
    from speech_signal_processing_amd import _lib, api
    ctx = api.default_context()
    lib = ctx._lib
    groups = cases["groups"][:3]
    x = np.concatenate([s for g in groups for s in g])
    lens = [s.shape[0] for g in groups for s in g]
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    grp_off = np.array([0, 4, 5, 8], dtype=np.int64)

    def call(x, seq_off, grp_off, dim=1):
        out = np.full(1100 + 65 + 64, -7.0)
        toff = np.full(4, -1, dtype=np.int64)
        rc = lib.ssp_dtw_templates(ctx._h, x.ctypes.data, seq_off.ctypes.data, len(seq_off) - 1, grp_off.ctypes.data,
                                   len(grp_off) - 1, dim, 0, out.ctypes.data, toff.ctypes.data, None)
        return rc, out, toff

    rc, out, toff = call(x, seq_off, grp_off)
    assert rc == _lib.SSP_OK, lib.ssp_last_error()
    assert toff.tolist() == [0, 1100, 1165, 1229]
    for g in range(3):
        assert np.array_equal(out[toff[g]:toff[g + 1]], cases["batched"][g]), g
    bad = x.copy()
    bad[500] = np.nan
    assert call(bad, seq_off, grp_off)[0] == _lib.SSP_ERR_INVALID                                   # a NaN in x
    assert call(x, seq_off, np.array([0, 4, 4, 8], dtype=np.int64))[0] == _lib.SSP_ERR_INVALID      # an empty group
    assert call(x, seq_off, grp_off, dim=0)[0] == _lib.SSP_ERR_INVALID                              # dim = 0
    rc, out, toff = call(x, seq_off, grp_off)                                                       # the context is still usable
    assert rc == _lib.SSP_OK and np.array_equal(out[:1100], cases["batched"][0])


def test_load_train_builds_all_templates_in_one_call(tmp_path, monkeypatch):
    import wave
    from speech_signal_processing_amd import MFCC_DTW
    rng = np.random.default_rng(5)
    files = {}
    for spk in ("s1", "s2", "s3"):
        (tmp_path / spk).mkdir()
        for i in range(3):
            x = (4000 * rng.standard_normal(8000 + 512 * i + 100 * len(spk) + 700 * int(spk[1]))).astype("<i2")
            with wave.open(str(tmp_path / spk / ("%d.wav" % i)), "wb") as w:
                w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
                w.writeframes(x.tobytes())
            files[(spk, i)] = x[::2]
    calls = []
    real = MFCC_DTW.generate_templates
    monkeypatch.setattr(MFCC_DTW, "generate_templates", lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1])
    tpl, lab = MFCC_DTW.load_train(str(tmp_path))
    assert calls == [3]
    assert lab == os.listdir(tmp_path) and len(tpl) == 3
    order = [(spk, int(name[0])) for spk in lab for name in os.listdir(tmp_path / spk)]   # the order load_train reads the files in
    feats = dict(zip(order, MFCC_DTW._extract_all([files[k] for k in order], MFCC_DTW._MFCC)))
    for t, spk in zip(tpl, lab):
        seqs = [feats[k] for k in order if k[0] == spk]
        assert _same(t, MFCC_DTW.generate_template(seqs)), spk


# Templates wider than one super-block of the widest forward kernel (24 columns per lane x 64 lanes = 1536 columns): the boundary column is
# parked in global memory and read back by lane 0 of the next super-block.  3072 ends exactly on the second block's edge, 1700 leaves a
# ragged second block, 1536 fills exactly one block (nothing parked) and 1537 spills one column into a second.  All groups go in ONE call, so
# every round holds several such pairs and all but the first park their columns at a non-zero offset; samples shorter than 64 rows keep
# the wave from ever having all lanes busy.  The reference, ssp_dtw_path, sweeps 1024-column super-blocks of its own, independently.
WIDE = [(50, 1700, 900), (3072, 40, 700), (1536, 30, 500), (7, 1537)]


@pytest.fixture(scope="module")
def wide():
    from speech_signal_processing_amd import MFCC_DTW
    rng = np.random.default_rng(31)
    groups = [[rng.standard_normal(n).astype(np.float32).astype(np.float64) for n in lens] for lens in WIDE]
    g3 = [rng.standard_normal((n, 3)).astype(np.float32).astype(np.float64) for n in (20, 1600)]   # dim > 1 across a block edge
    return {"groups": groups, "loop": [MFCC_DTW.generate_template(g) for g in groups], "batched": MFCC_DTW.generate_templates(groups),
            "g3": g3, "loop3": MFCC_DTW.generate_template(g3)}


def test_templates_of_several_super_blocks(wide):
    from speech_signal_processing_amd import MFCC_DTW
    groups, loop, got, g3, loop3 = wide["groups"], wide["loop"], wide["batched"], wide["g3"], wide["loop3"]
    assert [t.shape for t in got] == [(1700,), (3072,), (1536,), (1537,)]
    for g, (a, b) in enumerate(zip(got, loop)):
        assert _same(a, b), (g, int((a != b).sum()))
    for cap in (1, 2 * 900 * 1700):   # alone (offset 0) and in other company: the same bits
        for g, (a, b) in enumerate(zip(MFCC_DTW.generate_templates(groups[::-1], workspace_bytes=cap)[::-1], loop)):
            assert _same(a, b), (cap, g)
    got3 = MFCC_DTW.generate_templates([g3, g3])
    assert got3[0].shape == (1600, 3) and _same(got3[0], loop3) and _same(got3[1], loop3)


def test_wide_templates_against_the_oracle(wide):
    from oracle import ref_cpu as O
    groups, got = wide["groups"], wide["batched"]
    for g in (0, 3):   # (the ragged second block and the one-column second block; the other two are held to the loop, bit for bit, above)
        ref = O.generate_template(groups[g])
        assert got[g].shape == ref.shape and np.allclose(got[g], ref, rtol=1e-5, atol=1e-5), g
