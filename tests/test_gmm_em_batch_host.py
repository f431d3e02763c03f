"""Host-side checks of batched EM training (no GPU): the golden fixture of tests/golden/make_golden_em_batch.py is pinned by the float64
oracle, the vectorised M step of gmm_train.fit_many is sklearn's M step bit for bit, and the batched kernels of gmm_em.hip keep the
instruction classes they were written for."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_signal_processing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _speakers(g, tag):
    return int(g[tag + "_cfg"][2])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_reproduces_batch_golden(golden, tag):
    """oracle.ref_cpu.gmm_fit per speaker from the stored inits = sklearn's fit stored in the fixture (1e-11)"""
    from oracle import ref_cpu as O
    g = golden("gmm_em_batch")
    K, D, S, max_iter, tol = g[tag + "_cfg"]
    niters = set()
    for s in range(_speakers(g, tag)):
        p = "%s%d_" % (tag, s)
        w, mu, cov, n_iter, lb, conv = O.gmm_fit(g[p + "X"], g[p + "w0"], g[p + "mu0"].astype(np.float64), g[p + "cov0"].astype(np.float64),
                                                 max_iter=int(max_iter), tol=float(tol))
        assert n_iter == int(g[p + "niter"]) and conv == bool(g[p + "conv"])
        assert abs(lb - float(g[p + "lb"])) <= 1e-11 * abs(float(g[p + "lb"]))
        for got, key in ((w, "w"), (mu, "mu"), (cov, "cov")):  # (1e-11 of each array's scale: covariances of nearly empty
            ref = g[p + key]                                     # components are differences of large sums)
            assert np.allclose(got, ref, rtol=1e-11, atol=1e-11 * np.abs(ref).max()), (p, key, np.abs(got - ref).max())
        niters.add(n_iter)
    if tag == "a":
        assert len(niters) >= 3, niters  # the speakers stop at different iterations: the batch's per-model convergence is exercised


def test_m_step_many_is_m_step():
    """the M step fit_many runs over all active models at once = GaussianMixture._m_step per model, bit for bit"""
    from speech_signal_processing_amd.gmm_train import GaussianMixture, _m_step_many
    rng = np.random.default_rng(5)
    for K in (1, 2, 5, 7, 8, 9, 16, 33, 64, 128, 512):
        B, D = 9, 13
        nk = rng.uniform(0, 500, (B, K)) ** rng.uniform(0.5, 2.0, (B, K))
        nk[:, 0] = 0.0
        sx = 50 * rng.standard_normal((B, K, D))
        sxx = rng.uniform(1, 1e4, (B, K, D))
        n = rng.integers(1, 100000, B)
        w, mu, cv = _m_step_many(nk, sx, sxx, n.astype(np.float64), 1e-6)
        gm = GaussianMixture(n_components=K)
        for b in range(B):
            w1, mu1, cv1 = gm._m_step({"nk": nk[b], "sx": sx[b], "sxx": sxx[b]}, int(n[b]))
            assert np.array_equal(w1, w[b]) and np.array_equal(mu1, mu[b]) and np.array_equal(cv1, cv[b]), (K, b)


def _isa(src, tmp_path):
    """kernel name -> instruction lines, compiled with the shipped per-source flags (the helper shape of test_isa_guards._isa)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / (src + ".s"))
    from speech_signal_processing_amd.build import SOURCE_FLAGS
    extra = tuple(SOURCE_FLAGS.get(src, []))
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-munsafe-fp-atomics", "-Wno-pass-failed", *extra,
                        "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in open(out):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = m.group(1)
            kernels[cur] = []
            continue
        t = line.strip()
        if cur is None or not t or t.startswith((";", ".")):
            continue
        if t.split()[0] == "s_endpgm":
            cur = None
            continue
        kernels[cur].append(t)
    return kernels


def test_batched_em_kernels_isa(tmp_path):
    """the batched EM kernels (segmented accumulation, all 6 instances, and the K > 64 log-sum-exp): matrix-core GEMMs, no scratch, and
    no loop test on lane masks (their persistent tile walk reads its bounds through readfirstlane: a walk rebuilt over lane masks is
    round 4's hang, test_isa_guards.test_persistent_loops_stay_wave_uniform)"""
    k = _isa("gmm_em.hip", tmp_path)
    seg = {n: v for n, v in k.items() if "gmm_em_acc_mfma_seg_kernel" in n or "gmm_em_lse_mfma_seg_kernel" in n}
    assert len(seg) == 7, sorted(seg)
    for n, v in seg.items():
        assert any(t.startswith("v_mfma_f32_32x32x2_f32") for t in v), n
        assert not any(t.startswith("scratch_") for t in v), n
        assert not any(re.match(r"s_andn2_b64 exec, exec", t) for t in v), n
