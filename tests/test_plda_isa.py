"""Guards on the gfx950 ISA of the PLDA kernels (hipcc cross-compiles here, no GPU), in the pattern of tests/test_ivector_isa.py: no
scratch, both instances of the scoring kernel on the exact-fp32 MFMA, and the scoring kernel's registers inside the occupancy its
__launch_bounds__ plans."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_signal_processing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel name -> {"inst": instruction lines, "vgpr": vector + accumulator registers per lane} of csrc/plda.hip compiled to gfx950
    assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    src = "plda.hip"
    assert src in SOURCES, "%s is not part of the library build" % src
    out = str(tmp_path_factory.mktemp("isa") / (src + ".s"))
    r = subprocess.run([HIPCC, *FLAGS, *SOURCE_FLAGS.get(src, []), "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    found, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = m.group(1)
            found[cur] = {"inst": []}
            continue
        t = line.strip()
        if cur is None or not t or t.startswith((";", ".")):
            continue
        if t.split()[0] == "s_endpgm":
            cur = None
            continue
        found[cur]["inst"].append(t)
    for name, k in found.items():
        m = re.search(r"\.amdhsa_kernel %s\b(.*?)\.end_amdhsa_kernel" % re.escape(name), text, flags=re.S)
        assert m, name
        k["vgpr"] = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(1)).group(1))
        k["scratch"] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)).group(1))
    return found


def _count(instrs, pattern):
    return sum(1 for t in instrs if re.match(pattern, t.split()[0]))


def test_no_kernel_uses_scratch(kernels):
    names = [n for n in kernels if "plda_" in n]
    assert len(names) == 13, names  # label check, class sums, centring, scatter GEMM, accumulate, 2 x 4 scoring instances
    for n in names:
        assert _count(kernels[n]["inst"], r"scratch_") == 0 and kernels[n]["scratch"] == 0, n


def test_scoring_instances_run_on_fp32_mfma_inside_their_occupancy(kernels):
    for shared in ("Lb1E", "Lb0E"):
        inst = {nq: [k for n, k in kernels.items() if "plda_score_kernelILi%dE%s" % (nq, shared) in n] for nq in (8, 16, 24, 32)}
        for nq, ks in inst.items():
            assert len(ks) == 1, (shared, nq)
            assert _count(ks[0]["inst"], r"v_mfma_f32_32x32x2_f32") >= 4 * nq, (shared, nq)   # 4 per k-step of 8, each k half once at least
            assert ks[0]["vgpr"] <= 256, (shared, nq, ks[0]["vgpr"])  # __launch_bounds__(256, 2): two workgroups of four waves per CU
