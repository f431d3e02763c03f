"""Guards on the gfx950 ISA of the i-vector kernels (hipcc cross-compiles here, no GPU): register counts that keep the planned occupancy,
no scratch, and the GEMMs on the exact-fp32 MFMA."""
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
    """kernel name -> {"inst": instruction lines, "vgpr": vector + accumulator registers per lane} of csrc/ivector.hip compiled to gfx950
    assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    src = "ivector.hip"
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
    return found


def _count(instrs, pattern):
    return sum(1 for t in instrs if re.match(pattern, t.split()[0]))


def test_no_kernel_spills(kernels):
    names = [n for n in kernels if "iv_" in n]
    assert len(names) == 6, names  # pack, two GEMM tile shapes, fold, Cholesky, accumulate
    for n in names:
        assert _count(kernels[n]["inst"], r"scratch_") == 0, n


def test_gemms_run_on_fp32_mfma_at_their_occupancy(kernels):
    big = [k for n, k in kernels.items() if "iv_gemm_kernelILi2ELi2E" in n]
    small = [k for n, k in kernels.items() if "iv_gemm_kernelILi1ELi1E" in n]
    assert len(big) == 1 and len(small) == 1
    for k in big + small:
        assert _count(k["inst"], r"v_mfma_f32_32x32x2_f32") >= 8
    assert big[0]["vgpr"] <= 256    # vector + accumulator registers: two workgroups of four waves per CU
    assert small[0]["vgpr"] <= 128  # four


def test_cholesky_kernel_registers(kernels):
    k = [v for n, v in kernels.items() if "iv_chol_kernel" in n]
    assert len(k) == 1
    assert k[0]["vgpr"] <= 128  # (its LDS, not its registers, sets the occupancy: nothing is gained below this)
