"""Guards on the gfx950 ISA of the x-vector kernels (hipcc cross-compiles here, no GPU), in the pattern of tests/test_plda_isa.py:
xvector.hip is part of the build, no kernel uses scratch, the frame-layer kernel runs on the exact-fp32 MFMA and its registers and LDS
fit the two workgroups per CU its __launch_bounds__ plan."""
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
    """kernel name -> {"inst": instruction lines, "vgpr": vector + accumulator registers per lane, "scratch": bytes} of csrc/xvector.hip
    compiled to gfx950 assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    src = "xvector.hip"
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
    names = sorted(kernels)
    assert len(names) == 3 and [n for n in names if "tdnn_kernel" in n] and [n for n in names if "xv_pool_kernel" in n] and \
        [n for n in names if "xv_affine_kernel" in n], names     # the frame layer, the pooling, the segment layers' scale / offset
    for n in names:
        assert _count(kernels[n]["inst"], r"scratch_") == 0 and kernels[n]["scratch"] == 0, n


def test_frame_layer_runs_on_fp32_mfma_inside_its_occupancy(kernels):
    ks = [k for n, k in kernels.items() if "tdnn_kernel" in n]
    assert len(ks) == 1     # one instance: taps, dilation and the widths are run-time arguments
    k = ks[0]
    # a k-step of 32: 4 groups of 8, each 4 element pairs x (2 x 2) tiles of 32 x 32 per wave; the step is unrolled twice (two register sets)
    assert _count(k["inst"], r"v_mfma_f32_32x32x2_f32") >= 64, _count(k["inst"], r"v_mfma_f32_32x32x2_f32")
    assert _count(k["inst"], r"v_mfma_") == _count(k["inst"], r"v_mfma_f32_32x32x2_f32")    # no other (reduced-precision) MFMA
    assert k["vgpr"] <= 256, k["vgpr"]      # __launch_bounds__(256, 2): two workgroups of four waves per CU
    assert _count(k["inst"], r"buffer_load_dwordx4") >= 12     # the operand slabs come through the bounds-checked buffer resource
    assert _count(k["inst"], r"(global|buffer)_atomic") == 0


def test_pooling_accumulates_in_float64_without_atomics(kernels):
    k = [k for n, k in kernels.items() if "xv_pool_kernel" in n][0]
    assert _count(k["inst"], r"v_add_f64") >= 1 and _count(k["inst"], r"v_fma_f64|v_mul_f64") >= 1
    assert _count(k["inst"], r"(global|buffer|flat)_atomic") == 0
