"""Guards on the gfx950 ISA of the sliding-normalisation kernels (hipcc cross-compiles here, no GPU), in the pattern of
tests/test_snorm_isa.py: csrc/featnorm.hip is part of the library build, no kernel of the unit has a private segment, and every kernel's
registers per lane fit the occupancy its __launch_bounds__ states.  Nothing else is inspected."""
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
    """kernel name -> {"vgpr": vector + accumulator registers per lane, "scratch": private segment bytes, "spill": scratch instructions}
    of csrc/featnorm.hip compiled to gfx950 assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    src = "featnorm.hip"
    assert src in SOURCES, "%s is not part of the library build" % src
    out = str(tmp_path_factory.mktemp("isa") / (src + ".s"))
    r = subprocess.run([HIPCC, *FLAGS, *SOURCE_FLAGS.get(src, []), "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        name, desc = m.group(1), m.group(2)
        body = re.search(r"^%s:(.*?)^\s*s_endpgm" % re.escape(name), text, flags=re.S | re.M)
        assert body, name
        found[name] = {"vgpr": int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)),
                       "scratch": int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)),
                       "spill": len(re.findall(r"^\s*scratch_", body.group(1), flags=re.M))}
    return found


def test_every_instance_is_built(kernels):
    names = [n for n in kernels if "fn_" in n]
    # the three modes of the sliding kernel, the scan, and the selection's count and copy kernels
    assert len(names) == 6 and len(names) == len(kernels), sorted(kernels)
    for mode in (0, 1, 2):
        assert sum("fn_sliding_kernelILi%dEE" % mode in n for n in names) == 1, mode
    for k in ("fn_scan_kernel", "fn_select_count_kernel", "fn_select_copy_kernel"):
        assert sum(k in n for n in names) == 1, k


def test_no_kernel_has_a_private_segment(kernels):
    for n, k in kernels.items():
        assert k["scratch"] == 0 and k["spill"] == 0, (n, k)


def test_registers_fit_the_occupancy_of_the_launch_bounds(kernels):
    """waves per SIMD from the 512-register file: __launch_bounds__(256, w) plans for w, so at most 512 / w registers per lane — 4 waves
    for the sliding kernel, none stated for the scan and the selection kernels"""
    for n, k in kernels.items():
        cap = 128 if "fn_sliding_kernel" in n else 512
        assert k["vgpr"] <= cap, (n, k["vgpr"], cap)
