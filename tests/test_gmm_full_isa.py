"""Guards on the gfx950 ISA of the full-covariance GMM kernels (hipcc cross-compiles here, no GPU), in the pattern of
tests/test_featnorm_isa.py: csrc/gmm_full.hip is part of the library build, the expected kernel instances exist, no kernel of the unit has
a private segment, and every kernel's registers per lane fit the occupancy its __launch_bounds__ states.  Nothing else is inspected."""
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
    of csrc/gmm_full.hip compiled to gfx950 assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    src = "gmm_full.hip"
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
    names = [n for n in kernels if "gmm_full_" in n]
    # the E pass at one and two row tiles, the moment pass at one, two and three tiles, the two reductions and the utterance kernel
    assert len(names) == 8 and len(names) == len(kernels), sorted(kernels)
    for nrt in (1, 2):
        assert sum("gmm_full_e_kernelILi%dEE" % nrt in n for n in names) == 1, nrt
    for nt in (1, 2, 3):
        assert sum("gmm_full_mom_kernelILi%dEE" % nt in n for n in names) == 1, nt
    for k in ("gmm_full_reduce_kernel", "gmm_full_lse_reduce_kernel", "gmm_full_utt_kernel"):
        assert sum(k in n for n in names) == 1, k


def test_no_kernel_has_a_private_segment(kernels):
    for n, k in kernels.items():
        assert k["scratch"] == 0 and k["spill"] == 0, (n, k)


def test_registers_fit_the_occupancy_of_the_launch_bounds(kernels):
    """every kernel states __launch_bounds__(256) and no waves per SIMD: one wave per SIMD, at most 512 registers per lane"""
    for n, k in kernels.items():
        assert k["vgpr"] <= 512, (n, k["vgpr"])
