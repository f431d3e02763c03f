"""Guards on the gfx950 ISA of the VB-HMM resegmentation kernels (hipcc cross-compiles here, no GPU), in the pattern of
tests/test_featnorm_isa.py: csrc/vbhmm.hip is part of the library build, every instance is built, no kernel of the unit has a private
segment, and every kernel's registers per lane fit the occupancy its __launch_bounds__ states.  Nothing else is inspected."""
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
    of csrc/vbhmm.hip compiled to gfx950 assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    src = "vbhmm.hip"
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
    names = [n for n in kernels if "vb_" in n]
    # the row pre-pass and the main kernel for 16, 32 and 64 padded states, LDS- and workspace-resident
    assert len(names) == 7 and len(names) == len(kernels), sorted(kernels)
    assert sum("vb_rowstat_kernel" in n for n in names) == 1
    for ns in (1, 2, 4):
        for res in (0, 1):
            assert sum("vb_hmm_kernelILi%dELb%dEE" % (ns, res) in n for n in names) == 1, (ns, res)


def test_no_kernel_has_a_private_segment(kernels):
    for n, k in kernels.items():
        assert k["scratch"] == 0 and k["spill"] == 0, (n, k)


def test_registers_fit_the_occupancy_of_the_launch_bounds(kernels):
    """waves per SIMD from the 512-register file: __launch_bounds__(256, w) plans for w, so at most 512 / w registers per lane — 4 waves
    for the instances of 16 and 32 padded states, 2 for 64, none stated for the row pre-pass"""
    for n, k in kernels.items():
        cap = 512 if "vb_rowstat_kernel" in n else (256 if "vb_hmm_kernelILi4E" in n else 128)
        assert k["vgpr"] <= cap, (n, k["vgpr"], cap)
