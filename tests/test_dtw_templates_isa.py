"""Guards on the gfx950 ISA of the batched DTW template kernels (hipcc cross-compiles here, no GPU): neither kernel uses scratch, the
forward kernel does float64 arithmetic and writes directions as bytes or dwords, never 8-byte cell values."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_signal_processing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    """(kernel name -> instruction lines, kernel name -> scratch bytes of the resource summary) of csrc/dtw_templates.hip compiled to
    gfx950 assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    src = "dtw_templates.hip"
    assert src in SOURCES, "%s is not part of the library build" % src
    out = str(tmp_path_factory.mktemp("isa") / (src + ".s"))
    r = subprocess.run([HIPCC, *FLAGS, *SOURCE_FLAGS.get(src, []), "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, scratch, cur, last = {}, {}, None, None
    for line in open(out):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = last = m.group(1)
            kernels[cur] = []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):   # the end of the function, not its first s_endpgm: an early-exit block may precede the body
            cur = None
            continue
        t = line.strip()
        m = re.match(r";\s*ScratchSize:\s*(\d+)", t)
        if m and last is not None:
            scratch[last] = int(m.group(1))
        if cur is None or not t or t.startswith((";", ".")):
            continue
        kernels[cur].append(t)
    return kernels, scratch


def _count(instrs, pattern):
    return sum(1 for t in instrs if re.match(pattern, t.split()[0]))


def test_template_kernels_have_no_scratch(unit):
    kernels, scratch = unit
    names = [n for n in kernels if "dtw_dir_kernel" in n or "dtw_trace_kernel" in n]
    assert len([n for n in names if "dtw_dir_kernel" in n]) == 4 and len([n for n in names if "dtw_trace_kernel" in n]) == 1, list(kernels)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert _count(kernels[n], r"scratch_") == 0, n
        assert _count(kernels[n], r"buffer_(load|store)") == 0, n   # (spills would go through the scratch buffer)


def test_forward_kernel_is_float64_and_stores_no_cell_values(unit):
    kernels, _ = unit
    for n, v in kernels.items():
        if "dtw_dir_kernel" not in n:
            continue
        assert _count(v, r"v_add_f64") >= 4, n
        assert _count(v, r"v_(min|cmp_\w+)_f64|v_cmp\w*_f64") >= 4, n
        assert _count(v, r"global_store_dwordx2") == 0, n
        assert _count(v, r"flat_store_dwordx2") == 0, n
        assert _count(v, r"(global|flat)_store_dwordx[34]") == 0, n
        assert _count(v, r"global_store_(byte|dword)$") >= 1, n


def test_traceback_walks_in_lds(unit):
    kernels, _ = unit
    v = [v for n, v in kernels.items() if "dtw_trace_kernel" in n][0]
    assert _count(v, r"ds_read_u8") >= 1       # the walk's dependent reads are LDS reads
    assert _count(v, r"v_add_f64") >= 1        # (x + t) / 2 in float64
    assert _count(v, r"global_atomic|flat_atomic") == 0
