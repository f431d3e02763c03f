"""Guards on the gfx950 ISA of the VAD feature kernel (hipcc cross-compiles here, no GPU): only squared magnitudes are used (no square
root), the block shares come from a reciprocal (no division expansion), nothing spills in the frame loop, and log2 is the hardware
instruction."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_signal_processing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _kernels(src, tmp_path):
    """kernel name -> instruction lines of csrc/<src> compiled to gfx950 assembly with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    assert src in SOURCES, "%s is not part of the library build" % src
    out = str(tmp_path / (src + ".s"))
    r = subprocess.run([HIPCC, *FLAGS, *SOURCE_FLAGS.get(src, []), "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)],
                       capture_output=True, text=True, timeout=900)
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


def _count(instrs, pattern):
    return sum(1 for t in instrs if re.match(pattern, t.split()[0]))


def test_vad_feature_kernel_instruction_classes(tmp_path):
    k = _kernels("vad.hip", tmp_path)
    inst = {n: v for n, v in k.items() if "vad_feature_kernel" in n}
    assert len(inst) == 2, list(k)   # float32 and int16 samples
    for n, v in inst.items():
        assert _count(v, r"v_sqrt_f32") == 0, n
        assert _count(v, r"v_div_(scale|fmas|fixup)") == 0, n
        assert _count(v, r"scratch_") == 0, n
        assert _count(v, r"v_log_f32") >= 1, n
        assert _count(v, r"flat_(load|store)") == 0, n          # the stage and the images are addressed as LDS
        assert _count(v, r"buffer_load_dwordx4") >= 5, n        # the samples arrive by LDS-DMA: no other vector load of samples
        assert _count(v, r"v_pk_(fma|mul|add)_f32") > 100, n     # the transform runs on packed fp32
