"""Guards on the gfx950 ISA of the fused PLP tail's fixed instances (hipcc cross-compiles here, no GPU): nothing spills (the private
segment is empty), exp2 and log2 are the hardware instructions, and the per-frame part — from the first v_exp_f32 of the compression to
the v_log_f32 of c0, with the autocorrelation and Levinson-Durbin in between — holds no division expansion (div_nr is kept)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_signal_processing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _compile(src, tmp_path):
    """-> (kernel name -> instruction lines, kernel name -> private segment bytes) of csrc/<src> compiled with the shipped build's flags"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from speech_signal_processing_amd.build import FLAGS, SOURCE_FLAGS, SOURCES
    assert src in SOURCES, "%s is not part of the library build" % src
    out = str(tmp_path / (src + ".s"))
    r = subprocess.run([HIPCC, *FLAGS, *SOURCE_FLAGS.get(src, []), "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    kernels, cur = {}, None
    for line in text.splitlines():
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
    private = {}
    for name in kernels:   # the kernel's entry in the amdhsa.kernels metadata: fields in alphabetical order, .name before .private_...
        m = re.search(r"\.name:\s+%s\s*\n(?:\s+\.[a-z_]+:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), text)
        if m:
            private[name] = int(m.group(1))
    return kernels, private


def test_fused_plp_tail_instruction_classes(tmp_path):
    kernels, private = _compile("plp.hip", tmp_path)
    inst = {n: v for n, v in kernels.items() if "plp_feat_fixed_kernel" in n}
    assert len(inst) == 4, list(kernels)   # 21 and 17 bands, float32 and float64 rows
    for n, v in inst.items():
        assert private.get(n) == 0, (n, private.get(n))
        ops = [t.split()[0] for t in v]
        exp = [i for i, o in enumerate(ops) if o.startswith("v_exp_f32")]
        log = [i for i, o in enumerate(ops) if o.startswith("v_log_f32")]
        assert len(exp) >= 1 and len(log) >= 1, (n, len(exp), len(log))
        assert exp[0] < log[-1], n
        frame = ops[exp[0]:log[-1] + 1]
        assert len(frame) > 300, (n, len(frame))   # (the span does hold the autocorrelation and the Levinson recursion)
        assert not [o for o in frame if re.match(r"v_div_(scale|fmas|fixup)", o)], n
