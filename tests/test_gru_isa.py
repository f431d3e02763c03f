"""Guards on the gfx950 ISA of the GRU step kernel (hipcc cross-compiles here, no GPU): every instance multiplies on the exact-fp32
matrix instruction only, nothing spills, no division is expanded, and the logistic gates are the hardware exponential and reciprocal."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vad_isa import _count, _kernels  # noqa: E402  (compile csrc/<src> with the shipped flags -> kernel name: instruction lines)


def test_gru_step_kernel_instruction_classes(tmp_path):
    k = _kernels("gru.hip", tmp_path)
    inst = {n: v for n, v in k.items() if "gru_step_kernel" in n}
    # reset_after: one launch (mode 0) x 2 activations; without: gates (mode 1) x 2 activations + the candidate (mode 2, no gate)
    assert len(inst) == 5, list(k)
    for n, v in inst.items():
        m = re.search(r"gru_step_kernelILi(\d+)ELi(\d+)E", n)
        mode, act = int(m.group(1)), int(m.group(2))
        assert _count(v, r"v_mfma_f32_16x16x4_f32") >= 1, n
        assert _count(v, r"v_mfma_") == _count(v, r"v_mfma_f32_16x16x4_f32"), n   # no other matrix instruction
        assert _count(v, r"scratch_") == 0, n
        assert _count(v, r"v_div_(scale|fmas|fixup)") == 0, n
        if act == 1 and mode in (0, 1):
            assert _count(v, r"v_exp_f32") >= 1 and _count(v, r"v_rcp_f32") >= 1, n
