"""Guards on the gfx950 ISA of the dense trainer's kernels (hipcc cross-compiles here, no GPU): the step kernels do not spill, and the three
GEMM forms multiply on the exact-fp32 matrix instruction and on no other."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vad_isa import _count, _kernels  # noqa: E402  (compile csrc/<src> with the shipped flags -> kernel name: instruction lines)


def test_dnn_train_kernels_instruction_classes(tmp_path):
    k = _kernels("dnn_train.hip", tmp_path)
    gemm = {n: v for n, v in k.items() if "dt_gemm_kernel" in n}
    assert len(gemm) == 3, list(k)   # forward, dX, dW
    step = dict(gemm)
    step.update({n: v for n, v in k.items() if "dt_loss_kernel" in n or "dt_adam_kernel" in n})
    assert len(step) == 5, list(k)
    for n, v in step.items():
        assert _count(v, r"scratch_") == 0, n
    for n, v in gemm.items():
        assert _count(v, r"v_mfma_f32_16x16x4_f32") >= 4, n
        assert _count(v, r"v_mfma_") == _count(v, r"v_mfma_f32_16x16x4_f32"), n   # no other matrix instruction
