"""Guards on the gfx950 ISA of the conv + GRU trainer's recurrent step kernels (hipcc cross-compiles here, no GPU): the forward step
kernels and the two backward step kernels multiply on the exact-fp32 matrix instruction and on no other, use no scratch, and expand no
division.  (The file's GEMMs over the stash, the loss and Adam are dnn_train.hip's kernels: test_dnn_train_isa.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vad_isa import _count, _kernels  # noqa: E402  (compile csrc/<src> with the shipped flags -> kernel name: instruction lines)


def test_gru_train_step_kernels_instruction_classes(tmp_path):
    k = _kernels("gru_train.hip", tmp_path)
    fwd = {n: v for n, v in k.items() if "gt_fwd_kernel" in n}
    bwd = {n: v for n, v in k.items() if "gt_bwd_r_kernel" in n or "gt_bwd_h_kernel" in n}
    assert len(fwd) == 3, list(k)    # z | r with either activation, the candidate
    assert len(bwd) == 4, list(k)    # two launches per step, either activation
    for n, v in {**fwd, **bwd}.items():
        assert _count(v, r"v_mfma_f32_16x16x4_f32") >= 8, n   # (the k loop is not unrolled: two register sets x four k)
        assert _count(v, r"v_mfma_") == _count(v, r"v_mfma_f32_16x16x4_f32"), n   # no other matrix instruction
        assert _count(v, r"scratch_") == 0, n
        assert _count(v, r"v_div_(scale|fmas|fixup)") == 0, n
