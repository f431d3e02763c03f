"""Guards on the gfx950 ISA of the recurrent trainer's kernels (hipcc cross-compiles here, no GPU): the forward kernels (with and without
the stash) and the backward-through-time kernels multiply on the exact-fp32 matrix instruction and on no other, keep their weights in
registers without spilling, and expand no division.  (The file's GEMMs, loss and Adam are dnn_train.hip's kernels: test_dnn_train_isa.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vad_isa import _count, _kernels  # noqa: E402  (compile csrc/<src> with the shipped flags -> kernel name: instruction lines)


def test_lstm_train_kernels_instruction_classes(tmp_path):
    k = _kernels("lstm_train.hip", tmp_path)
    fwd = {n: v for n, v in k.items() if "lt_fwd_kernel" in n}
    bwd = {n: v for n, v in k.items() if "lt_bwd_kernel" in n}
    assert len(fwd) == 22, list(k)   # 2 .. 12 groups of 16 k, with and without the stash
    assert len(bwd) == 8, list(k)    # 1 .. 8 hidden tiles
    assert len(k) == 30, list(k)     # and no other kernel in the file
    for n, v in {**fwd, **bwd}.items():
        assert _count(v, r"v_mfma_f32_16x16x4_f32") >= 16, n
        assert _count(v, r"v_mfma_") == _count(v, r"v_mfma_f32_16x16x4_f32"), n   # no other matrix instruction
        assert _count(v, r"scratch_") == 0, n
        assert _count(v, r"v_div_(scale|fmas|fixup)") == 0, n
