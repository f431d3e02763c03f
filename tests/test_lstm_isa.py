"""Guards on the gfx950 ISA of the LSTM kernel (hipcc cross-compiles here, no GPU): every instance multiplies on the exact-fp32 matrix
instruction, nothing spills, the gates' reciprocals are the hardware instruction (no division expansion), and the weight ring is
addressed as LDS."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vad_isa import _count, _kernels  # noqa: E402  (compile csrc/<src> with the shipped flags -> kernel name: instruction lines)


def test_lstm_kernel_instruction_classes(tmp_path):
    k = _kernels("lstm.hip", tmp_path)
    inst = {n: v for n, v in k.items() if "lstm_kernel" in n}
    assert len(inst) == 8, list(k)   # 1, 2, 4, 8 hidden tiles x hard_sigmoid, sigmoid
    for n, v in inst.items():
        m = re.search(r"lstm_kernelILi(\d+)ELi(\d+)E", n)
        HT, act = int(m.group(1)), int(m.group(2))
        # per hidden tile: 4 gates x 4 k-steps for each of up to 4 input groups and HT state groups (one unrolled time step)
        assert _count(v, r"v_mfma_f32_16x16x4_f32") == HT * 16 * (4 + HT), n
        assert _count(v, r"v_mfma_") == _count(v, r"v_mfma_f32_16x16x4_f32"), n   # no other matrix instruction
        assert _count(v, r"scratch_") == 0, n
        assert _count(v, r"v_div_(scale|fmas|fixup)") == 0, n
        assert _count(v, r"flat_(load|store|atomic)") == 0, n          # ring and bias table are addressed as LDS
        assert _count(v, r"global_load_lds_dwordx4") >= 1, n          # the weights arrive by LDS-DMA
        assert _count(v, r"ds_read_b128") >= HT * 4 * (1 + HT), n      # operand fragments in 16-byte reads
        # per unit and step: tanh twice (v_exp + v_rcp each), and a logistic gate three times more in the sigmoid instances
        per_tile = 4 * (2 + (3 if act else 0))
        assert _count(v, r"v_exp_f32") == HT * per_tile and _count(v, r"v_rcp_f32") == HT * per_tile, (n, _count(v, r"v_exp_f32"))
