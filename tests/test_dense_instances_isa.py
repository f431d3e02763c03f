"""The kernels behind ssp_dense_forward and ssp_dnn_forward that csrc/cosine.hip, csrc/dense.hip and csrc/dnn_chain.hip compile for gfx950
are exactly tests/dense_cases.py's INSTANCES (hipcc cross-compiles here, no GPU).  A list of kernel names, read the way
tests/test_isa_guards.py reads them."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_cases as K  # noqa: E402
from test_isa_guards import _isa  # noqa: E402


def test_register_gemm_dense_instances_are_the_table(tmp_path):
    k = _isa("cosine.hip", tmp_path)
    got = []
    for n in k:
        m = re.search(r"cosine_reg_kernelILi(\d+)ELb1EE", n)      # <NQ, DENSE = true>
        if m:
            got.append(("cosine_reg_kernel", int(m.group(1))))
    want = [i for i in K.INSTANCES if i[0] == "cosine_reg_kernel"]
    assert sorted(got) == sorted(want), (sorted(got), [n for n in k if "cosine_reg" in n])
    assert sorted(nq for _, nq in want) == sorted(set(K.kernel_of(d)[1] for d in range(1, 257)))


def test_tiled_gemm_is_present(tmp_path):
    k = _isa("dense.hip", tmp_path)
    names = [n for n in k if re.search(r"\d+dense_kernelE", n)]
    assert len(names) == 1 and ("dense_kernel",) in K.INSTANCES, list(k)


def test_chain_and_pack_kernels_are_present(tmp_path):
    k = _isa("dnn_chain.hip", tmp_path)
    for name in ("dnn_chain_kernel", "dnn_pack_kernel"):
        assert (name,) in K.INSTANCES
        assert len([n for n in k if re.search(r"\d+%sE" % name, n)]) == 1, (name, list(k))
