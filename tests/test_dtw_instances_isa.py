"""The all-pairs DTW matcher instances that csrc/dtw.hip compiles for gfx950 are exactly tests/dtw_cases.py's INSTANCES (hipcc
cross-compiles here, no GPU).  A list of kernel names, read the way tests/test_isa_guards.py reads them."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_cases as K  # noqa: E402
from test_isa_guards import _isa  # noqa: E402


def test_compiled_matcher_instances_are_the_table(tmp_path):
    k = _isa("dtw.hip", tmp_path)
    got = []
    for n in k:
        m = re.search(r"dtw1_kernelILi(\d+)EE", n)
        if m:
            got.append(("dtw1_kernel", int(m.group(1))))
        m = re.search(r"dtw_kernelILi(\d+)EfLb0EE", n)     # <W, float, false>: the matcher; <16, double, true> is ssp_dtw_path's
        if m:
            got.append(("dtw_kernel", int(m.group(1))))
    assert sorted(got) == sorted(K.INSTANCES), (sorted(got), [n for n in k if "dtw" in n])
    others = [n for n in k if re.search(r"dtw_kernelILi\d+E", n) and "EfLb0EE" not in n]
    assert len(others) == 1 and "ILi16EdLb1EE" in others[0], others
