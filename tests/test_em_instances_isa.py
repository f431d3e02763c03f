"""The kernels csrc/gmm_em.hip compiles for gfx950 are exactly tests/em_cases.py's INSTANCES (hipcc cross-compiles here, no GPU).  A list
of kernel names, read the way tests/test_isa_guards.py reads them; the instruction text is not looked at."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_cases as E  # noqa: E402
from test_isa_guards import _isa  # noqa: E402


def _instance(mangled):
    """_ZN3ssp<len><name>[ILi<NCT>ELb<FUSE>EE]Ev... -> the tuple of em_cases.INSTANCES"""
    m = re.match(r"_ZN3ssp(\d+)", mangled)
    assert m, mangled
    start = m.end()
    name = mangled[start:start + int(m.group(1))]
    t = re.match(r"ILi(\d+)ELb([01])EE", mangled[start + len(name):])
    return (name, int(t.group(1)), t.group(2) == "1") if t else (name,)


def test_em_kernels_are_the_table(tmp_path):
    got = sorted(_instance(n) for n in _isa("gmm_em.hip", tmp_path))
    assert got == sorted(E.INSTANCES), (got, sorted(E.INSTANCES))
    assert len(set(E.INSTANCES)) == len(E.INSTANCES)
