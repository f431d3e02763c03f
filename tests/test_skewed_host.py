"""CPU test of tests/skewed.py on its numpy backend: the helper the alignment tests stand on must itself place views exactly and notice
a single changed guard byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skewed as SK  # noqa: E402

# every (dtype, skew) tests/test_gpu_alignment.py uses, and the aligned placement its baselines use
SKEWS = {"float32": (0, 4, 8, 12), "int32": (0, 4, 8, 12), "int16": (0, 2, 6, 8), "uint8": (0, 1, 3)}
CASES = [(d, s) for d, ss in SKEWS.items() for s in ss]


@pytest.mark.parametrize("dtype,skew", CASES)
@pytest.mark.parametrize("n", [0, 1, 77])
def test_view_lands_on_the_asked_skew_with_full_guards(dtype, skew, n):
    fill = (np.arange(n) % 100).astype(dtype)
    for f in (fill, None):
        arr, tok = SK.view(n, dtype, skew, f, "numpy")
        assert arr.dtype == np.dtype(dtype) and arr.shape == (n,)
        base = tok.buf.ctypes.data
        if n:
            assert arr.ctypes.data % 16 == skew and arr.ctypes.data == base + tok.off
        assert (base + tok.off) % 16 == skew
        assert tok.off >= SK.GUARD_BYTES and tok.buf.size - tok.off - tok.nbytes >= SK.GUARD_BYTES
        assert tok.nbytes == n * np.dtype(dtype).itemsize
        if f is None:
            assert (tok.buf == SK.PATTERN).all()          # guards and the unwritten view alike
        else:
            assert np.array_equal(arr, fill)
        SK.check_guards(tok)
        arr[:] = 1                                        # writing the view itself is not a guard fault
        SK.check_guards(tok)


@pytest.mark.parametrize("dtype,skew", CASES)
def test_input_guards_hold_values_that_cannot_go_unnoticed(dtype, skew):
    arr, tok = SK.view(5, dtype, skew, np.ones(5, dtype), "numpy")
    isz = np.dtype(dtype).itemsize
    before = tok.buf[tok.off - 64 * isz: tok.off].view(dtype)
    behind = tok.buf[tok.off + tok.nbytes: tok.off + tok.nbytes + 64 * isz].view(dtype)
    for g in (before, behind):
        if dtype == "float32":
            assert np.isnan(g).all()
        else:
            assert (g == np.iinfo(dtype).max).all()
    assert SK.POISON["int16"] == 32767
    if dtype == "float32":   # a finite guard for results a NaN would not reach (a maximum)
        arr, tok = SK.view(5, dtype, skew, np.ones(5, dtype), "numpy", guard=SK.BIG)
        around = np.concatenate([tok.buf[tok.off - 256: tok.off].view(dtype), tok.buf[tok.off + tok.nbytes: tok.off + tok.nbytes + 256].view(dtype)])
        assert (around == SK.BIG).all() and np.isfinite(SK.BIG) and np.array_equal(arr, np.ones(5, dtype))
        SK.check_guards(tok)


@pytest.mark.parametrize("dtype,skew", CASES)
@pytest.mark.parametrize("as_input", [True, False])
def test_check_guards_notices_one_changed_byte_on_either_side(dtype, skew, as_input):
    fill = np.ones(9, dtype) if as_input else None
    for where in ("first", "before", "behind", "last"):
        arr, tok = SK.view(9, dtype, skew, fill, "numpy")
        pos = {"first": 0, "before": tok.off - 1, "behind": tok.off + tok.nbytes, "last": tok.buf.size - 1}[where]
        tok.buf[pos] ^= 0x01
        with pytest.raises(AssertionError, match="in front of" if where in ("first", "before") else "behind"):
            SK.check_guards(tok, where)
        tok.buf[pos] ^= 0x01
        SK.check_guards(tok, where)


def test_view_refuses_a_skew_the_element_type_cannot_have():
    with pytest.raises(AssertionError):
        SK.view(4, "float32", 2, None, "numpy")
    with pytest.raises(AssertionError):
        SK.view(4, "int16", 3, None, "numpy")
    with pytest.raises(AssertionError):
        SK.view(4, "float32", 4, np.zeros(5, np.float32), "numpy")
