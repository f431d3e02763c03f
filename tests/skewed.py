"""Skewed, guarded array views for the alignment tests (tests/test_gpu_alignment.py; an ordinary module like tests/vad_oracle.py).

include/ssp.h asks of a device array only the natural alignment of its element type, while the kernels choose between 16-byte and scalar
code from the low four address bits.  ``view`` places an array at a chosen address modulo 16 inside a larger flat buffer and surrounds
it with guard zones of at least 256 bytes:

  input arrays  (``fill`` = the values): the guards hold elements that cannot go unnoticed if a kernel uses them — NaN for float32,
                32767 for int16 (it would become an utterance's peak), the largest value for the other integer types;
  output arrays (``fill`` = None): the guards, and the view itself before the call, hold the byte 0xA5.

A NaN does not show in every result: a reduction with fmaxf (the VAD peak) drops it.  ``guard`` replaces the value for such a case —
the float32 VAD inputs take ``BIG`` (3e38, finite), which would become the utterance's peak if a kernel read it.

``check_guards`` reads the buffer back and asserts that every guard byte still holds what ``view`` put there, for both kinds.
``backend`` "torch" allocates on the current CUDA device, "numpy" on the host (the helper's own CPU test).
"""
import numpy as np

GUARD_BYTES = 256
PATTERN = 0xA5
POISON = {"float32": np.float32(np.nan), "int16": np.int16(32767), "int32": np.int32(2 ** 31 - 1), "uint8": np.uint8(255)}
BIG = np.float32(3e38)


class Guarded:
    """what check_guards needs: the flat buffer, where the view lies in it and the guard bytes as they were written"""

    def __init__(self, buf, off, nbytes, front, back, backend):
        self.buf, self.off, self.nbytes, self.front, self.back, self.backend = buf, off, nbytes, front, back, backend

    def bytes(self):
        if self.backend == "torch":
            return self.buf.cpu().numpy()
        return np.array(self.buf, copy=True)


def _address(buf, backend):
    return int(buf.data_ptr()) if backend == "torch" else int(buf.ctypes.data)


def view(n, dtype, skew_bytes, fill=None, backend="torch", guard=None):
    """-> (array of n elements of dtype whose address modulo 16 is skew_bytes, Guarded token); guard: the value around an input
    array instead of POISON's"""
    dt = np.dtype(dtype)
    n, skew_bytes, isz = int(n), int(skew_bytes), dt.itemsize
    assert dt.name in POISON, "no guard value for %s" % dt.name
    assert 0 <= skew_bytes < 16 and skew_bytes % isz == 0, "a %s array cannot sit %d bytes past a 16-byte line" % (dt.name, skew_bytes)
    nbytes = n * isz
    total = nbytes + 2 * GUARD_BYTES + 32
    if backend == "torch":
        import torch
        buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    elif backend == "numpy":
        buf = np.empty(total, dtype=np.uint8)
    else:
        raise ValueError("backend must be 'torch' or 'numpy'")
    base = _address(buf, backend)   # the real address: the allocator's alignment is not assumed
    off = GUARD_BYTES + (skew_bytes - (base + GUARD_BYTES)) % 16
    assert (base + off) % 16 == skew_bytes and (base + off) % isz == 0
    assert off >= GUARD_BYTES and total - off - nbytes >= GUARD_BYTES
    img = np.full(total, PATTERN, dtype=np.uint8)
    if fill is not None:
        vals = np.ascontiguousarray(fill, dtype=dt).reshape(-1)
        assert vals.shape[0] == n, "fill holds %d elements, the view %d" % (vals.shape[0], n)
        lead = off % isz
        typed = img[lead: lead + (total - lead) // isz * isz].view(dt)   # elements on the view's own grid, before and behind it
        typed[:] = POISON[dt.name] if guard is None else dt.type(guard)
        typed[(off - lead) // isz: (off - lead) // isz + n] = vals
    front, back = img[:off].copy(), img[off + nbytes:].copy()
    if backend == "torch":
        buf.copy_(torch.from_numpy(img))
        arr = buf[off: off + nbytes].view(getattr(torch, dt.name))
        got = int(arr.data_ptr()) if n else base + off
    else:
        buf[:] = img
        arr = buf[off: off + nbytes].view(dt)
        got = int(arr.ctypes.data) if n else base + off
    assert got == base + off and got % 16 == skew_bytes, "view landed at %#x, wanted %d past a 16-byte line" % (got, skew_bytes)
    return arr, Guarded(buf, off, nbytes, front, back, backend)


def check_guards(token, what=""):
    """every guard byte in front of and behind the view holds what view() wrote"""
    now = token.bytes()
    front, back = now[:token.off], now[token.off + token.nbytes:]
    bad = np.flatnonzero(front != token.front)
    assert bad.size == 0, "%s: %d guard bytes in front of the view changed, the nearest %d bytes before it" % (
        what, bad.size, token.off - int(bad[-1]))
    bad = np.flatnonzero(back != token.back)
    assert bad.size == 0, "%s: %d guard bytes behind the view changed, the nearest %d bytes past its end" % (what, bad.size, int(bad[0]))
