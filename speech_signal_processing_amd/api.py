"""Object layer over the C-ABI (include/ssp.h): Context, Segments, MfccPlan, GmmScorer, cosine_identify.

Bulk arrays may be numpy arrays (host pointers, the library stages them) or torch CUDA tensors (device pointers,
results stay on the device).  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import contextlib
import os

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .frontend import MfccConfig, MfccTables


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _as_f32(x, name):
    """-> (array-like kept alive, raw address, where)"""
    if _is_torch(x):
        import torch
        if not x.is_cuda:
            raise ValueError("%s: torch tensors must live on the GPU (pass numpy arrays for host data)" % name)
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        return x, x.data_ptr(), _lib.DEVICE
    a = np.ascontiguousarray(x, dtype=np.float32)
    return a, a.ctypes.data, _lib.HOST


def _as_samples(x, name):
    """-> (array kept alive, raw address, where, is_int16): int16 PCM (what utils.tools.read / scipy.io.wavfile return) stays int16 —
    half the bytes cross PCIe and the device widens (ssp_mfcc_run_i16); everything else goes as float32"""
    if _is_torch(x):
        import torch
        if x.is_cuda and x.dtype == torch.int16:
            x = x.contiguous()
            return x, x.data_ptr(), _lib.DEVICE, True
    elif isinstance(x, np.ndarray) and x.dtype == np.int16:
        a = np.ascontiguousarray(x)
        return a, a.ctypes.data, _lib.HOST, True
    return _as_f32(x, name) + (False,)


def _as_frames(feats, D, frame_seg=None):
    """_as_f32 of a (frames, D) feature matrix which, given ``frame_seg``, has a row for every frame of it"""
    keep, ptr, where = _as_f32(feats, "feats")
    if keep.ndim != 2 or keep.shape[1] != D:
        raise ValueError("feats must be (frames, %d)" % D)
    if frame_seg is not None and keep.shape[0] < frame_seg.total:
        raise ValueError("feats has fewer rows than the frame segments cover")
    return keep, ptr, where


def _current_raw_stream(device: int) -> int:
    """torch's current hipStream_t on ``device`` as an integer (0 = the default stream).  Every device-pointer call asks, so the short
    way is taken where torch has it: no Stream object is built."""
    import torch
    try:
        return int(torch._C._cuda_getCurrentRawStream(device))
    except AttributeError:
        return int(torch.cuda.current_stream(device).cuda_stream)


def _raw_ptr(x, where):
    # the address of an array on the side ``where`` names; None (an output nobody asked for) stays None: NULL for the library
    if x is None:
        return None
    return x.data_ptr() if where == _lib.DEVICE else x.ctypes.data


def _result(timing, ms, **arrays):
    """the dict an entry point returns: the named values in the order given, those that are None (not asked for) left out, and
    "kernel_ms" when ``timing`` is set"""
    res = {k: v for k, v in arrays.items() if v is not None}
    if timing:
        res["kernel_ms"] = ms
    return res


def _new_handle(fn, *args):
    """a handle made by a create call, which takes the address of the handle last; the return code is checked first"""
    h = C.c_void_p()
    _lib.check(fn(*args, C.byref(h)))
    return h


def _read_int(ctype, fn, *args):
    """the integer a getter of the library writes through its last argument"""
    n = ctype(0)
    _lib.check(fn(*args, C.byref(n)))
    return n.value


class _Handle:
    """What every object over a library handle shares: ``ctx``, ``_lib``, ``_h`` and the handle's life.  A class names its destroy symbol
    in ``_DESTROY`` and makes ``_h`` with ``_create``.  ``close`` may be called twice, on an object whose __init__ raised, and after the
    context has gone (the object holds the library itself)."""

    _DESTROY = ""

    def __init__(self, ctx):
        self.ctx = ctx
        self._lib = ctx._lib

    def _create(self, fn, *args):
        self._h = _new_handle(fn, *args)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """One HIP device + one stream (ssp_ctx).  stream=None: the library owns a stream; an int is a borrowed
    hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; 0 = the HIP default stream).  Device-pointer calls are ordered
    against torch's current stream whichever stream the context runs on (_ordered)."""

    _DESTROY = "ssp_ctx_destroy"

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = _lib.load()
        self._create(self._lib.ssp_ctx_create, int(device), C.c_void_p(stream or 0), 0 if stream is None else 1)
        self.device = int(device)
        self.stream = stream

    @classmethod
    def for_torch(cls, device: Optional[int] = None) -> "Context":
        import torch
        dev = torch.cuda.current_device() if device is None else int(device)
        return cls(dev, torch.cuda.current_stream(dev).cuda_stream)

    def sync(self):
        _lib.check(self._lib.ssp_ctx_sync(self._h))

    def calibrate(self, target_ms: float = 20.0) -> dict:
        """what this box sustains on two textbook loads (ssp_calibrate): a float4 copy (GB/s) and packed-fp32 FMA chains (TFLOP/s), each
        run for about target_ms on this context's stream — bench.py divides its headline by them to compare boxes"""
        v = [C.c_double() for _ in range(4)]
        _lib.check(self._lib.ssp_calibrate(self._h, float(target_ms), *[C.byref(x) for x in v]))
        return {"copy_gbs": v[0].value, "fma_tflops": v[1].value, "copy_ms": v[2].value, "fma_ms": v[3].value}

    @contextlib.contextmanager
    def _ordered(self, where):
        """Stream ordering around a call that takes device pointers.  The contract: the call sees everything queued on torch's CURRENT
        stream (of this device) at the time of the call, and work queued on that stream after the call returns sees the call's results.
        A context whose stream IS torch's current stream needs nothing for that (the kernels are queued behind the producers of their
        inputs and ahead of the consumers of their outputs): no event, no host wait.  Any other context — one that owns its stream, or
        one that borrowed a torch stream which is not the current one any more (a cached default_context(torch_stream=True) called
        under ``with torch.cuda.stream(s)``) — is ordered against nothing torch does now, so around the call its stream first waits
        for torch's current stream and torch's current stream then waits for it: two events, no host wait (ssp_ctx_wait_stream /
        _signal_stream).  Calls on different owned-stream contexts overlap, and the host runs ahead as it does with torch's own kernels."""
        order, ts = False, None
        if where == _lib.DEVICE:
            cur = _current_raw_stream(self.device)
            order = self.stream is None or int(self.stream) != cur
        host_sync = order and bool(os.environ.get("SSP_ORDER_SYNC"))  # (diagnostic: host waits on both sides, as before round 3)
        if order:
            if host_sync:
                import torch
                torch.cuda.current_stream(self.device).synchronize()
            else:
                ts = C.c_void_p(cur)
                _lib.check(self._lib.ssp_ctx_wait_stream(self._h, ts))
        try:
            yield
        finally:
            if order:
                if host_sync:
                    self.sync()
                else:
                    _lib.check(self._lib.ssp_ctx_signal_stream(self._h, ts))

    def _run(self, fn, where, timing, *args):
        """THE call of an entry point that takes ``float* kernel_ms`` last: inside _ordered, with that argument NULL unless ``timing`` is
        set, the return code checked before _ordered ends (its ``finally`` signals the stream for a failed call too).  -> the kernel
        milliseconds (0.0 without timing).  Everything ``args`` points into is a local of the caller, alive until this returns."""
        ms = C.c_float(0.0)
        with self._ordered(where):
            _lib.check(fn(*args, C.byref(ms) if timing else None))
        return ms.value

    # ---- collectives (include/ssp.h: ssp_comm_*): one process and one Context per GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        """128 opaque bytes made on rank 0; ship them to every rank (any transport) and pass them to comm_init."""
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        _lib.check(_lib.load().ssp_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank: int, nranks: int, unique_id: bytes):
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % _lib.COMM_ID_BYTES)
        _lib.check(self._lib.ssp_comm_init(self._h, int(rank), int(nranks), C.c_char_p(unique_id)))

    def comm_destroy(self):
        _lib.check(self._lib.ssp_comm_destroy(self._h))

    def comm_info(self):
        r, n = C.c_int(), C.c_int()
        _lib.check(self._lib.ssp_comm_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def allgather(self, local):
        """All-gather of equally shaped device tensors: returns [nranks * local.shape[0], ...] in rank order (RCCL over xGMI)."""
        import torch
        local = local.contiguous()
        _, n = self.comm_info()
        out = torch.empty((n * local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        with self._ordered(_lib.DEVICE):
            _lib.check(self._lib.ssp_allgather(self._h, C.c_void_p(local.data_ptr()), C.c_void_p(out.data_ptr()),
                                               C.c_size_t(local.numel() * local.element_size())))
        return out

    def allreduce_sum_(self, t):
        """In-place sum over ranks of a float32 / float64 device tensor."""
        import torch
        if t.dtype not in (torch.float32, torch.float64) or not t.is_contiguous():
            raise ValueError("allreduce_sum_ takes a contiguous float32 / float64 device tensor")
        with self._ordered(_lib.DEVICE):
            _lib.check(self._lib.ssp_allreduce_sum(self._h, C.c_void_p(t.data_ptr()), C.c_size_t(t.numel()), int(t.dtype == torch.float64)))
        return t

    def _empty(self, shape, where, dtype="float32"):
        if where == _lib.DEVICE:
            import torch
            return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda:%d" % self.device)
        return np.empty(shape, dtype=dtype)


_default_ctx = {}


def default_context(device: int = 0, torch_stream: bool = False) -> Context:
    key = (device, torch_stream)
    if key not in _default_ctx:
        _default_ctx[key] = Context.for_torch(device) if torch_stream else Context(device)
    return _default_ctx[key]


class Segments(_Handle):
    """Per-utterance offsets (ssp_segments): int64[n+1], uploaded once."""

    _DESTROY = "ssp_segments_destroy"

    def __init__(self, ctx: Context, offsets=None, _handle=None):
        super().__init__(ctx)
        if _handle is not None:
            self._h = _handle
        else:
            off = np.ascontiguousarray(offsets, dtype=np.int64)
            if off.ndim != 1 or off.size < 1:
                raise ValueError("offsets must be a 1-D int64 array of length n+1")
            self._create(self._lib.ssp_segments_create, ctx._h, off.ctypes.data_as(C.POINTER(C.c_int64)), off.size - 1)
        n, tot = C.c_int64(), C.c_int64()
        _lib.check(self._lib.ssp_segments_count(self._h, C.byref(n), C.byref(tot)))
        self.n = n.value
        out = np.empty(self.n + 1, dtype=np.int64)
        _lib.check(self._lib.ssp_segments_read(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        self.offsets = out

    @classmethod
    def from_lengths(cls, ctx: Context, lengths: Sequence[int]) -> "Segments":
        off = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(np.asarray(lengths, dtype=np.int64), out=off[1:])
        return cls(ctx, off)

    @property
    def total(self) -> int:
        return int(self.offsets[-1])


def _cfg_struct(cfg: MfccConfig) -> _lib.ssp_mfcc_cfg:
    s = _lib.ssp_mfcc_cfg()
    for k, v in cfg.as_dict().items():
        setattr(s, k, v)
    return s


class MfccPlan(_Handle):
    """Fused MFCC (+delta, +CMVN) pass for one dialect (ssp_mfcc_plan)."""

    _DESTROY = "ssp_mfcc_plan_destroy"

    def __init__(self, ctx: Context, tables: MfccTables):
        super().__init__(ctx)
        self.cfg = tables.cfg
        nb = self.cfg.n_fft // 2 + 1
        w = np.ascontiguousarray(tables.window, dtype=np.float32)
        fb = np.ascontiguousarray(tables.fbank, dtype=np.float32)
        dct = np.ascontiguousarray(tables.dct, dtype=np.float32)
        if w.shape != (self.cfg.win_len,) or fb.shape != (self.cfg.n_filt, nb) or dct.shape != (self.cfg.n_ceps, self.cfg.n_filt):
            raise ValueError("table shapes do not match the cfg")
        self._cs = _cfg_struct(self.cfg)
        self._create(self._lib.ssp_mfcc_plan_create, ctx._h, C.byref(self._cs), w.ctypes.data, fb.ctypes.data, dct.ctypes.data)

    @property
    def d_out(self) -> int:
        return self.cfg.d_out

    def set_reproducible(self, on: bool = True) -> "MfccPlan":
        """SSP_MFCC_REPRODUCIBLE (include/ssp.h): an utterance's float32 bits no longer depend on the batch or the machine."""
        _lib.check(self._lib.ssp_mfcc_plan_set_flags(self._h, 1 if on else 0))
        return self

    def num_frames(self, n_samples: int) -> int:
        return _read_int(C.c_int64, self._lib.ssp_mfcc_num_frames, C.byref(self._cs), int(n_samples))

    def frame_segments(self, sample_seg: Segments) -> Segments:
        return Segments(self.ctx, _handle=_new_handle(self._lib.ssp_mfcc_frame_segments, self._h, sample_seg._h))

    def run(self, samples, sample_seg: Segments, frame_seg: Optional[Segments] = None, out=None, variant: int = 0,
            timing: bool = False):
        """samples: float32[total samples] or int16 PCM (numpy -> host path, torch cuda -> device path).  Large host batches run as a
        copy / compute / copy-back pipeline inside the library (include/ssp.h, ssp_mfcc_run); pinned arrays (`pinned_empty`) get the
        full PCIe rate.  Returns feats (total_frames, d_out) [and kernel milliseconds when timing=True]."""
        if frame_seg is None:
            frame_seg = self.frame_segments(sample_seg)
        keep, ptr, where, is_i16 = _as_samples(samples, "samples")
        if keep.ndim != 1 and not (keep.ndim == 2 and keep.shape[0] * keep.shape[1] == sample_seg.total):
            raise ValueError("samples must be a flat array of all utterances' samples")
        if int(np.prod(keep.shape)) < sample_seg.total:
            raise ValueError("samples shorter than the segment table")
        if out is None:
            out = self.ctx._empty((frame_seg.total, self.d_out), where)
        okeep, optr, owhere = _as_f32(out, "out")
        if owhere != where or okeep is not out:
            raise ValueError("out must be a contiguous float32 array of the same kind as samples")
        fn = self._lib.ssp_mfcc_run_i16 if is_i16 else self._lib.ssp_mfcc_run
        ms = self.ctx._run(fn, where, timing, self._h, sample_seg._h, frame_seg._h, ptr, optr, where, int(variant))
        return (out, ms) if timing else out


def flatten_signals(signals):
    """a list of 1-D utterances -> (one flat array, their lengths).  When every utterance is int16 PCM (utils.tools.read /
    scipy.io.wavfile, utils/tools.py:45-47) the flat array stays int16: no widening pass on the host, half the bytes over PCIe, the
    device widens (ssp_mfcc_run_i16).  Anything else is converted to float32 as before."""
    sig = [np.asarray(s).reshape(-1) for s in signals]
    if sig and all(s.dtype == np.int16 for s in sig):
        return (sig[0] if len(sig) == 1 else np.concatenate(sig)), [s.shape[0] for s in sig]
    sig = [np.asarray(s, dtype=np.float32) for s in sig]
    return (np.concatenate(sig) if sig else np.zeros(0, dtype=np.float32)), [s.shape[0] for s in sig]


def list_table(arrays, kind="samples"):
    """The pointer table of a list-fed call (ssp_mfcc_run_list / ssp_gmm_score_list) -> (table np.uintp[n], kept arrays, element type).

    kind "samples": 1-D utterances after reshape(-1), with flatten_signals' dtype rule (all int16 -> int16, type 1; anything else float32
    per array, type 0).  kind "rows": 2-D feature matrices as np.vstack(...).astype(float32) would stack them (float32 -> type 0, float64 ->
    type 1 and narrowed by the library; any other common type is converted to it per array, then to float32 here).  A non-contiguous
    array is made contiguous for that array alone.  The kept arrays own the memory the table points into: hold them until the call
    returns."""
    if kind == "samples":
        keep = [np.asarray(a).reshape(-1) for a in arrays]
        if keep and all(a.dtype == np.int16 for a in keep):
            typ = 1
            keep = [np.ascontiguousarray(a) for a in keep]
        else:
            typ = 0
            keep = [np.ascontiguousarray(a, dtype=np.float32) for a in keep]
    elif kind == "rows":
        keep = [np.asarray(a) for a in arrays]
        rt = np.result_type(*{a.dtype for a in keep}) if keep else np.dtype(np.float32)   # (dtypes, not arrays: any count)
        if rt == np.float64:
            typ = 1
        else:
            typ = 0
            if rt != np.float32:   # (vstack promotes to the common type first, then astype rounds once)
                keep = [np.asarray(a, dtype=rt).astype(np.float32) for a in keep]
        keep = [np.ascontiguousarray(a, dtype=np.float64 if typ else np.float32) for a in keep]
    else:
        raise ValueError("kind must be 'samples' or 'rows'")
    # (__array_interface__ costs a fraction of .ctypes.data per array: thousands of utterances make that visible)
    table = np.fromiter((a.__array_interface__["data"][0] for a in keep), dtype=np.uintp, count=len(keep))
    return table, keep, typ


def mfcc_run_list(plan: "MfccPlan", signals, out_dtype=np.float64, timing: bool = False):
    """The MFCC pass on a list of 1-D utterances, read by the library from each array as it is (ssp_mfcc_run_list: no concatenation on
    the host; pinned slots filled by worker threads).  The same bits as plan.run(*flatten_signals(signals)) widened to out_dtype
    (float32 or float64).  Returns (feats (sum T_i, d_out), frame Segments) [and kernel milliseconds when timing=True]."""
    out_dtype = np.dtype(out_dtype)
    if out_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("out_dtype must be float32 or float64")
    table, keep, typ = list_table(signals, "samples")
    seg = Segments.from_lengths(plan.ctx, [a.shape[0] for a in keep])
    fseg = plan.frame_segments(seg)
    out = np.empty((fseg.total, plan.d_out), dtype=out_dtype)
    ms = plan.ctx._run(plan._lib.ssp_mfcc_run_list, _lib.HOST, timing, plan._h, seg._h, fseg._h, table.ctypes.data if table.size else None, typ,
                       out.ctypes.data, 1 if out_dtype == np.float64 else 0, 0)   # (keep owns what the table points into)
    return (out, fseg, ms) if timing else (out, fseg)


def pinned_empty(shape, dtype=np.float32):
    """a numpy array over page-locked host memory (torch's pinned allocator = hipHostMalloc): host-fed calls copy from / to such arrays
    asynchronously and at the full PCIe rate; the array keeps its tensor alive"""
    import torch
    t = torch.empty(tuple(np.atleast_1d(shape)), dtype=getattr(torch, np.dtype(dtype).name), pin_memory=True)
    return t.numpy()   # (the array's base keeps the pinned storage alive)


def enframe(ctx: Context, samples, frame_size: int, step: int, window):
    """(frame_size, ceil(n/step)) float32 frames, zero padded tail, times window — utils/processing.py:19-38."""
    keep, ptr, where = _as_f32(samples, "samples")
    if keep.ndim != 1:
        raise ValueError("samples must be 1-D")
    n = int(keep.shape[0])
    n_frames = -(-n // step)
    w = np.ascontiguousarray(window, dtype=np.float32)
    if w.shape != (frame_size,):
        raise ValueError("window must have frame_size taps")
    out = ctx._empty((frame_size, n_frames), where)
    ctx._run(ctx._lib.ssp_enframe, where, False, ctx._h, ptr, n, int(frame_size), int(step), w.ctypes.data, _raw_ptr(out, where), where)
    return out


def cepstrum(ctx: Context, X, fbank, dct, log_mode: int, floor_mode: int, eps: float):
    """DCT(log(X . fbank^T)) per row of X — utils/processing.py:91-107 on a batch of spectra."""
    keep, ptr, where = _as_f32(X, "X")
    if keep.ndim != 2:
        raise ValueError("X must be (rows, bins)")
    fb = np.ascontiguousarray(fbank, dtype=np.float32)
    dc = np.ascontiguousarray(dct, dtype=np.float32)
    if fb.ndim != 2 or fb.shape[1] != keep.shape[1] or dc.shape != (dc.shape[0], fb.shape[0]):
        raise ValueError("fbank must be (n_filt, bins) and dct (n_ceps, n_filt)")
    out = ctx._empty((int(keep.shape[0]), dc.shape[0]), where)
    ctx._run(ctx._lib.ssp_cepstrum, where, False, ctx._h, ptr, int(keep.shape[0]), int(keep.shape[1]), fb.ctypes.data, fb.shape[0],
             dc.ctypes.data, dc.shape[0], int(log_mode), int(floor_mode), float(eps), _raw_ptr(out, where), where)
    return out


def spectrum_abs(ctx: Context, reim, n_bins: int, scale: float = 1.0, power: int = 1):
    """rows of [re | im] (rows, 2 n_bins) -> scale * |.| (power 1) or scale * |.|^2 (power 2), (rows, n_bins)."""
    keep, ptr, where = _as_f32(reim, "reim")
    if keep.ndim != 2 or keep.shape[1] != 2 * n_bins:
        raise ValueError("reim must be (rows, 2 * n_bins)")
    out = ctx._empty((int(keep.shape[0]), int(n_bins)), where)
    ctx._run(ctx._lib.ssp_spectrum_abs, where, False, ctx._h, ptr, int(keep.shape[0]), int(n_bins), float(scale), int(power), _raw_ptr(out, where),
             where)
    return out


def delta_features(ctx: Context, feats, frame_seg: Segments, N: int = 2, timing: bool = False):
    keep, ptr, where = _as_f32(feats, "feats")
    if keep.ndim != 2:
        raise ValueError("feats must be (frames, dim)")
    out = ctx._empty(tuple(keep.shape), where)
    ms = ctx._run(ctx._lib.ssp_delta, where, timing, ctx._h, ptr, frame_seg._h, int(keep.shape[1]), int(N), _raw_ptr(out, where), where)
    return (out, ms) if timing else out


def cmvn_features(ctx: Context, feats, frame_seg: Segments, timing: bool = False):
    keep, ptr, where = _as_f32(feats, "feats")
    if keep.ndim != 2:
        raise ValueError("feats must be (frames, dim)")
    out = ctx._empty(tuple(keep.shape), where)
    ms = ctx._run(ctx._lib.ssp_cmvn, where, timing, ctx._h, ptr, frame_seg._h, int(keep.shape[1]), _raw_ptr(out, where), where)
    return (out, ms) if timing else out


def featnorm_sliding(ctx: Context, feats, frame_seg: Segments, window: int = 300, mode: int = 1, timing: bool = False):
    """Sliding-window normalisation of a ragged batch of feature rows (ssp_featnorm_sliding): per column, over the ``window`` frames
    centred on each frame and slid back inside its utterance, mode 0 subtracts the mean, mode 1 also divides by the deviation, mode 2
    warps to a standard normal by rank (feature warping).  feats (frames, dim): numpy -> host path, torch cuda -> device path (no host
    wait).  Returns an array like feats [and kernel milliseconds when timing=True]."""
    keep, ptr, where = _as_f32(feats, "feats")
    if keep.ndim != 2:
        raise ValueError("feats must be (frames, dim)")
    if int(keep.shape[0]) < frame_seg.total:
        raise ValueError("feats has fewer rows than the segment table")
    out = ctx._empty(tuple(keep.shape), where)
    ms = ctx._run(ctx._lib.ssp_featnorm_sliding, where, timing, ctx._h, ptr, frame_seg._h, int(keep.shape[1]), int(window), int(mode),
                  _raw_ptr(out, where), where)
    return (out, ms) if timing else out


def featnorm_table(window: int) -> np.ndarray:
    """The warping table of a window (ssp_featnorm_table; host only): float32[window * window], row n at offset (n - 1)^2 holds
    phi^-1(k / 2n) for k = 1 .. 2n - 1."""
    if not 1 <= int(window) <= _lib.FEATNORM_MAX_WINDOW:
        raise ValueError("window must lie in [1, %d]" % _lib.FEATNORM_MAX_WINDOW)
    out = np.empty(int(window) * int(window), dtype=np.float32)
    _lib.check(_lib.load().ssp_featnorm_table(int(window), out.ctypes.data))
    return out


def select_frames(ctx: Context, feats, frame_seg: Segments, mask, timing: bool = False):
    """The rows of feats whose mask entry is non-zero, packed in order (ssp_select_frames): feats (frames, dim) and mask (frames,) are
    arrays of the same kind (numpy, or torch cuda: the rows stay on the device; one host wait for the counts).  Returns (kept rows,
    the Segments of the kept rows, kept rows per utterance int64[n]) [and kernel milliseconds when timing=True]."""
    keep, ptr, where = _as_f32(feats, "feats")
    mk, mptr, mwhere = _as_u8(mask, "mask")
    if keep.ndim != 2:
        raise ValueError("feats must be (frames, dim)")
    if mwhere != where:
        raise ValueError("feats and mask must be arrays of the same kind")
    if int(keep.shape[0]) < frame_seg.total or int(np.prod(mk.shape)) < frame_seg.total:
        raise ValueError("feats or mask has fewer rows than the segment table")
    rows = int(frame_seg.offsets[-1] - frame_seg.offsets[0])
    out = ctx._empty((rows, int(keep.shape[1])), where)
    counts = np.zeros(frame_seg.n, dtype=np.int64)
    ms = ctx._run(ctx._lib.ssp_select_frames, where, timing, ctx._h, ptr, frame_seg._h, int(keep.shape[1]), mptr, _raw_ptr(out, where),
                  counts.ctypes.data_as(C.POINTER(C.c_int64)), where)
    kept = out[:int(counts.sum())]
    seg = Segments.from_lengths(ctx, counts)
    return (kept, seg, counts, ms) if timing else (kept, seg, counts)


def plp_post(ctx: Context, logspec, frame_seg: Segments, fmax_hz: float, plp_order: int = 13, rasta: bool = True, lift: float = 0.6,
             timing: bool = False):
    """Back end of sidekit's plp on the GPU (ssp_plp_post): (frames, bands) ln critical-band energies -> (frames, plp_order)
    cepstra (RASTA along each utterance of ``frame_seg``, equal loudness, ^0.33, autocorrelation, Levinson, LPC->cepstrum, lifter)."""
    keep, ptr, where = _as_f32(logspec, "logspec")
    if keep.ndim != 2:
        raise ValueError("logspec must be (frames, bands)")
    out = ctx._empty((int(keep.shape[0]), int(plp_order)), where)
    ms = ctx._run(ctx._lib.ssp_plp_post, where, timing, ctx._h, ptr, frame_seg._h, int(keep.shape[1]), float(fmax_hz), int(plp_order),
                  int(bool(rasta)), float(lift), _raw_ptr(out, where), where)
    return (out, ms) if timing else out


def plp_feature_columns(plp_order: int, left_dim: int = 0, delta_order: int = 0):
    """Column layout of ``plp_features``: -> (left columns, PLP columns), index arrays into an output row.  For b = 0 .. delta_order the
    row holds [left block b | PLP block b], a left block being left_dim / (1 + delta_order) columns wide."""
    nblk = 1 + int(delta_order)
    if left_dim % nblk:
        raise ValueError("left_dim=%d must be a multiple of 1 + delta_order = %d" % (left_dim, nblk))
    lw = left_dim // nblk
    bw = lw + int(plp_order)
    col = np.arange(nblk * bw).reshape(nblk, bw)
    return col[:, :lw].reshape(-1), col[:, lw:].reshape(-1)


def plp_features(ctx: Context, logspec, frame_seg: Segments, fmax_hz: float, plp_order: int = 13, rasta: bool = True, lift: float = 0.6,
                 left=None, delta_order: int = 0, scale: bool = False, out_dtype=np.float32, timing: bool = False, out=None):
    """The PLP feature recipes of the reference on the GPU (ssp_plp_features): (frames, bands) ln critical-band energies ->
    RASTA, cepstra, delta (delta_order >= 1), delta of delta (2), per-utterance scale — one kernel per call for 21 / 17 bands at order 13.
    ``left``: (frames, left_dim) finished columns (the MFCC plan's output with cmvn = scale and the same delta_order), interleaved
    unchanged: rows are [left block b | PLP block b] for b = 0 .. delta_order (``plp_feature_columns``).  numpy arrays in, numpy array
    out; torch cuda tensors in, torch cuda tensor out (no host wait).  Returns feats (frames, left_dim + (1 + delta_order) plp_order)
    of ``out_dtype`` (float32 or float64) [and kernel milliseconds when timing=True]."""
    out_dtype = np.dtype(out_dtype)
    if out_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("out_dtype must be float32 or float64")
    keep, ptr, where = _as_f32(logspec, "logspec")
    if keep.ndim != 2:
        raise ValueError("logspec must be (frames, bands)")
    F = int(keep.shape[0])
    lkeep, lptr, left_dim = None, None, 0
    if left is not None:
        lkeep, lptr, lwhere = _as_f32(left, "left")
        if lwhere != where:
            raise ValueError("left must be the same kind of array as logspec")
        if lkeep.ndim != 2 or int(lkeep.shape[0]) != F:
            raise ValueError("left must be (frames, left_dim)")
        left_dim = int(lkeep.shape[1])
    D = left_dim + (1 + int(delta_order)) * int(plp_order) if 0 <= int(delta_order) <= 2 else left_dim + int(plp_order)
    if out is None:
        out = ctx._empty((F, D), where, out_dtype.name)
    elif tuple(out.shape) != (F, D) or _is_torch(out) != (where == _lib.DEVICE) or str(out.dtype).split(".")[-1] != out_dtype.name \
            or not (out.is_contiguous() if _is_torch(out) else out.flags.c_contiguous):
        raise ValueError("out must be a contiguous (%d, %d) %s array of the same kind as logspec" % (F, D, out_dtype.name))
    ms = ctx._run(ctx._lib.ssp_plp_features, where, timing, ctx._h, ptr, frame_seg._h, int(keep.shape[1]), float(fmax_hz), int(plp_order),
                  int(bool(rasta)), float(lift), lptr, left_dim, int(delta_order), int(bool(scale)), _raw_ptr(out, where),
                  1 if out_dtype == np.float64 else 0, where)
    return (out, ms) if timing else out


def vad_num_frames(n_samples: int, step: int = 128) -> int:
    """math.ceil(n / step) — VAD.py:37 (no GPU)."""
    return _read_int(C.c_int64, _lib.load().ssp_vad_num_frames, int(n_samples), int(step))


def vad_frame_segments(ctx: Context, sample_seg: Segments, step: int = 128) -> Segments:
    return Segments(ctx, _handle=_new_handle(ctx._lib.ssp_vad_frame_segments, ctx._h, sample_seg._h, int(step)))


def vad_features(ctx: Context, samples, sample_seg: Segments, frame_seg: Optional[Segments] = None, frame_size: int = 256, step: int = 128,
                 normalize: bool = True, gate_zcr: bool = True, timing: bool = False):
    """VAD.py's feature() for every frame of a ragged batch in one pass (ssp_vad_features): samples float32 or int16 PCM, flat, laid out
    by sample_seg (numpy -> host path, torch cuda -> device path).  normalize: divide every utterance by its peak first (False: the samples are taken as
    they are); gate_zcr=False leaves the zero-crossing count ungated (VAD.py's bare ZCR).  Returns (zcr, power, entropy, frame_seg),
    float32[total frames] each
    [and kernel milliseconds when timing=True]."""
    if frame_seg is None:
        frame_seg = vad_frame_segments(ctx, sample_seg, step)
    keep, ptr, where, is_i16 = _as_samples(samples, "samples")
    if int(np.prod(keep.shape)) < sample_seg.total:
        raise ValueError("samples shorter than the segment table")
    zcr, power, ent = (ctx._empty((frame_seg.total,), where) for _ in range(3))
    ms = ctx._run(ctx._lib.ssp_vad_features, where, timing, ctx._h, ptr, 1 if is_i16 else 0, sample_seg._h, frame_seg._h, int(frame_size),
                  int(step), 1 if normalize else 0, 0 if gate_zcr else _lib.VAD_ZCR_UNGATED, _raw_ptr(zcr, where), _raw_ptr(power, where),
                  _raw_ptr(ent, where), where)
    return (zcr, power, ent, frame_seg, ms) if timing else (zcr, power, ent, frame_seg)


def vad_detect(ctx: Context, zcr, power_or_entropy, frame_seg: Segments, mode: int = 0, zcr_gate: float = 35.0, ampl: float = 0.3,
               amph: float = 12.0, min_len: int = 16, timing: bool = False):
    """mode 0: VAD_detection (VAD.py:136-182) per utterance on (zcr, power); mode 1: VAD_frequency (VAD.py:185-186) on the entropy with
    threshold ``ampl`` (ssp_vad_detect).  Returns (mask uint8[total frames], speech frames per utterance int32[n])
    [and kernel milliseconds when timing=True]."""
    pk, pptr, where = _as_f32(power_or_entropy, "power_or_entropy")
    if mode == 0:
        zk, zptr, zwhere = _as_f32(zcr, "zcr")
        if zwhere != where or int(np.prod(zk.shape)) < frame_seg.total:
            raise ValueError("zcr and power must be arrays of the same kind holding every frame of frame_seg")
    else:
        zk, zptr = None, None
    if int(np.prod(pk.shape)) < frame_seg.total:
        raise ValueError("fewer values than frame_seg has frames")
    mask = ctx._empty((frame_seg.total,), where, "uint8")
    count = ctx._empty((frame_seg.n,), where, "int32")
    ms = ctx._run(ctx._lib.ssp_vad_detect, where, timing, ctx._h, zptr, pptr, frame_seg._h, int(mode), float(zcr_gate), float(ampl), float(amph),
                  int(min_len), _raw_ptr(mask, where), _raw_ptr(count, where), where)
    return (mask, count, ms) if timing else (mask, count)


def _as_u8(x, name):
    """-> (array-like kept alive, raw address, where) of frame labels: nonzero = speech"""
    if _is_torch(x):
        import torch
        if not x.is_cuda:
            raise ValueError("%s: torch tensors must live on the GPU (pass numpy arrays for host data)" % name)
        if x.dtype != torch.uint8:
            x = (x != 0).to(torch.uint8)
        x = x.contiguous()
        return x, x.data_ptr(), _lib.DEVICE
    a = np.asarray(x)
    a = np.ascontiguousarray(a if a.dtype == np.uint8 else a != 0, dtype=np.uint8)
    return a, a.ctypes.data, _lib.HOST


def vad_sweep(ctx: Context, zcr, power_or_entropy, labels, frame_seg: Segments, zcr_gate=35.0, ampl=0.3, amph=12.0, mode: int = 0,
              min_len: int = 16, timing: bool = False):
    """The counts behind the F1 score of ``vad_detect`` against frame labels, for many threshold sets in one launch (ssp_vad_sweep; the
    objective of VAD.py's optimize, :204-210).  ``zcr_gate`` / ``ampl`` / ``amph``: scalars or arrays that broadcast against each other
    to ``n_par`` sets (mode 1 reads ``ampl`` only: the entropy thresholds).  ``labels``: nonzero = speech, one per frame of frame_seg.
    Returns counts int32 ``(n_par, n_utt, 3)`` = tp, fp, fn per set and utterance — a torch tensor for device inputs, numpy otherwise
    [and kernel milliseconds when timing=True]."""
    pk, pptr, where = _as_f32(power_or_entropy, "power_or_entropy")
    lk, lptr, lwhere = _as_u8(labels, "labels")
    if lwhere != where:
        raise ValueError("labels and power_or_entropy must be arrays of the same kind")
    if mode == 0:
        zk, zptr, zwhere = _as_f32(zcr, "zcr")
        if zwhere != where or int(np.prod(zk.shape)) < frame_seg.total:
            raise ValueError("zcr and power must be arrays of the same kind holding every frame of frame_seg")
        g, lo, hi = np.broadcast_arrays(*(np.asarray(v, dtype=np.float32) for v in (zcr_gate, ampl, amph)))
    else:
        zk, zptr = None, None
        lo = np.asarray(ampl, dtype=np.float32)
        g = hi = lo
    if int(np.prod(pk.shape)) < frame_seg.total or int(np.prod(lk.shape)) < frame_seg.total:
        raise ValueError("fewer values than frame_seg has frames")
    g, lo, hi = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (g, lo, hi))
    n_par = int(lo.shape[0])
    counts = ctx._empty((n_par, frame_seg.n, 3), where, "int32")
    ms = ctx._run(ctx._lib.ssp_vad_sweep, where, timing, ctx._h, zptr, pptr, lptr, frame_seg._h, int(mode), n_par,
                  g.ctypes.data if mode == 0 else None, lo.ctypes.data, hi.ctypes.data if mode == 0 else None, int(min_len),
                  _raw_ptr(counts, where), where)
    return (counts, ms) if timing else counts


def gmm_em_stats(ctx: "Context", weights, means, covars, feats, timing: bool = False) -> dict:
    """E step + M-step sums of ONE EM iteration of a diagonal GMM on the GPU (ssp_gmm_em_stats).
    weights (K,), means (K,D), covars (K,D) float64; feats (n, D) float32 (numpy or device tensor).
    Returns nk (K,), sx (K,D), sxx (K,D), loglik_sum (float) as float64."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    mu = np.ascontiguousarray(means, dtype=np.float64)
    cv = np.ascontiguousarray(covars, dtype=np.float64)
    if w.ndim != 1 or mu.ndim != 2 or mu.shape != cv.shape or mu.shape[0] != w.shape[0]:
        raise ValueError("expected weights (K,), means (K,D), covars (K,D)")
    K, D = mu.shape
    keep, ptr, where = _as_frames(feats, D)
    nk = np.empty(K, dtype=np.float64)
    sx = np.empty((K, D), dtype=np.float64)
    sxx = np.empty((K, D), dtype=np.float64)
    ll = C.c_double(0.0)
    ms = ctx._run(ctx._lib.ssp_gmm_em_stats, where, timing, ctx._h, K, D, w.ctypes.data, mu.ctypes.data, cv.ctypes.data, ptr, int(keep.shape[0]),
                  nk.ctypes.data, sx.ctypes.data, sxx.ctypes.data, C.byref(ll), where)
    return _result(timing, ms, nk=nk, sx=sx, sxx=sxx, loglik_sum=ll.value)


def gmm_em_stats_batch(ctx: "Context", weights, means, covars, feats, row_off, n_frames, timing: bool = False) -> dict:
    """gmm_em_stats for M models in one call (ssp_gmm_em_stats_batch): model m over rows [row_off[m], row_off[m] + n_frames[m]) of feats.
    weights (M,K), means (M,K,D), covars (M,K,D) float64; feats (n_rows, D) float32 (numpy or device tensor); row_off, n_frames (M,).
    Returns nk (M,K), sx (M,K,D), sxx (M,K,D), loglik_sum (M,) as float64; for K <= 64 each model's are the bits gmm_em_stats gives
    on its rows.  D > 47: NotImplementedError."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    mu = np.ascontiguousarray(means, dtype=np.float64)
    cv = np.ascontiguousarray(covars, dtype=np.float64)
    if w.ndim != 2 or mu.ndim != 3 or mu.shape != cv.shape or mu.shape[:2] != w.shape:
        raise ValueError("expected weights (M,K), means (M,K,D), covars (M,K,D)")
    M, K, D = mu.shape
    off = np.ascontiguousarray(row_off, dtype=np.int64)
    cnt = np.ascontiguousarray(n_frames, dtype=np.int64)
    if off.shape != (M,) or cnt.shape != (M,):
        raise ValueError("row_off and n_frames must be (%d,)" % M)
    keep, ptr, where = _as_frames(feats, D)
    nk = np.empty((M, K), dtype=np.float64)
    sx = np.empty((M, K, D), dtype=np.float64)
    sxx = np.empty((M, K, D), dtype=np.float64)
    ll = np.empty(M, dtype=np.float64)
    ms = ctx._run(ctx._lib.ssp_gmm_em_stats_batch, where, timing, ctx._h, M, K, D, w.ctypes.data, mu.ctypes.data, cv.ctypes.data, ptr,
                  int(keep.shape[0]), off.ctypes.data, cnt.ctypes.data, nk.ctypes.data, sx.ctypes.data, sxx.ctypes.data, ll.ctypes.data, where)
    return _result(timing, ms, nk=nk, sx=sx, sxx=sxx, loglik_sum=ll)


def gmm_em_stats_shared(ctx: "Context", weights, means, covars, feats, row_off, n_frames, timing: bool = False) -> dict:
    """The statistics of M row ranges of feats under ONE model (ssp_gmm_em_stats_shared): what MAP adaptation of a UBM needs per speaker.
    weights (K,), means (K,D), covars (K,D) float64 — packed and uploaded once; feats, row_off, n_frames and the result as
    gmm_em_stats_batch, whose bits (called with the parameters repeated M times) these are.  D > 47: NotImplementedError."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    mu = np.ascontiguousarray(means, dtype=np.float64)
    cv = np.ascontiguousarray(covars, dtype=np.float64)
    if w.ndim != 1 or mu.ndim != 2 or mu.shape != cv.shape or mu.shape[0] != w.shape[0]:
        raise ValueError("expected weights (K,), means (K,D), covars (K,D)")
    K, D = mu.shape
    off = np.ascontiguousarray(row_off, dtype=np.int64)
    cnt = np.ascontiguousarray(n_frames, dtype=np.int64)
    if off.ndim != 1 or off.shape != cnt.shape:
        raise ValueError("row_off and n_frames must be (M,)")
    M = int(off.shape[0])
    keep, ptr, where = _as_frames(feats, D)
    nk = np.empty((M, K), dtype=np.float64)
    sx = np.empty((M, K, D), dtype=np.float64)
    sxx = np.empty((M, K, D), dtype=np.float64)
    ll = np.empty(M, dtype=np.float64)
    ms = ctx._run(ctx._lib.ssp_gmm_em_stats_shared, where, timing, ctx._h, M, K, D, w.ctypes.data, mu.ctypes.data, cv.ctypes.data, ptr,
                  int(keep.shape[0]), off.ctypes.data, cnt.ctypes.data, nk.ctypes.data, sx.ctypes.data, sxx.ctypes.data, ll.ctypes.data, where)
    return _result(timing, ms, nk=nk, sx=sx, sxx=sxx, loglik_sum=ll)


GMM_FULL_MAX_D = 64  # ssp_gmm_full_em_stats / ssp_gmm_full_pack's feature dimension (include/ssp.h)


def gmm_full_em_stats(ctx: "Context", weights, means, prec_chol, feats, shift=None, timing: bool = False) -> dict:
    """E step + M-step sums of ONE EM iteration of a full-covariance GMM on the GPU (ssp_gmm_full_em_stats).
    weights (K,), means (K,D), prec_chol (K,D,D) float64 — sklearn's precisions_cholesky_, upper triangular; feats (n, D) float32 (numpy
    or device tensor); shift (D,) or None: the statistics are taken about it, x' = x - shift.
    Returns nk (K,), sx (K,D), sxx (K,D,D), loglik_sum (float) as float64."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    mu = np.ascontiguousarray(means, dtype=np.float64)
    pc = np.ascontiguousarray(prec_chol, dtype=np.float64)
    if w.ndim != 1 or mu.ndim != 2 or mu.shape[0] != w.shape[0] or pc.shape != mu.shape + mu.shape[1:]:
        raise ValueError("expected weights (K,), means (K,D), prec_chol (K,D,D)")
    K, D = mu.shape
    sh = None
    if shift is not None:
        sh = np.ascontiguousarray(shift, dtype=np.float64)
        if sh.shape != (D,):
            raise ValueError("shift must be (%d,)" % D)
    keep, ptr, where = _as_frames(feats, D)
    nk = np.empty(K, dtype=np.float64)
    sx = np.empty((K, D), dtype=np.float64)
    sxx = np.empty((K, D, D), dtype=np.float64)
    ll = C.c_double(0.0)
    ms = ctx._run(ctx._lib.ssp_gmm_full_em_stats, where, timing, ctx._h, K, D, w.ctypes.data, mu.ctypes.data, pc.ctypes.data,
                  _raw_ptr(sh, _lib.HOST), ptr, int(keep.shape[0]), nk.ctypes.data, sx.ctypes.data, sxx.ctypes.data,
                  C.byref(ll), where)
    return _result(timing, ms, nk=nk, sx=sx, sxx=sxx, loglik_sum=ll.value)


class GmmFullScorer(_Handle):
    """Packed full-covariance GMMs (ssp_gmm_full).  weights (M,K), means (M,K,D), prec_chol (M,K,D,D) float64 — sklearn's
    precisions_cholesky_ of covariance_type='full', upper triangular.  has_ubm: model 0 is the UBM; scores / argmax as GmmScorer's."""

    _DESTROY = "ssp_gmm_full_destroy"

    def __init__(self, ctx: Context, weights, means, prec_chol, has_ubm: bool = True):
        super().__init__(ctx)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        mu = np.ascontiguousarray(means, dtype=np.float64)
        pc = np.ascontiguousarray(prec_chol, dtype=np.float64)
        if w.ndim != 2 or mu.ndim != 3 or mu.shape[:2] != w.shape or pc.shape != mu.shape + mu.shape[2:]:
            raise ValueError("expected weights (M,K), means (M,K,D), prec_chol (M,K,D,D)")
        self.n_models, self.K, self.D = mu.shape
        self.has_ubm = bool(has_ubm)
        self._create(self._lib.ssp_gmm_full_pack, ctx._h, self.n_models, self.K, self.D, w.ctypes.data, mu.ctypes.data, pc.ctypes.data,
                     1 if has_ubm else 0)

    @classmethod
    def from_sklearn(cls, ctx: Context, models: Sequence, ubm=None) -> "GmmFullScorer":
        """models / ubm: fitted sklearn or gmm_train GaussianMixture(covariance_type='full') objects (duck-typed: weights_, means_,
        precisions_cholesky_), all with the same K and D."""
        allm = ([ubm] if ubm is not None else []) + list(models)
        for g in allm:
            if getattr(g, "covariance_type", "full") != "full" or np.ndim(g.precisions_cholesky_) != 3:
                raise ValueError("only covariance_type='full' models are supported here (GmmScorer takes 'diag' models)")
        return cls(ctx, np.stack([g.weights_ for g in allm]), np.stack([g.means_ for g in allm]),
                   np.stack([g.precisions_cholesky_ for g in allm]), has_ubm=ubm is not None)

    def score(self, feats, frame_seg: Segments, loglik: bool = False, scores: bool = True, argmax: bool = True, timing: bool = False) -> dict:
        """Returns a dict with the requested arrays: loglik (M, F) per-frame log-likelihood per model (= score_samples), scores (U, M)
        mean log-likelihood (= GaussianMixture.score), argmax (U,) int32 over speaker models of score - score_ubm."""
        keep, ptr, where = _as_frames(feats, self.D, frame_seg)
        F, U = frame_seg.total, frame_seg.n
        ll = self.ctx._empty((self.n_models, F), where) if loglik else None
        sc = self.ctx._empty((U, self.n_models), where) if scores else None
        am = self.ctx._empty((U,), where, "int32") if argmax else None
        ms = self.ctx._run(self._lib.ssp_gmm_full_score, where, timing, self._h, ptr, frame_seg._h, _raw_ptr(ll, where), _raw_ptr(sc, where),
                           _raw_ptr(am, where), where)
        return _result(timing, ms, loglik=ll, scores=sc, argmax=am)

    def score_list(self, feats_list, timing: bool = False) -> dict:
        """score() on a list of (T_j, D) feature matrices, stacked on the host (not the hot path): scores (U, M) and argmax (U,)."""
        mats = [np.asarray(a, dtype=np.float32) for a in feats_list]
        for a in mats:
            if a.ndim != 2 or a.shape[1] != self.D:
                raise ValueError("every feature matrix must be (frames, %d)" % self.D)
        fseg = Segments.from_lengths(self.ctx, [a.shape[0] for a in mats])
        X = np.ascontiguousarray(np.concatenate(mats)) if mats else np.zeros((0, self.D), np.float32)
        return self.score(X, fseg, loglik=False, scores=True, argmax=True, timing=timing)


KMEANSPP_MAX_D = 64  # ssp_kmeanspp_seed's feature dimension (include/ssp.h)


def kmeanspp_candidates(K: int) -> int:
    """candidates per k-means++ step: 2 + int(ln K) (sklearn's kmeans_plusplus; the last axis of ``u`` in kmeanspp_seeds)"""
    return 2 + int(np.log(K))


def kmeanspp_seeds(ctx: "Context", feats, K, first, u, row_off=None, n_sel=None, sel=None, centres=True, timing=False) -> dict:
    """k-means++ seeds of P problems in one launch, the random numbers handed in (ssp_kmeanspp_seed).
    feats (n_rows, D) float32, numpy or device tensor.  Problem p: rows [row_off[p], row_off[p] + n_sel[p]) of feats, or — with ``sel``, the
    concatenated sorted row lists — the rows sel[row_off[p] : row_off[p] + n_sel[p]]; with neither, ONE problem over every row.  first
    (P,): position of the first centre among the problem's rows; u (P, K-1, 2 + int(ln K)) uniforms in [0, 1).
    Returns rows (P, K) int64, absolute row numbers of feats, and centres (P, K, D) float64 unless centres=False
    [and kernel_ms when timing=True].  D > 64: NotImplementedError."""
    keep, ptr, where = _as_f32(feats, "feats")
    if keep.ndim != 2:
        raise ValueError("feats must be (rows, D)")
    n_rows, D = int(keep.shape[0]), int(keep.shape[1])
    K = int(K)
    fi = np.ascontiguousarray(first, dtype=np.int64).reshape(-1)
    P = int(fi.shape[0])
    if row_off is None and n_sel is None:
        if P != 1:
            raise ValueError("row_off and n_sel are needed for more than one problem")
        off = np.zeros(1, dtype=np.int64)
        cnt = np.array([n_rows if sel is None else np.size(sel)], dtype=np.int64)
    elif row_off is None or n_sel is None:
        raise ValueError("row_off and n_sel come together")
    else:
        off = np.ascontiguousarray(row_off, dtype=np.int64).reshape(-1)
        cnt = np.ascontiguousarray(n_sel, dtype=np.int64).reshape(-1)
    if off.shape != (P,) or cnt.shape != (P,):
        raise ValueError("row_off, n_sel and first must be (%d,)" % P)
    L = kmeanspp_candidates(K) if K >= 1 else 2
    uu = np.ascontiguousarray(u, dtype=np.float64)
    if uu.size != P * max(K - 1, 0) * L:
        raise ValueError("u must be (%d, %d, %d)" % (P, K - 1, L))
    sl = None
    if sel is not None:
        sl = np.ascontiguousarray(sel, dtype=np.int64).reshape(-1)
        if P and cnt.min(initial=1) >= 0 and off.min(initial=0) >= 0 and int((off + cnt).max(initial=0)) > sl.shape[0]:
            raise ValueError("sel is shorter than row_off + n_sel asks for")
    rows = np.empty((P, max(K, 0)), dtype=np.int64)
    cen = np.empty((P, max(K, 0), D), dtype=np.float64) if centres else None
    ms = ctx._run(ctx._lib.ssp_kmeanspp_seed, where, timing, ctx._h, P, K, D, ptr, n_rows, where, off.ctypes.data, cnt.ctypes.data,
                  _raw_ptr(sl, _lib.HOST), fi.ctypes.data, uu.ctypes.data if uu.size else None, rows.ctypes.data, _raw_ptr(cen, _lib.HOST))
    return _result(timing, ms, rows=rows, centres=cen)


class GmmScorer(_Handle):
    """Packed diagonal GMMs (ssp_gmm).  weights (M,K), means (M,K,D), covars (M,K,D) float64.
    has_ubm: model 0 is the UBM (GMM_UBM.py:169-170); scores/argmax are then taken against it."""

    _DESTROY = "ssp_gmm_destroy"

    def __init__(self, ctx: Context, weights, means, covars, has_ubm: bool = True):
        super().__init__(ctx)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        mu = np.ascontiguousarray(means, dtype=np.float64)
        cv = np.ascontiguousarray(covars, dtype=np.float64)
        if w.ndim != 2 or mu.ndim != 3 or mu.shape != cv.shape or mu.shape[:2] != w.shape:
            raise ValueError("expected weights (M,K), means (M,K,D), covars (M,K,D)")
        self.n_models, self.K, self.D = mu.shape
        self.has_ubm = bool(has_ubm)
        self._create(self._lib.ssp_gmm_pack, ctx._h, self.n_models, self.K, self.D, w.ctypes.data, mu.ctypes.data, cv.ctypes.data,
                     1 if has_ubm else 0)

    @classmethod
    def from_sklearn(cls, ctx: Context, models: Sequence, ubm=None) -> "GmmScorer":
        """models / ubm: fitted sklearn GaussianMixture(covariance_type='diag') objects (duck-typed:
        weights_, means_, covariances_), all with the same K and D — the lists GMM_UBM.py:141-146 pickles."""
        allm = ([ubm] if ubm is not None else []) + list(models)
        for g in allm:
            if getattr(g, "covariance_type", "diag") != "diag":
                raise ValueError("only covariance_type='diag' models are supported here (GmmFullScorer takes 'full' models)")
        return cls(ctx, np.stack([g.weights_ for g in allm]), np.stack([g.means_ for g in allm]),
                   np.stack([g.covariances_ for g in allm]), has_ubm=ubm is not None)

    def score(self, feats, frame_seg: Segments, loglik: bool = False, scores: bool = True, argmax: bool = True,
              precision: int = 0, timing: bool = False) -> dict:
        """Returns a dict with the requested arrays:
        loglik (M, F) per-frame log-likelihood per model (= score_samples), scores (U, M) mean log-likelihood
        (= GaussianMixture.score), argmax (U,) int32 over speaker models of score - score_ubm.
        precision: 0 exact-fp32 MFMA | 1 bf16x3 split MFMA with the close calls (top-2 margin inside the split-precision error
        BOUND) scored again in fp32, so the arg-max equals precision 0's (``last_rescored`` = how many) | 2 bf16x3 alone | 3 as 1
        with the calibrated, heuristic band (about 100 times narrower than the bound: far fewer utterances scored twice) | 4 or
        "auto": precision 1's guarantee at the cost of the cheaper of 1 and 0 — a pilot on the first ~2 % of the utterances prices the
        re-scoring; ``last_auto`` says what it chose (include/ssp.h, ssp_gmm_score)."""
        if precision == "auto":
            precision = 4
        keep, ptr, where = _as_frames(feats, self.D, frame_seg)
        F, U = frame_seg.total, frame_seg.n
        ll = self.ctx._empty((self.n_models, F), where) if loglik else None
        sc = self.ctx._empty((U, self.n_models), where) if scores else None
        am = self.ctx._empty((U,), where, "int32") if argmax else None
        ms = self.ctx._run(self._lib.ssp_gmm_score, where, timing, self._h, ptr, frame_seg._h, _raw_ptr(ll, where), _raw_ptr(sc, where),
                           _raw_ptr(am, where), where, int(precision))
        return _result(timing, ms, loglik=ll, scores=sc, argmax=am)

    def score_list(self, feats_list, precision: int = 0, timing: bool = False) -> dict:
        """score() on a list of (T_j, D) feature matrices without stacking them on the host (ssp_gmm_score_list: the rows are gathered
        and narrowed to float32 into pinned memory by worker threads): the same bits as score(np.vstack(feats_list).astype(float32),
        ...) with scores=True, argmax=True.  Returns a dict with scores (U, M) and argmax (U,) [and kernel_ms]."""
        if precision == "auto":
            precision = 4
        table, keep, typ = list_table(feats_list, "rows")
        for a in keep:
            if a.ndim != 2 or a.shape[1] != self.D:
                raise ValueError("every feature matrix must be (frames, %d)" % self.D)
        fseg = Segments.from_lengths(self.ctx, [a.shape[0] for a in keep])
        sc = np.empty((fseg.n, self.n_models), dtype=np.float32)
        am = np.empty((fseg.n,), dtype=np.int32)
        ms = self.ctx._run(self._lib.ssp_gmm_score_list, _lib.HOST, timing, self._h, table.ctypes.data if table.size else None, typ, self.D,
                           fseg._h, sc.ctypes.data, am.ctypes.data, int(precision))   # (keep owns what the table points into)
        return _result(timing, ms, scores=sc, argmax=am)

    @property
    def last_rescored(self) -> int:
        return _read_int(C.c_int32, self._lib.ssp_gmm_last_rescored, self._h)

    @property
    def last_auto(self) -> dict:
        """what the last precision = "auto" call chose and what its pilot saw (precision_used -1: no such call yet)"""
        a, b, c, f = C.c_int32(-1), C.c_int32(0), C.c_int32(0), C.c_float(0.0)
        _lib.check(self._lib.ssp_gmm_last_auto(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(f)))
        return {"precision_used": a.value, "pilot_utterances": b.value, "pilot_listed": c.value, "predicted_cost_of_precision_1": f.value}


MAP_MAX_C = 8   # ssp_gmm_map_score's largest top-C (include/ssp.h)
MAP_MAX_D = 47  # ... and feature dimension


class MapScorer(_Handle):
    """Top-C fast scorer of mean-adapted GMM-UBM speaker models (ssp_gmm_map; an extension the reference does not have).
    ubm_w (K,), ubm_mu (K,D), ubm_cv (K,D), spk_means (S,K,D) float64: speaker s is the UBM with its means replaced by spk_means[s].
    Per utterance: diff[u, s] = mean_t (L_s(x_t) - L_ubm(x_t)) over the UBM's best ``top_c`` mixtures of every frame — with top_c = K the
    dense models[s].score(x) - ubm.score(x) of GMM_UBM.py:185."""

    _DESTROY = "ssp_gmm_map_destroy"

    def __init__(self, ctx: Context, ubm_w, ubm_mu, ubm_cv, spk_means):
        super().__init__(ctx)
        w = np.ascontiguousarray(ubm_w, dtype=np.float64)
        mu = np.ascontiguousarray(ubm_mu, dtype=np.float64)
        cv = np.ascontiguousarray(ubm_cv, dtype=np.float64)
        sm = np.ascontiguousarray(spk_means, dtype=np.float64)
        if w.ndim != 1 or mu.ndim != 2 or mu.shape != cv.shape or mu.shape[0] != w.shape[0] or sm.ndim != 3 or sm.shape[1:] != mu.shape:
            raise ValueError("expected ubm_w (K,), ubm_mu (K,D), ubm_cv (K,D), spk_means (S,K,D)")
        self.K, self.D = mu.shape
        self.S = int(sm.shape[0])
        self._create(self._lib.ssp_gmm_map_pack, ctx._h, self.K, self.D, w.ctypes.data, mu.ctypes.data, cv.ctypes.data, self.S, sm.ctypes.data)

    @classmethod
    def from_sklearn(cls, ctx: Context, models: Sequence, ubm) -> "MapScorer":
        """models: mean-adapted speaker models (gmm_train.map_adapt(ubm, Xs, adapt='m')), ubm: the fitted UBM they were adapted from.
        ValueError naming the first model whose weights_ or covariances_ are not element for element the UBM's."""
        uw, ucv = np.asarray(ubm.weights_), np.asarray(ubm.covariances_)
        for i, g in enumerate(models):
            if getattr(g, "covariance_type", "diag") != "diag":
                raise ValueError("only covariance_type='diag' models are supported (top-C scoring of 'full' models is not built)")
            for name, ref in (("weights_", uw), ("covariances_", ucv)):
                v = np.asarray(getattr(g, name))
                if v.shape != ref.shape or not np.array_equal(v, ref):
                    raise ValueError("model %d: %s differ from the UBM's: the top-C scorer takes mean-adapted models only "
                                     "(map_adapt(..., adapt='m'))" % (i, name))
        return cls(ctx, uw, ubm.means_, ucv, np.stack([g.means_ for g in models]))

    def score(self, feats, frame_seg: Segments, top_c: int = 5, diff: bool = True, ubm: bool = False, argmax: bool = True, idx: bool = False,
              timing: bool = False) -> dict:
        """Returns a dict with the requested arrays: diff (U, S) float32, ubm (U,) float32 = mean_t L_ubm, argmax (U,) int32 (first index
        of the row's maximum), idx (F, top_c) int32: the selected mixtures of every frame in rank order (-1: a non-finite frame).  A
        non-finite frame or an empty utterance: a NaN diff row, NaN ubm, arg-max 0 (include/ssp.h, ssp_gmm_map_score)."""
        keep, ptr, where = _as_frames(feats, self.D, frame_seg)
        F, U, Ck = frame_seg.total, frame_seg.n, int(top_c)
        df = self.ctx._empty((U, self.S), where) if diff else None
        ub = self.ctx._empty((U,), where) if ubm else None
        am = self.ctx._empty((U,), where, "int32") if argmax else None
        ix = self.ctx._empty((F, max(Ck, 0)), where, "int32") if idx else None
        ms = self.ctx._run(self._lib.ssp_gmm_map_score, where, timing, self._h, ptr, frame_seg._h, Ck, _raw_ptr(df, where), _raw_ptr(ub, where),
                           _raw_ptr(am, where), _raw_ptr(ix, where), where)
        return _result(timing, ms, diff=df, ubm=ub, argmax=am, idx=ix)

    def score_list(self, feats_list, top_c: int = 5, timing: bool = False) -> dict:
        """score() on a list of (T_j, D) feature matrices without stacking them on the host (ssp_gmm_map_score_list: GmmScorer.score_list's
        gather): the bits of score(np.vstack(feats_list).astype(float32), ...).  Returns diff (U, S), ubm (U,), argmax (U,)."""
        table, keep, typ = list_table(feats_list, "rows")
        for a in keep:
            if a.ndim != 2 or a.shape[1] != self.D:
                raise ValueError("every feature matrix must be (frames, %d)" % self.D)
        fseg = Segments.from_lengths(self.ctx, [a.shape[0] for a in keep])
        df = np.empty((fseg.n, self.S), dtype=np.float32)
        ub = np.empty((fseg.n,), dtype=np.float32)
        am = np.empty((fseg.n,), dtype=np.int32)
        ms = self.ctx._run(self._lib.ssp_gmm_map_score_list, _lib.HOST, timing, self._h, table.ctypes.data if table.size else None, typ, self.D,
                           fseg._h, int(top_c), df.ctypes.data, ub.ctypes.data, am.ctypes.data, None)   # (keep owns what the table points into)
        return _result(timing, ms, diff=df, ubm=ub, argmax=am)


IVECTOR_MAX_R = 256  # ssp_ivector_create's largest rank (include/ssp.h)
IVECTOR_STAGES = ("gemm_L", "gemm_b", "cholesky", "gemm_A", "gemm_C")  # ssp_ivector_last_stages


class IvectorExtractor(_Handle):
    """i-vector extraction and the E-step of total-variability training (ssp_ivector; an extension the reference does not have).
    ubm_mu (K,D), ubm_cv (K,D), T (K,D,R) float64.  Statistics nk (U,K), sx (U,K,D) float64 on the host, as gmm_em_stats_shared returns
    them; include/ssp.h has the definitions."""

    _DESTROY = "ssp_ivector_destroy"

    def __init__(self, ctx: Context, ubm_mu, ubm_cv, T):
        mu = np.ascontiguousarray(ubm_mu, dtype=np.float64)
        cv = np.ascontiguousarray(ubm_cv, dtype=np.float64)
        T = np.ascontiguousarray(T, dtype=np.float64)
        if mu.ndim != 2 or mu.shape != cv.shape or T.ndim != 3 or T.shape[:2] != mu.shape:
            raise ValueError("expected ubm_mu (K,D), ubm_cv (K,D), T (K,D,R)")
        self.K, self.D = mu.shape
        self.R = int(T.shape[2])
        if self.R < 1:
            raise ValueError("T (K,D,R): the rank R must be at least 1")
        if self.R > IVECTOR_MAX_R:
            raise NotImplementedError("R=%d exceeds the supported rank (%d)" % (self.R, IVECTOR_MAX_R))
        super().__init__(ctx)
        self._create(self._lib.ssp_ivector_create, ctx._h, self.K, self.D, self.R, mu.ctypes.data, cv.ctypes.data, T.ctypes.data)

    def set_T(self, T) -> "IvectorExtractor":
        """replace T (K,D,R): P and G are packed again on the device"""
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.shape != (self.K, self.D, self.R):
            raise ValueError("T must be (%d, %d, %d)" % (self.K, self.D, self.R))
        _lib.check(self._lib.ssp_ivector_set_t(self._h, T.ctypes.data))
        return self

    def set_workspace(self, nbytes: int) -> "IvectorExtractor":
        """cap of the workspace that grows with the slab; larger batches run in slabs of whole utterances (same bits per utterance)"""
        _lib.check(self._lib.ssp_ivector_set_workspace(self._h, C.c_size_t(int(nbytes))))
        return self

    @property
    def last_slab(self) -> int:
        return _read_int(C.c_int64, self._lib.ssp_ivector_last_slab, self._h)

    @property
    def last_stages(self) -> dict:
        """device milliseconds per stage of the last call made with timing=True"""
        ms = (C.c_float * len(IVECTOR_STAGES))()
        _lib.check(self._lib.ssp_ivector_last_stages(self._h, ms))
        return dict(zip(IVECTOR_STAGES, [float(v) for v in ms]))

    def _stats(self, nk, sx, check):
        nk = np.ascontiguousarray(nk, dtype=np.float64)
        sx = np.ascontiguousarray(sx, dtype=np.float64)
        if nk.ndim != 2 or nk.shape[1] != self.K or sx.shape != (nk.shape[0], self.K, self.D):
            raise ValueError("expected nk (U, %d) and sx (U, %d, %d)" % (self.K, self.K, self.D))
        if nk.shape[0] < 1:
            raise ValueError("at least one utterance is needed")
        if check:
            ok = np.isfinite(nk).all(axis=1) & np.isfinite(sx).all(axis=(1, 2))
            if not ok.all():
                raise ValueError("the statistics of utterance %d contain NaN or infinity" % int(np.argmin(ok)))
        return nk, sx

    def extract(self, nk, sx, logdet: bool = False, quad: bool = False, timing: bool = False, check: bool = True):
        """-> w (U, R) float32, or a dict with "w" and the requested "logdet" / "quad" (U,) [and "kernel_ms"].  ValueError names the first
        utterance with a non-finite statistic; check=False hands such a batch to the library, which answers that utterance with NaN."""
        nk, sx = self._stats(nk, sx, check)
        U = int(nk.shape[0])
        w = np.empty((U, self.R), dtype=np.float32)
        ld = np.empty(U, dtype=np.float32) if logdet else None
        qd = np.empty(U, dtype=np.float32) if quad else None
        ms = self.ctx._run(self._lib.ssp_ivector_extract, _lib.HOST, timing, self._h, nk.ctypes.data, sx.ctypes.data, U, w.ctypes.data,
                           _raw_ptr(ld, _lib.HOST), _raw_ptr(qd, _lib.HOST))
        if not (logdet or quad or timing):
            return w
        return _result(timing, ms, w=w, logdet=ld, quad=qd)

    def estep(self, nk, sx, timing: bool = False, check: bool = True) -> dict:
        """-> {"A" (K,R,R), "C" (K,D,R), "objective"} float64 [and "kernel_ms"]: the accumulators of one EM iteration under the current T"""
        nk, sx = self._stats(nk, sx, check)
        U = int(nk.shape[0])
        A = np.empty((self.K, self.R, self.R), dtype=np.float64)
        Cm = np.empty((self.K, self.D, self.R), dtype=np.float64)
        obj = C.c_double(0.0)
        ms = self.ctx._run(self._lib.ssp_ivector_estep, _lib.HOST, timing, self._h, nk.ctypes.data, sx.ctypes.data, U, A.ctypes.data, Cm.ctypes.data,
                           C.byref(obj))
        return _result(timing, ms, A=A, C=Cm, objective=obj.value)


PLDA_MAX_Q = 256  # largest dimension of ssp_plda_stats / ssp_plda_pack (include/ssp.h)
PLDA_NO_CLASS_PATH = _lib.PLDA_NO_CLASS_PATH  # PldaScorer flags bit 0: never use the class-shared path of the t^2 term


def _as_labels(labels, where, n):
    """-> (int32 array kept alive, raw address) on the side ``where`` names; one label per row"""
    if where == _lib.DEVICE:
        import torch
        if not _is_torch(labels):
            labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int32), device="cuda")
        lab = labels.to(torch.int32).contiguous()
        ptr = lab.data_ptr()
    else:
        lab = np.ascontiguousarray(labels.cpu().numpy() if _is_torch(labels) else labels, dtype=np.int32)
        ptr = lab.ctypes.data
    if lab.ndim != 1 or int(lab.shape[0]) != n:
        raise ValueError("one label per row of X")
    return lab, ptr


def plda_stats(ctx: Context, X, labels, S: int, timing: bool = False) -> dict:
    """Class statistics for PLDA / LDA training (ssp_plda_stats; include/ssp.h has the definitions).  X (N, q) numpy or torch CUDA
    tensor, labels (N,) in [0, S).  Returns HOST arrays: "sum" (S, q) float64 (row order), "count" (S,) int64, "mean" (q,) float64 (of
    all rows), "sw" (q, q) float64, exactly symmetric.  ValueError for a label outside [0, S); q > 256: NotImplementedError.  A
    non-finite row makes the outputs non-finite (plda.class_stats names the row)."""
    keep, ptr, where = _as_f32(X, "X")
    if keep.ndim != 2:
        raise ValueError("X must be (N, q)")
    N, q, S = int(keep.shape[0]), int(keep.shape[1]), int(S)
    lab, lptr = _as_labels(labels, where, N)
    sm = np.zeros((max(S, 0), q), dtype=np.float64)
    cnt = np.zeros(max(S, 0), dtype=np.int64)
    mean = np.zeros(q, dtype=np.float64)
    sw = np.zeros((q, q), dtype=np.float64)
    ms = ctx._run(ctx._lib.ssp_plda_stats, where, timing, ctx._h, ptr, lptr, N, q, S, sm.ctypes.data, cnt.ctypes.data, mean.ctypes.data,
                  sw.ctypes.data, where)
    return _result(timing, ms, sum=sm, count=cnt, mean=mean, sw=sw)


class PldaScorer(_Handle):
    """Enrolled speakers of a diagonalised PLDA model packed for the log-likelihood-ratio sweep (ssp_plda; an extension the reference
    does not have).  psi (q,) float64 >= 0, enrol_mean (S, q) float64 ALREADY transformed by A (the mean of each speaker's transformed
    enrolment vectors), enrol_count (S,) >= 1.  flags: PLDA_NO_CLASS_PATH keeps the t^2 term off the class-shared path."""

    _DESTROY = "ssp_plda_destroy"

    def __init__(self, ctx: Context, psi, enrol_mean, enrol_count, flags: int = 0):
        super().__init__(ctx)
        psi = np.ascontiguousarray(psi, dtype=np.float64)
        em = np.ascontiguousarray(enrol_mean, dtype=np.float64)
        ec = np.ascontiguousarray(enrol_count, dtype=np.int32)
        if psi.ndim != 1 or em.ndim != 2 or em.shape[1] != psi.shape[0] or ec.shape != (em.shape[0],):
            raise ValueError("expected psi (q,), enrol_mean (S, q), enrol_count (S,)")
        self.q, self.S = int(psi.shape[0]), int(em.shape[0])
        self._create(self._lib.ssp_plda_pack, ctx._h, self.q, psi.ctypes.data, self.S, em.ctypes.data, ec.ctypes.data, int(flags))
        g, shared = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.ssp_plda_info(self._h, C.byref(g), C.byref(shared)))   # what the pack decided, from the handle
        self.n_classes, self.class_shared = g.value, bool(shared.value)

    def score(self, T, llr: bool = False, argmax: bool = True, maxval: bool = True, timing: bool = False) -> dict:
        """T (N, q) ALREADY transformed, numpy or torch CUDA tensor.  Returns a dict of the same kind of arrays: "argmax" (N,) int32 (first
        index of the row's maximum; -1 for a non-finite test vector), "max" (N,) float32 = llr[argmax] and, with llr=True, "llr" (N, S)
        float32.  A device call returns without a host wait."""
        keep, ptr, where = _as_f32(T, "T")
        if keep.ndim != 2 or keep.shape[1] != self.q:
            raise ValueError("T must be (N, %d)" % self.q)
        N = int(keep.shape[0])
        lr = self.ctx._empty((N, self.S), where) if llr else None
        am = self.ctx._empty((N,), where, "int32") if argmax else None
        mx = self.ctx._empty((N,), where) if maxval else None
        ms = self.ctx._run(self._lib.ssp_plda_score, where, timing, self._h, ptr, N, _raw_ptr(lr, where), _raw_ptr(am, where), _raw_ptr(mx, where),
                           where)
        return _result(timing, ms, argmax=am, max=mx, llr=lr)


TOPN_MAX_LINE = 65536  # longest line of ssp_topn_stats (include/ssp.h)
DET_MAX_THRESHOLDS = 4096  # most thresholds of ssp_det_counts


def _as_matrix(x, name):
    """-> (array kept alive, raw address, where, leading dimension) of a 2-D float32 matrix.  A view whose rows are contiguous and at
    least one row apart (a column slice of a wider matrix) is passed as it is, with its row stride as the leading dimension."""
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("%s must be a matrix" % name)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    if _is_torch(x):
        import torch
        if x.is_cuda and x.dtype == torch.float32 and cols >= 1 and x.stride(1) == 1 and (rows <= 1 or x.stride(0) >= cols):
            return x, x.data_ptr(), _lib.DEVICE, (int(x.stride(0)) if rows > 1 else cols)
    elif isinstance(x, np.ndarray) and x.dtype == np.float32 and cols >= 1 and x.strides[1] == 4 and (
            rows <= 1 or (x.strides[0] >= 4 * cols and x.strides[0] % 4 == 0)):
        return x, x.ctypes.data, _lib.HOST, (x.strides[0] // 4 if rows > 1 else cols)
    keep, ptr, where = _as_f32(x, name)
    return keep, ptr, where, max(cols, 1)


def _as_vector(x, name, n, where):
    """-> (float32 array kept alive, raw address) of n entries on the side ``where`` names"""
    keep, ptr, w = _as_f32(x, name)
    if w != where:
        raise ValueError("%s must live where the scores live (numpy with numpy, torch CUDA with torch CUDA)" % name)
    if keep.ndim != 1 or int(keep.shape[0]) != n:
        raise ValueError("%s must have %d entries" % (name, n))
    return keep, ptr


def topn_stats(ctx: Context, scores, n: int, axis: int = 1, timing: bool = False) -> dict:
    """Mean, population deviation and smallest member of the ``n`` largest entries of every row (axis=1) or column (axis=0) of a score
    matrix (ssp_topn_stats; include/ssp.h has the definitions): the cohort statistics of adaptive score normalisation.  scores (rows,
    cols) numpy or torch CUDA tensor (a row-strided view is read in place).  Returns "mean", "std", "kth", float32, one entry per line,
    of the same kind of array.  A line with a non-finite entry gives NaN.  A device call returns without a host wait."""
    keep, ptr, where, ld = _as_matrix(scores, "scores")
    rows, cols = int(keep.shape[0]), int(keep.shape[1])
    lines = rows if axis == 1 else cols
    out = [ctx._empty((max(lines, 0),), where) for _ in range(3)]
    ms = ctx._run(ctx._lib.ssp_topn_stats, where, timing, ctx._h, ptr, rows, cols, ld, int(axis), int(n), *[_raw_ptr(o, where) for o in out], where)
    return _result(timing, ms, mean=out[0], std=out[1], kth=out[2])


def snorm_apply(ctx: Context, scores, row_mean=None, row_std=None, col_mean=None, col_std=None, std_floor: float = 1e-6, out=True,
                argmax: bool = True, maxval: bool = True, timing: bool = False) -> dict:
    """z = 0.5 ((x - col_mean) / max(col_std, floor) + (x - row_mean) / max(row_std, floor)) and its row-wise decision (ssp_snorm_apply).
    Row statistics alone give T-norm, column statistics alone Z-norm (no 0.5 then).  out: True — a new matrix; False — no matrix, only
    the decision; a float32 matrix of scores' kind and shape — written in place (``scores`` itself is allowed).  Returns {"argmax" (N,)
    int32 over the entries that are not NaN, first index on ties, -1 for none; "max" (N,) = z[argmax]; "scores" (N, S)}."""
    keep, ptr, where, ld = _as_matrix(scores, "scores")
    N, S = int(keep.shape[0]), int(keep.shape[1])
    if (row_mean is None) != (row_std is None) or (col_mean is None) != (col_std is None):
        raise ValueError("a mean needs its deviation")
    rm = rs = cm = cs = (None, None)
    if row_mean is not None:
        rm, rs = _as_vector(row_mean, "row_mean", N, where), _as_vector(row_std, "row_std", N, where)
    if col_mean is not None:
        cm, cs = _as_vector(col_mean, "col_mean", S, where), _as_vector(col_std, "col_std", S, where)
    z, zp, ldz = None, None, S
    if out is True:
        z = ctx._empty((N, S), where)
        zp = _raw_ptr(z, where)
    elif out is not False and out is not None:
        z, zp, zwhere, ldz = _as_matrix(out, "out")
        if z is not out or zwhere != where or tuple(z.shape) != (N, S):
            raise ValueError("out must be a float32 matrix of scores' shape and kind with contiguous rows")
    am = ctx._empty((N,), where, "int32") if argmax else None
    mx = ctx._empty((N,), where) if maxval else None
    ms = ctx._run(ctx._lib.ssp_snorm_apply, where, timing, ctx._h, ptr, N, S, ld, rm[1], rs[1], cm[1], cs[1], float(std_floor), zp, ldz,
                  _raw_ptr(am, where), _raw_ptr(mx, where), where)
    return _result(timing, ms, argmax=am, max=mx, scores=z)


def det_counts(ctx: Context, scores, target, thresholds=(), timing: bool = False) -> dict:
    """Target and non-target trials per threshold bin (ssp_det_counts): scores (N, S) numpy or torch CUDA tensor, target (N,) the enrolled
    speaker each row belongs to (-1: none), thresholds ascending float32, at most 4096 (none: totals and ranges only).  Returns HOST
    arrays: "tar_hist" / "non_hist" (M + 1,) int64 with bin = searchsorted(thresholds, x, "right"), "nan_count" (2,) int64, "range" (4,)
    float32 (min, max of the target scores, then of the non-target scores) and "thresholds".  ValueError for a target outside [-1, S)."""
    keep, ptr, where, ld = _as_matrix(scores, "scores")
    N, S = int(keep.shape[0]), int(keep.shape[1])
    lab, lptr = _as_labels(target, where, N)
    th = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
    M = int(th.shape[0])
    tar, non = np.zeros(M + 1, dtype=np.int64), np.zeros(M + 1, dtype=np.int64)
    nan, rng = np.zeros(2, dtype=np.int64), np.zeros(4, dtype=np.float32)
    ms = ctx._run(ctx._lib.ssp_det_counts, where, timing, ctx._h, ptr, N, S, ld, lptr, th.ctypes.data, M, tar.ctypes.data, non.ctypes.data,
                  nan.ctypes.data, rng.ctypes.data, where)
    return _result(timing, ms, tar_hist=tar, non_hist=non, nan_count=nan, range=rng, thresholds=th)


PAIRWISE_MAX_Q = 1024   # largest dimension of ssp_pairwise_scores (include/ssp.h)
AHC_MAX_SEGMENTS = 4096  # most segments of one recording (ssp_pairwise_scores, ssp_ahc_cluster)
AHC_N_LDS = 192          # recordings up to this many segments are clustered in LDS, longer ones in the context's workspace
AHC_LINKAGES = {"average": 0, "complete": 1, "single": 2}


def _as_recordings(ctx: Context, seg_or_counts) -> Segments:
    """a Segments object as it is, anything else as the segments per recording"""
    if isinstance(seg_or_counts, Segments):
        return seg_or_counts
    counts = np.asarray(seg_or_counts, dtype=np.int64).reshape(-1)
    if counts.size and counts.min() < 0:
        raise ValueError("a recording with a negative number of segments")
    return Segments.from_lengths(ctx, counts)


def pairwise_size(seg: Segments) -> int:
    """sum of n_r^2 over the recordings (ssp_pairwise_size): the floats of a packed batch of score matrices"""
    return _read_int(C.c_int64, seg._lib.ssp_pairwise_size, seg._h)


def pairwise_offsets(seg: Segments) -> np.ndarray:
    """int64[R + 1]: float offset of every recording's block in a packed batch of score matrices"""
    n = np.diff(seg.offsets)
    out = np.zeros(seg.n + 1, dtype=np.int64)
    np.cumsum(n * n, out=out[1:])
    return out


def pairwise_scores(ctx: Context, X, seg_or_counts, g=None, h=None, c0: float = 0.0, out=None, timing: bool = False):
    """S[i,j] = sum_d g_d x_id x_jd - (r_i + r_j) + c0, r_i = sum_d h_d x_id^2, for every pair of rows of the same recording
    (ssp_pairwise_scores; include/ssp.h has the definition).  X (total, q) numpy or torch CUDA tensor; seg_or_counts a Segments object
    or the rows per recording; g, h host vectors of q entries (None: ones / zeros): g = h = None on L2-normalised rows is the cosine,
    plda.Plda.pairwise_coeffs() gives the PLDA log-likelihood ratio.  Returns the packed blocks as one flat float32 array of X's kind
    (recording r's n_r x n_r block at pairwise_offsets(seg)[r]); out: such an array to write into.  A device call given a Segments
    object returns without a host wait (counts make one per call, which uploads and waits)."""
    keep, ptr, where = _as_f32(X, "X")
    if keep.ndim != 2:
        raise ValueError("X must be (total, q)")
    seg = _as_recordings(ctx, seg_or_counts)
    q = int(keep.shape[1])
    if int(keep.shape[0]) != seg.total:
        raise ValueError("X has %d rows, the recordings %d" % (int(keep.shape[0]), seg.total))
    vec = []
    for name, v in (("g", g), ("h", h)):
        if v is None:
            vec.append(None)
            continue
        v = np.ascontiguousarray(v.cpu().numpy() if _is_torch(v) else v, dtype=np.float32).reshape(-1)
        if v.shape[0] != q:
            raise ValueError("%s must have %d entries" % (name, q))
        vec.append(v)
    total = pairwise_size(seg)
    if out is None:
        out = ctx._empty((total,), where)
    else:
        ok = (_is_torch(out) and where == _lib.DEVICE and out.is_cuda and str(out.dtype) == "torch.float32" and out.is_contiguous()) or (
            isinstance(out, np.ndarray) and where == _lib.HOST and out.dtype == np.float32 and out.flags.c_contiguous)
        if not ok or int(np.prod(out.shape)) != total:
            raise ValueError("out must be a contiguous float32 array of X's kind with %d entries" % total)
    ms = ctx._run(ctx._lib.ssp_pairwise_scores, where, timing, ctx._h, ptr, seg._h, q, _raw_ptr(vec[0], _lib.HOST), _raw_ptr(vec[1], _lib.HOST),
                  float(c0), _raw_ptr(out, where), where)
    return (out, ms) if timing else out


def ahc_cluster(ctx: Context, scores, seg_or_counts, linkage: str = "average", threshold: float = 0.0, min_clusters: int = 1,
                n_speakers=None, merges: bool = False, timing: bool = False) -> dict:
    """Agglomerative hierarchical clustering of every recording of a packed batch of score matrices, one workgroup per recording
    (ssp_ahc_cluster; include/ssp.h has the definition).  scores: what pairwise_scores returns, numpy or torch CUDA tensor.  Merging
    goes on while the best pair scores >= threshold and more than min_clusters clusters are left; n_speakers (one entry per recording,
    0 = not known) fixes the count of a recording instead.  Returns "labels" (total,) int32 — clusters numbered by their smallest
    member; -1 for a recording with a non-finite score — and "n_clusters" (R,) int32, with merges=True also "merge_pair" (total, 2)
    int32 and "merge_score" (total,) float32: merge m of recording r in row offsets[r] + m, unused rows (-1, -1) and NaN.  The arrays
    are of scores' kind; a device call given a Segments object returns without a host wait."""
    if linkage not in AHC_LINKAGES:
        raise ValueError("linkage must be one of %s" % sorted(AHC_LINKAGES))
    keep, ptr, where = _as_f32(scores, "scores")
    seg = _as_recordings(ctx, seg_or_counts)
    if int(np.prod(keep.shape)) != pairwise_size(seg):
        raise ValueError("scores has %d entries, the recordings' blocks %d" % (int(np.prod(keep.shape)), pairwise_size(seg)))
    ns = None
    if n_speakers is not None:
        ns = np.ascontiguousarray(n_speakers, dtype=np.int32).reshape(-1)
        if ns.shape[0] != seg.n:
            raise ValueError("n_speakers must have one entry per recording")
    total = seg.total
    lab = ctx._empty((total,), where, "int32")
    cnt = ctx._empty((seg.n,), where, "int32")
    cnt[...] = 0   # (a recording without segments is not written)
    mp = ctx._empty((total, 2), where, "int32") if merges else None
    msc = ctx._empty((total,), where) if merges else None
    ms = ctx._run(ctx._lib.ssp_ahc_cluster, where, timing, ctx._h, ptr, seg._h, AHC_LINKAGES[linkage], float(threshold), int(min_clusters),
                  _raw_ptr(ns, _lib.HOST), _raw_ptr(lab, where), _raw_ptr(cnt, where), _raw_ptr(mp, where), _raw_ptr(msc, where), where)
    return _result(timing, ms, labels=lab, n_clusters=cnt, merge_pair=mp, merge_score=msc)


VBHMM_MAX_STATES = 64     # most HMM states of ssp_vbhmm_resegment (include/ssp.h); its q, rows and iterations: 1024, 4096, 100
VBHMM_MAX_ITERS = 100
VBHMM_LDS_BYTES = _lib.VBHMM_LDS_BYTES              # LDS a workgroup has for alpha and its two T x SP buffers
VBHMM_ALPHA_LDS_BYTES = _lib.VBHMM_ALPHA_LDS_BYTES  # alpha (SP x (q | 1) floats) sits in LDS up to this many bytes, else in the workspace
VBHMM_WANT = ("gamma", "pi", "elbo", "loglik")


def vbhmm_padded_states(n_states: int) -> int:
    """SP: the columns the kernel pads n_states to (its three template instances)"""
    return 16 if n_states <= 16 else (32 if n_states <= 32 else 64)


def vbhmm_alpha_in_lds(n_states: int, q: int) -> bool:
    return vbhmm_padded_states(n_states) * (int(q) | 1) * 4 <= VBHMM_ALPHA_LDS_BYTES


def vbhmm_n_lds(n_states: int, q: int) -> int:
    """the residency border of ssp_vbhmm_resegment: recordings of up to this many rows keep their two T x SP buffers in LDS (beside
    alpha, where that sits in LDS), longer ones in the context's workspace"""
    a = vbhmm_padded_states(n_states) * (int(q) | 1) * 4
    return (VBHMM_LDS_BYTES - (a if a <= VBHMM_ALPHA_LDS_BYTES else 0)) // (8 * vbhmm_padded_states(n_states))


def vb_resegment(ctx: Context, X, seg_or_counts, phi, init_labels, n_init=None, n_states=None, loop_prob: float = 0.99, Fa: float = 0.3,
                 Fb: float = 17.0, init_smoothing: float = 5.0, max_iters: int = 10, epsilon: float = 1e-4, want=("gamma", "pi", "elbo"),
                 out=None, timing: bool = False) -> dict:
    """VB-HMM resegmentation of every recording of a batch, one workgroup per recording (ssp_vbhmm_resegment; include/ssp.h has the
    model).  X (total, q) numpy or torch CUDA tensor: the PROJECTED vectors (plda.Plda.project) in time order; phi: host vector of q
    entries (plda.Plda.psi_); init_labels (total,) and n_init (R,) or None, int32 of X's kind: what ahc_cluster returns as "labels" and
    "n_clusters" feeds it on the device with no read-back.  n_states: HMM states, default 64 for device inputs (no read-back) and
    max(init_labels) + 1 clamped to [1, 64] for host inputs.  Returns "labels", "states" (total,) int32, "n_speakers", "n_iters" (R,)
    int32 — -1 / -1 / -1 / 0 for a recording with a non-finite entry — and what ``want`` names of "gamma" (total, S) float32, "pi"
    (R, S) float32, "elbo" (R, max_iters) float64 (NaN beyond n_iters) and "loglik" (total, S) float32 (inert columns unspecified).
    out: a dict of arrays of X's kind to write into, by those names.  A device call given a Segments object returns without a host wait."""
    keep, ptr, where = _as_f32(X, "X")
    if keep.ndim != 2:
        raise ValueError("X must be (total, q)")
    seg = _as_recordings(ctx, seg_or_counts)
    q, total = int(keep.shape[1]), seg.total
    if int(keep.shape[0]) != total:
        raise ValueError("X has %d rows, the recordings %d" % (int(keep.shape[0]), total))
    for w in want:
        if w not in VBHMM_WANT:
            raise ValueError("want: %r is not one of %s" % (w, VBHMM_WANT))
    ph = np.ascontiguousarray(phi.cpu().numpy() if _is_torch(phi) else phi, dtype=np.float32).reshape(-1)
    if ph.shape[0] != q:
        raise ValueError("phi must have %d entries" % q)

    def ints(x, name, n):
        if where == _lib.DEVICE:
            import torch
            if not (_is_torch(x) and x.is_cuda):
                raise ValueError("%s must be a torch CUDA tensor, as X is" % name)
            x = x.to(torch.int32).contiguous().reshape(-1)
        else:
            x = np.ascontiguousarray(x.cpu().numpy() if _is_torch(x) else x, dtype=np.int32).reshape(-1)
        if int(x.shape[0]) != n:
            raise ValueError("%s must have %d entries" % (name, n))
        return x
    lab0 = ints(init_labels, "init_labels", total)
    ni = None if n_init is None else ints(n_init, "n_init", seg.n)
    if n_states is None:
        n_states = VBHMM_MAX_STATES if where == _lib.DEVICE else int(min(VBHMM_MAX_STATES, max(1, (int(lab0.max()) + 1) if total else 1)))
    S, mi = int(n_states), int(max_iters)
    shapes = {"labels": ((total,), "int32"), "states": ((total,), "int32"), "n_speakers": ((seg.n,), "int32"), "n_iters": ((seg.n,), "int32"),
              "elbo": ((seg.n, mi), "float64"), "gamma": ((total, S), "float32"), "pi": ((seg.n, S), "float32"), "loglik": ((total, S), "float32")}
    res = {}
    for name in ("labels", "states", "n_speakers", "n_iters") + tuple(w for w in VBHMM_WANT if w in want):
        shape, dt = shapes[name]
        if out is not None and name in out:
            o = out[name]
            ok = (_is_torch(o) and where == _lib.DEVICE and o.is_cuda and str(o.dtype) == "torch." + dt and o.is_contiguous()) or (
                isinstance(o, np.ndarray) and where == _lib.HOST and o.dtype == np.dtype(dt) and o.flags.c_contiguous)
            if not ok or tuple(int(v) for v in o.shape) != tuple(shape):
                raise ValueError("out[%r] must be a contiguous %s array of X's kind and shape %s" % (name, dt, tuple(shape)))
            res[name] = o
        else:
            res[name] = ctx._empty(shape, where, dt)
            if name in ("n_speakers", "n_iters", "pi", "elbo"):
                res[name][...] = 0   # (a recording without rows is not written)
    outs = [_raw_ptr(res.get(name), where) for name in ("labels", "states", "n_speakers", "n_iters", "elbo", "gamma", "pi", "loglik")]
    ms = ctx._run(ctx._lib.ssp_vbhmm_resegment, where, timing, ctx._h, ptr, seg._h, q, ph.ctypes.data, _raw_ptr(lab0, where), _raw_ptr(ni, where), S,
                  float(loop_prob), float(Fa), float(Fb), float(init_smoothing), mi, float(epsilon), *outs, where)
    return _result(timing, ms, **res)


def centroids(ctx: Context, X, labels, num: int):
    """avg[s] = mean(X[labels == s]) (float64 accumulator, row order) — d_vector.py:310-313."""
    keep, ptr, where = _as_f32(X, "X")
    if keep.ndim != 2:
        raise ValueError("X must be (N, d)")
    if where == _lib.DEVICE:
        import torch
        lab = labels.to(torch.int32).contiguous()
        lptr = lab.data_ptr()
    else:
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        lptr = lab.ctypes.data
    if int(lab.shape[0]) != int(keep.shape[0]):
        raise ValueError("one label per row of X")
    out = ctx._empty((int(num), int(keep.shape[1])), where)
    ctx._run(ctx._lib.ssp_centroids, where, False, ctx._h, ptr, lptr, int(keep.shape[0]), int(keep.shape[1]), int(num), _raw_ptr(out, where), where)
    return out


def dtw_distances(ctx: Context, queries, templates, normalize: bool = False, timing: bool = False):
    """All-pairs DTW distances (ssp_dtw_distances).  queries / templates: lists of arrays, each (L,) (the reference's
    flattened MFCCs) or (L, dim).  Returns the (n_q, n_t) float32 matrix (numpy).  A pair with an empty sequence scores +inf; a pair
    with a NaN or an infinity scores what the float64 recurrence gives, NaN or +inf (include/ssp.h)."""
    def pack(seqs):
        arrs = [np.asarray(s, dtype=np.float32) for s in seqs]
        arrs = [a.reshape(-1, 1) if a.ndim == 1 else a for a in arrs]
        dims = {a.shape[1] for a in arrs if a.shape[0] > 0}
        if len(dims) > 1:
            raise ValueError("all sequences must share the feature dimension")
        dim = dims.pop() if dims else 1
        flat = np.concatenate([a.reshape(-1, dim) for a in arrs]) if arrs else np.zeros((0, dim), np.float32)
        return np.ascontiguousarray(flat), Segments.from_lengths(ctx, [a.shape[0] for a in arrs]), dim
    q, qs, dq = pack(queries)
    t, ts, dt = pack(templates)
    if q.shape[0] == 0 or t.shape[0] == 0:   # a side without a single row has no dimension of its own: every pair is +inf
        dq = dt = dt if q.shape[0] == 0 else dq
    if dq != dt:
        raise ValueError("queries and templates must share the feature dimension")
    out = np.empty((qs.n, ts.n), dtype=np.float32)
    ms = ctx._run(ctx._lib.ssp_dtw_distances, _lib.HOST, timing, ctx._h, q.ctypes.data, qs._h, t.ctypes.data, ts._h, dq, 1 if normalize else 0,
                  out.ctypes.data, _lib.HOST)
    return (out, ms) if timing else out


def fastdtw_distances(ctx: Context, queries, templates, radius: int = 1, timing: bool = False):
    """All-pairs FastDTW distances (ssp_fastdtw_distances): the reference's dtw_method = 2 (MFCC_DTW.py:69-70) on 1-D sequences,
    float64.  Returns the (n_q, n_t) float64 matrix."""
    def pack(seqs):
        arrs = [np.ascontiguousarray(np.asarray(s, dtype=np.float32).reshape(-1)) for s in seqs]
        flat = np.concatenate(arrs) if arrs else np.zeros(0, np.float32)
        return flat, Segments.from_lengths(ctx, [a.shape[0] for a in arrs])
    fq, sq = pack(queries)
    ft, st = pack(templates)
    out = np.empty((sq.n, st.n), dtype=np.float64)
    ms = ctx._run(ctx._lib.ssp_fastdtw_distances, _lib.HOST, timing, ctx._h, fq.ctypes.data, sq._h, ft.ctypes.data, st._h, int(radius), out.ctypes.data)
    return (out, ms) if timing else out


def dtw_path(ctx: Context, x, y):
    """d and the warping path of dtw.accelerated_dtw(x, y, 'euclidean') (ssp_dtw_path, float64 on the GPU).
    x (r,) or (r, dim), y (c,) or (c, dim).  Returns (d, path_i int64[len], path_j int64[len])."""
    a = np.asarray(x, dtype=np.float32)
    b = np.asarray(y, dtype=np.float32)
    a = np.ascontiguousarray(a.reshape(-1, 1) if a.ndim == 1 else a)
    b = np.ascontiguousarray(b.reshape(-1, 1) if b.ndim == 1 else b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or a.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError("x (r, dim) and y (c, dim) must be non-empty and share dim")
    r, c = a.shape[0], b.shape[0]
    pi = np.empty(r + c, dtype=np.int32)
    pj = np.empty(r + c, dtype=np.int32)
    d = C.c_double(0.0)
    n = C.c_int32(0)
    _lib.check(ctx._lib.ssp_dtw_path(ctx._h, a.ctypes.data, r, b.ctypes.data, c, a.shape[1], C.byref(d), pi.ctypes.data,
                                      pj.ctypes.data, C.byref(n)))
    return d.value, pi[:n.value].astype(np.int64), pj[:n.value].astype(np.int64)


def _dtw_direction_bytes(r: int, c: int) -> int:
    """Bytes of the direction store ssp_dtw_templates keeps for one (sample of r rows, template of c rows) pair: one byte per cell,
    rows padded to a multiple of four.  ``workspace_bytes`` of dtw_templates caps the sum over the pairs of one round."""
    return int(r) * ((int(c) + 3) // 4 * 4)


def _pack_template_groups(groups):
    """The argument checks of dtw_templates (no context needed): (x float64 (rows, dim), seq_off, grp_off, dim, flat)."""
    x, lens, grp_off, dims, flat = [], [], [0], set(), set()
    for g, group in enumerate(groups):
        group = list(group)
        if not group:
            raise ValueError("group %d is empty" % g)
        for s in group:
            a = np.asarray(s, dtype=np.float64)
            if a.ndim not in (1, 2):
                raise ValueError("samples must be (L,) or (L, dim) arrays")
            if a.shape[0] < 1 or (a.ndim == 2 and a.shape[1] < 1):
                raise ValueError("group %d has an empty sample" % g)
            if not np.isfinite(a).all():
                raise ValueError("group %d has a non-finite value" % g)
            flat.add(a.ndim == 1)
            dims.add(1 if a.ndim == 1 else a.shape[1])
            x.append(a.reshape(a.shape[0], -1))
            lens.append(a.shape[0])
        grp_off.append(len(lens))
    if len(flat) > 1 or len(dims) > 1:
        raise ValueError("all samples must share the number of dimensions and the feature dimension")
    seq_off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=seq_off[1:])
    return np.ascontiguousarray(np.concatenate(x)), seq_off, np.asarray(grp_off, dtype=np.int64), dims.pop(), flat.pop()


def dtw_templates(ctx, groups, workspace_bytes: int = 0, timing: bool = False):
    """One DTW template per group of samples (ssp_dtw_templates): what MFCC_DTW.generate_template gives for each group, with round k of
    ALL groups in one launch.  groups: a list of lists of arrays, every array (L,) (the reference's flattened MFCCs) or every array
    (L, dim).  Returns a list of float64 arrays (L_g,) / (L_g, dim), L_g the length of group g's longest sample.  ``workspace_bytes``
    caps the direction store of one round (0: 1 GiB; a pair of r x c cells takes r rows of c bytes, rows padded to a multiple of four); the result does not depend on it.  The arguments are
    checked before a context is needed: ``ctx=None`` takes the default context after they passed."""
    groups = list(groups)
    if int(workspace_bytes) < 0:
        raise ValueError("workspace_bytes must be >= 0")
    if not groups:
        return ([], 0.0) if timing else []
    x, seq_off, grp_off, dim, flat = _pack_template_groups(groups)
    if ctx is None:
        ctx = default_context()
    n_grp = len(grp_off) - 1
    longest = [int(np.diff(seq_off[grp_off[g]:grp_off[g + 1] + 1]).max()) for g in range(n_grp)]
    out = np.empty((sum(longest), dim), dtype=np.float64)
    toff = np.empty(n_grp + 1, dtype=np.int64)
    ms = ctx._run(ctx._lib.ssp_dtw_templates, _lib.HOST, timing, ctx._h, x.ctypes.data, seq_off.ctypes.data, len(seq_off) - 1, grp_off.ctypes.data,
                  n_grp, dim, int(workspace_bytes), out.ctypes.data, toff.ctypes.data)
    res = [out[toff[g]:toff[g + 1]].reshape(-1).copy() if flat else out[toff[g]:toff[g + 1]].copy() for g in range(n_grp)]
    return (res, ms) if timing else res


def dense_forward(ctx: Context, X, Wt, bias=None, relu: bool = False, timing: bool = False):
    """Y = act(X @ Wt.T + bias) — one Keras Dense layer (ssp_dense_forward).  X (N, d_in); Wt (units, d_in) is the Keras
    kernel transposed; all arrays numpy (host) or all torch CUDA tensors.  Returns Y (N, units) of the same kind."""
    xk, xp, where = _as_f32(X, "X")
    wk, wp, wwhere = _as_f32(Wt, "Wt")
    if wwhere != where:
        raise ValueError("X and Wt must both be numpy arrays or both be torch CUDA tensors")
    if xk.ndim != 2 or wk.ndim != 2 or xk.shape[1] != wk.shape[1]:
        raise ValueError("X (N,d_in) and Wt (units,d_in) must share d_in")
    N, d_in, units = int(xk.shape[0]), int(xk.shape[1]), int(wk.shape[0])
    bk, bp = None, None
    if bias is not None:
        bk, bp, bwhere = _as_f32(bias, "bias")
        if bwhere != where or int(np.prod(bk.shape)) != units:
            raise ValueError("bias must have `units` entries and live where X lives")
    Y = ctx._empty((N, units), where)
    ms = ctx._run(ctx._lib.ssp_dense_forward, where, timing, ctx._h, xp, N, d_in, wp, bp, units, 1 if relu else 0, _raw_ptr(Y, where), where)
    return (Y, ms) if timing else Y


class DnnForward(_Handle):
    """A fully connected network packed once for the GPU forward pass (ssp_dnn): ``layers`` = list of (Wt (units, d_in) float32 — the
    Keras kernel transposed —, bias (units,) or None, relu bool).  ``forward(X)`` = predict: the layers whose widths are <= 256 run in
    one kernel with the activations kept in registers (the d-vector network's hidden and output layers), wider layers in front of
    them one GEMM launch each."""

    _DESTROY = "ssp_dnn_destroy"

    def __init__(self, ctx: Context, layers):
        super().__init__(ctx)
        n = len(layers)
        if n < 1:
            raise ValueError("at least one layer")
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w, _, _ in layers]
        bs = [None if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for _, b, _ in layers]
        dims = [int(ws[0].shape[1])] + [int(w.shape[0]) for w in ws]
        for i, w in enumerate(ws):
            if w.ndim != 2 or w.shape[1] != dims[i] or (bs[i] is not None and bs[i].shape[0] != dims[i + 1]):
                raise ValueError("layer %d: kernel (units, d_in) / bias (units,) do not chain" % i)
        self.dims = dims
        c_dims = (C.c_int32 * (n + 1))(*dims)
        c_w = (C.c_void_p * n)(*[w.ctypes.data for w in ws])
        c_b = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for b in bs])
        c_r = (C.c_int32 * n)(*[1 if r else 0 for _, _, r in layers])
        self._create(self._lib.ssp_dnn_create, ctx._h, n, c_dims, c_w, c_b, c_r)

    def forward(self, X, timing: bool = False):
        xk, xp, where = _as_f32(X, "X")
        if xk.ndim != 2 or int(xk.shape[1]) != self.dims[0]:
            raise ValueError("X must be (N, %d)" % self.dims[0])
        N = int(xk.shape[0])
        Y = self.ctx._empty((N, self.dims[-1]), where)
        ms = self.ctx._run(self._lib.ssp_dnn_forward, where, timing, self._h, xp, N, _raw_ptr(Y, where), where)
        return (Y, ms) if timing else Y


class _Trainer(_Handle):
    """What DnnTrainer, LstmTrainer and GruTrainer share: the data checks, epoch / evaluate, the step counter and the handle's life.  A
    subclass names its entry points' prefix (ssp_<prefix>_trainer_*), creates ``_h`` and sets ``_row``, the shape of one row of X."""

    _PREFIX = ""
    _CHANNEL_AXIS = False  # X may come with a trailing axis of one channel, (N, T, D, 1): what the Keras model takes

    def _fn(self, name):
        return getattr(self._lib, "ssp_%s_trainer_%s" % (self._PREFIX, name))

    @property
    def _DESTROY(self):
        return "ssp_%s_trainer_destroy" % self._PREFIX

    def _data(self, X, labels):
        xk, xp, where = _as_f32(X, "X")
        if self._CHANNEL_AXIS and xk.ndim == 4 and int(xk.shape[3]) == 1:
            xk = xk.reshape(xk.shape[0], xk.shape[1], xk.shape[2])
        if tuple(int(v) for v in xk.shape[1:]) != self._row:
            raise ValueError("X must be (N, %s)" % ", ".join("%d" % v for v in self._row))
        if where == _lib.DEVICE:
            import torch
            if not (_is_torch(labels) and labels.is_cuda):
                raise ValueError("labels must live where X lives")
            lk = labels.to(torch.int32).contiguous()
            lp = lk.data_ptr()
        else:
            lk = np.ascontiguousarray(labels, dtype=np.int32)
            lp = lk.ctypes.data
        if lk.ndim != 1 or int(lk.shape[0]) != int(xk.shape[0]):
            raise ValueError("one label per row of X")
        return (xk, lk), xp, lp, int(xk.shape[0]), where

    def _epoch(self, X, labels, order, batch_size, lr, extra, timing):
        keep, xp, lp, N, where = self._data(X, labels)
        ok, op = None, None
        if order is not None:
            ok = np.ascontiguousarray(order, dtype=np.int64)
            if ok.shape != (N,):
                raise ValueError("order must hold N row indices")
            op = ok.ctypes.data
        loss, corr = C.c_double(0.0), C.c_int64(0)
        ms = self.ctx._run(self._fn("epoch"), where, timing, self._h, xp, lp, N, op, int(batch_size), float(lr), *extra, C.byref(loss),
                           C.byref(corr), where)
        return (loss.value, corr.value, ms) if timing else (loss.value, corr.value)

    def epoch(self, X, labels, order=None, batch_size: int = 128, lr: float = 1e-4, timing: bool = False):
        """ceil(N / batch_size) training steps over the rows in ``order`` (int64 (N,), default 0..N-1) -> (loss sum, correct rows)
        as the steps ran; with ``timing`` the kernel milliseconds as a third entry"""
        return self._epoch(X, labels, order, batch_size, lr, (), timing)

    def evaluate(self, X, labels, timing: bool = False):
        """loss sum and correct rows over (X, labels), dropout off; nothing is updated"""
        keep, xp, lp, N, where = self._data(X, labels)
        loss, corr = C.c_double(0.0), C.c_int64(0)
        ms = self.ctx._run(self._fn("evaluate"), where, timing, self._h, xp, lp, N, C.byref(loss), C.byref(corr), where)
        return (loss.value, corr.value, ms) if timing else (loss.value, corr.value)

    def _read_into(self, name, out):
        """the array ``read`` fills for tensor ``name``: a new one, or ``out`` when it is a contiguous float32 array of the tensor's size"""
        if out is None:
            return np.empty(self.shapes[name], dtype=np.float32)
        if out.dtype != np.float32 or out.size != int(np.prod(self.shapes[name])) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous float32 array of %d entries" % int(np.prod(self.shapes[name])))
        return out

    @property
    def steps(self) -> int:
        return _read_int(C.c_int64, self._fn("steps"), self._h)


class DnnTrainer(_Trainer):
    """A fully connected network with its gradients and Adam state on the GPU (ssp_dnn_trainer): nn_model.inference's spk.fit,
    d_vector.py:168-206.  ``layers`` = list of (W (d_in, units) float32 in Keras' layout, bias (units,) or None, relu bool, dropout rate
    after the activation).  X and labels are numpy arrays (host) or torch CUDA tensors (X float32, labels int32)."""

    WHAT = {"W": 0, "b": 1, "dW": 2, "db": 3, "mW": 4, "mb": 5, "vW": 6, "vb": 7}
    _PREFIX = "dnn"

    def __init__(self, ctx: Context, layers, max_batch: int = 128):
        super().__init__(ctx)
        n = len(layers)
        if n < 1:
            raise ValueError("at least one layer")
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w, _, _, _ in layers]
        bs = [None if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for _, b, _, _ in layers]
        if any(w.ndim != 2 for w in ws):
            raise ValueError("kernels must be (d_in, units)")
        dims = [int(ws[0].shape[0])] + [int(w.shape[1]) for w in ws]
        for i, w in enumerate(ws):
            if w.shape[0] != dims[i] or (bs[i] is not None and bs[i].shape[0] != dims[i + 1]):
                raise ValueError("layer %d: kernel (d_in, units) / bias (units,) do not chain" % i)
        self.dims, self.has_bias, self.max_batch = dims, [b is not None for b in bs], int(max_batch)
        self._row = (dims[0],)
        c_dims = (C.c_int32 * (n + 1))(*dims)
        c_r = (C.c_int32 * n)(*[1 if r else 0 for _, _, r, _ in layers])
        c_p = (C.c_float * n)(*[float(p) for _, _, _, p in layers])
        c_w = (C.c_void_p * n)(*[w.ctypes.data for w in ws])
        c_b = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for b in bs])
        self._create(self._lib.ssp_dnn_trainer_create, ctx._h, n, c_dims, c_r, c_p, c_w, c_b, int(max_batch))

    def epoch(self, X, labels, order=None, batch_size: int = 128, lr: float = 1e-4, seed: int = 0, timing: bool = False):
        """ceil(N / batch_size) training steps over the rows in ``order`` (int64 (N,), default 0..N-1) -> (loss sum, correct rows)
        as the steps ran; with ``timing`` the kernel milliseconds as a third entry.  ``seed`` keys the dropout"""
        return self._epoch(X, labels, order, batch_size, lr, (int(seed) & (2 ** 64 - 1),), timing)

    def read(self, what: str, layer: int):
        """'W', 'b' (parameters), 'dW', 'db' (the last step's gradients), 'mW', 'mb', 'vW', 'vb' (Adam's moments) of ``layer`` -> numpy"""
        layer = int(layer)
        if not 0 <= layer < len(self.dims) - 1:
            raise ValueError("layer %d of %d" % (layer, len(self.dims) - 1))
        code = self.WHAT[what]
        out = np.empty((self.dims[layer + 1],) if code & 1 else (self.dims[layer], self.dims[layer + 1]), dtype=np.float32)
        _lib.check(self._lib.ssp_dnn_trainer_read(self._h, code, layer, out.ctypes.data))
        return out


def dropout_keep(seed: int, step: int, layer: int, rows: int, width: int, rate: float):
    """the trainer's dropout decision (ssp_dropout_keep; computed on the host, no device): bool (rows, width), True = kept"""
    out = np.empty((int(rows), int(width)), dtype=np.uint8)
    lib = _lib.load()
    _lib.check(lib.ssp_dropout_keep(int(seed) & (2 ** 64 - 1), int(step), int(layer), int(rows), int(width), float(rate), out.ctypes.data))
    return out.astype(bool)


LSTM_ACTIVATIONS = {"hard_sigmoid": 0, "sigmoid": 1}


def _lstm_arrays(W, U, b):
    """contiguous float32 (W (d_in, 4 units), U (units, 4 units), b (4 units,) or None) in Keras' layout, shapes checked"""
    W = np.ascontiguousarray(W, dtype=np.float32)
    U = np.ascontiguousarray(U, dtype=np.float32)
    if W.ndim != 2 or U.ndim != 2 or U.shape[1] != 4 * U.shape[0] or W.shape[1] != U.shape[1]:
        raise ValueError("W must be (d_in, 4 units) and U (units, 4 units)")
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    if b is not None and b.shape[0] != U.shape[1]:
        raise ValueError("b must have 4 units entries")
    return W, U, b


def lstm_pack_weights(W, U, b=None):
    """The operand-order weight image LstmForward uploads, built on the host by ssp_lstm_pack_weights (no device, no context): float32
    vector laid out as include/ssp.h documents.  W (d_in, 4 units), U (units, 4 units), b (4 units,) or None — Keras' layout."""
    W, U, b = _lstm_arrays(W, U, b)
    lib = _lib.load()
    d_in, units = int(W.shape[0]), int(U.shape[0])
    img = np.empty(_read_int(C.c_int64, lib.ssp_lstm_pack_weights, d_in, units, None, None, None, None), dtype=np.float32)
    _lib.check(lib.ssp_lstm_pack_weights(d_in, units, W.ctypes.data, U.ctypes.data, _raw_ptr(b, _lib.HOST), img.ctypes.data, None))
    return img


class LstmForward(_Handle):
    """One Keras LSTM layer packed once for the GPU forward pass (ssp_lstm; d_vector.py:271-294): W (d_in, 4 units), U (units, 4 units),
    b (4 units,) or None in Keras' layout (gate blocks i | f | c | o), ``recurrent_activation`` 'hard_sigmoid' or 'sigmoid' — named by
    the caller, there is no default.  ``forward`` returns the last hidden state of every sequence.  units: a multiple of 16 up to 128,
    d_in up to 64 (NotImplementedError otherwise)."""

    _DESTROY = "ssp_lstm_destroy"

    def __init__(self, ctx: Context, W, U, b, recurrent_activation):
        if recurrent_activation not in LSTM_ACTIVATIONS:
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        super().__init__(ctx)
        W, U, b = _lstm_arrays(W, U, b)
        self.d_in, self.units = int(W.shape[0]), int(U.shape[0])
        self.recurrent_activation = recurrent_activation
        self._create(self._lib.ssp_lstm_create, ctx._h, self.d_in, self.units, W.ctypes.data, U.ctypes.data, _raw_ptr(b, _lib.HOST),
                     LSTM_ACTIVATIONS[recurrent_activation])

    def forward(self, feats, frame_seg: Optional[Segments] = None, timing: bool = False):
        """feats (N, T, d_in) — equal lengths, no segments needed — or (frames, d_in) laid out by ``frame_seg`` (what MfccPlan.run
        returns); numpy (host) or torch CUDA tensor.  Returns (n sequences, units) of the same kind [and kernel milliseconds]."""
        keep, ptr, where = _as_f32(feats, "feats")
        if keep.ndim == 3:
            if frame_seg is not None:
                raise ValueError("(N, T, d_in) input takes no frame_seg")
            if int(keep.shape[2]) != self.d_in:
                raise ValueError("feats must be (N, T, %d)" % self.d_in)
            if int(keep.shape[0]) == 0:
                out = self.ctx._empty((0, self.units), where)
                return (out, 0.0) if timing else out
            frame_seg = Segments(self.ctx, np.arange(int(keep.shape[0]) + 1, dtype=np.int64) * int(keep.shape[1]))
        elif keep.ndim != 2 or int(keep.shape[1]) != self.d_in or frame_seg is None:
            raise ValueError("feats must be (N, T, %d), or (frames, %d) with frame_seg" % (self.d_in, self.d_in))
        elif int(keep.shape[0]) < int(frame_seg.offsets[-1]):
            raise ValueError("fewer rows than frame_seg has frames")
        out = self.ctx._empty((frame_seg.n, self.units), where)
        ms = self.ctx._run(self._lib.ssp_lstm_forward, where, timing, self._h, ptr, frame_seg._h, _raw_ptr(out, where), where)
        return (out, ms) if timing else out


class LstmTrainer(_Trainer):
    """The recurrent d-vector network with its gradients and Adam state on the GPU (ssp_lstm_trainer): nn_model.inference_lstm's spk.fit,
    d_vector.py:271-294 — one LSTM(units) over a (T, d_in) chunk, Dense(n_class) and a softmax on the last hidden state.  W (d_in, 4 units),
    U (units, 4 units), b (4 units,) or None, Wd (units, n_class), bd (n_class,) or None in Keras' layout; ``recurrent_activation``
    'hard_sigmoid' or 'sigmoid', named by the caller.  X (N, T, d_in) and labels are numpy arrays (host) or torch CUDA tensors (X float32,
    labels int32).  units: a multiple of 16 up to 128, d_in up to 64, T up to 1024 (NotImplementedError otherwise)."""

    WHAT = {"": 0, "d": 1, "m": 2, "v": 3}
    TENSOR = {"W": 0, "U": 1, "b": 2, "Wd": 3, "bd": 4}
    _PREFIX = "lstm"

    def __init__(self, ctx: Context, W, U, b, Wd, bd, *, T, recurrent_activation, max_batch: int = 128):
        if recurrent_activation not in LSTM_ACTIVATIONS:
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        super().__init__(ctx)
        W, U, b = _lstm_arrays(W, U, b)
        Wd = np.ascontiguousarray(Wd, dtype=np.float32)
        bd = None if bd is None else np.ascontiguousarray(bd, dtype=np.float32).reshape(-1)
        if Wd.ndim != 2 or Wd.shape[0] != U.shape[0] or (bd is not None and bd.shape[0] != Wd.shape[1]):
            raise ValueError("Wd must be (units, n_class) and bd (n_class,)")
        self.d_in, self.units, self.n_class, self.T = int(W.shape[0]), int(U.shape[0]), int(Wd.shape[1]), int(T)
        self._row = (self.T, self.d_in)
        self.recurrent_activation, self.max_batch = recurrent_activation, int(max_batch)
        self.has_bias = {"b": b is not None, "bd": bd is not None}
        self.shapes = {"W": (self.d_in, 4 * self.units), "U": (self.units, 4 * self.units), "b": (4 * self.units,),
                       "Wd": (self.units, self.n_class), "bd": (self.n_class,)}
        self._create(self._lib.ssp_lstm_trainer_create, ctx._h, self.d_in, self.units, self.n_class, self.T, LSTM_ACTIVATIONS[recurrent_activation],
                     W.ctypes.data, U.ctypes.data, _raw_ptr(b, _lib.HOST), Wd.ctypes.data, _raw_ptr(bd, _lib.HOST), int(max_batch))

    STEP_LAUNCHES = ("forward+stash", "dense head", "loss", "dWd", "dh_T", "backward through time", "dW+db", "dU", "adam")

    def step_times(self, X, labels, batch_size: int = 128, lr: float = 1e-4):
        """ONE training step on the first ``batch_size`` rows of torch CUDA tensors with a hipEvent between its nine launches ->
        {launch name: milliseconds} (a measurement aid: the step counts like any other)"""
        keep, xp, lp, N, where = self._data(X, labels)
        if where != _lib.DEVICE or N < int(batch_size):
            raise ValueError("step_times takes torch CUDA tensors of at least batch_size rows")
        ms = (C.c_float * len(self.STEP_LAUNCHES))()
        with self.ctx._ordered(where):
            _lib.check(self._lib.ssp_lstm_trainer_step_times(self._h, xp, lp, int(batch_size), float(lr), ms))
        return dict(zip(self.STEP_LAUNCHES, (float(v) for v in ms)))

    def read(self, what: str, out=None):
        """'W', 'U', 'b', 'Wd', 'bd' (parameters), with a prefix 'd' (the last step's gradients), 'm' or 'v' (Adam's moments), e.g. 'dU',
        'mWd' -> numpy; ``out``: a float32 array of the tensor's size to fill instead (it needs 4-byte alignment only)"""
        for prefix in ("", "d", "m", "v"):
            if what.startswith(prefix) and what[len(prefix):] in self.TENSOR and (prefix or what in self.TENSOR):
                name = what[len(prefix):]
                break
        else:
            raise ValueError("unknown tensor %r" % (what,))
        out = self._read_into(name, out)
        _lib.check(self._lib.ssp_lstm_trainer_read(self._h, self.WHAT[prefix], self.TENSOR[name], out.ctypes.data))
        return out


GRU_ACTIVATIONS = LSTM_ACTIVATIONS


def _gru_arrays(W, U, b, reset_after):
    """contiguous float32 (W (d_in, 3 units), U (units, 3 units), b (3 units,) / (2, 3 units) or None) in Keras' layout, shapes checked"""
    W = np.ascontiguousarray(W, dtype=np.float32)
    U = np.ascontiguousarray(U, dtype=np.float32)
    if W.ndim != 2 or U.ndim != 2 or U.shape[1] != 3 * U.shape[0] or W.shape[1] != U.shape[1]:
        raise ValueError("W must be (d_in, 3 units) and U (units, 3 units)")
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32)
        want = (2, U.shape[1]) if reset_after else (U.shape[1],)
        if b.shape != want:
            raise ValueError("b must be %s with reset_after=%s" % (want, bool(reset_after)))
    return W, U, b


class GruForward(_Handle):
    """One Keras GRU layer packed once for the GPU forward pass (ssp_gru; the GRU(1024, return_sequences=True) layers of d_vector.py:229-231):
    W (d_in, 3 units), U (units, 3 units), b in Keras' layout (gate blocks z | r | h).  Both switches are named by the caller, there is no
    default: ``recurrent_activation`` 'hard_sigmoid' or 'sigmoid', ``reset_after`` False (stand-alone Keras; b (3 units,) or None) or True
    (tf.keras 2; b (2, 3 units) or None).  units: a multiple of 16 up to 1024, d_in up to 4096 (NotImplementedError otherwise)."""

    _DESTROY = "ssp_gru_destroy"

    def __init__(self, ctx: Context, W, U, b, recurrent_activation, reset_after):
        if recurrent_activation not in GRU_ACTIVATIONS:
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        if not isinstance(reset_after, (bool, np.bool_)):
            raise ValueError("reset_after must be True or False")
        super().__init__(ctx)
        W, U, b = _gru_arrays(W, U, b, reset_after)
        self.d_in, self.units = int(W.shape[0]), int(U.shape[0])
        self.recurrent_activation, self.reset_after = recurrent_activation, bool(reset_after)
        self._create(self._lib.ssp_gru_create, ctx._h, self.d_in, self.units, W.ctypes.data, U.ctypes.data, _raw_ptr(b, _lib.HOST),
                     GRU_ACTIVATIONS[recurrent_activation], 1 if reset_after else 0)

    def set_workspace(self, nbytes: int) -> "GruForward":
        """cap of the workspace one forward call may hold; larger batches run in slabs of whole chunks (same bits)"""
        _lib.check(self._lib.ssp_gru_set_workspace(self._h, C.c_size_t(int(nbytes))))
        return self

    @property
    def last_slab(self) -> int:
        return _read_int(C.c_int64, self._lib.ssp_gru_last_slab, self._h)

    def forward(self, X, mean: bool = False, timing: bool = False):
        """X (N, T, d_in), numpy (host) or torch CUDA tensor -> the output sequence (N, T, units) of the same kind, or with ``mean=True``
        its mean over time (N, units) [and kernel milliseconds]."""
        keep, ptr, where = _as_f32(X, "X")
        if keep.ndim != 3 or int(keep.shape[2]) != self.d_in or int(keep.shape[1]) < 1:
            raise ValueError("X must be (N, T >= 1, %d)" % self.d_in)
        N, T = int(keep.shape[0]), int(keep.shape[1])
        out = self.ctx._empty((N, self.units) if mean else (N, T, self.units), where)
        ms = 0.0
        if N:
            ms = self.ctx._run(self._lib.ssp_gru_forward, where, timing, self._h, ptr, N, T, None if mean else _raw_ptr(out, where),
                               _raw_ptr(out, where) if mean else None, where)
        return (out, ms) if timing else out


def _xv_vec(x, units, what, where=None):
    """a per-unit vector (bias / scale / offset) or None -> (kept array, address); ``where``: the side it must live on (None: host)"""
    if x is None:
        return None, None
    if where is None:
        a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if a.shape[0] != units:
            raise ValueError("%s must have %d entries" % (what, units))
        return a, a.ctypes.data
    k, p, w = _as_f32(x, what)
    if w != where or int(np.prod(k.shape)) != units:
        raise ValueError("%s must have %d entries and live where X lives" % (what, units))
    return k, p


def _xv_windows(windows, seg: Segments):
    """a window table (n_win, 3) of (sequence, first, end) or None -> (kept int64 array or None, pointer or None, output rows)"""
    if windows is None:
        return None, None, seg.n
    w = np.ascontiguousarray(windows, dtype=np.int64)
    if w.ndim != 2 or w.shape[1] != 3:
        raise ValueError("windows must be (n_win, 3): sequence, first frame, end frame")
    return w, w.ctypes.data_as(C.POINTER(C.c_int64)), int(w.shape[0])


def tdnn_forward(ctx: Context, X, seg_or_counts, W, bias=None, dilation: int = 1, relu: bool = False, scale=None, offset=None,
                 timing: bool = False):
    """ONE frame layer of an x-vector network (ssp_tdnn_forward; include/ssp.h has the definition): X (frames, d_in) laid out by the
    segments, W (units, taps, d_in), bias / scale / offset (units,) or None; all numpy or all torch CUDA tensors.  -> (Y (frames, units)
    of X's kind with the ROW INDEX of X, valid lengths int64 (n_seq,)): the last (taps - 1) dilation rows of each sequence in Y are
    unspecified [and kernel milliseconds]."""
    xk, xp, where = _as_f32(X, "X")
    wk, wp, wwhere = _as_f32(W, "W")
    if wwhere != where:
        raise ValueError("X and W must both be numpy arrays or both be torch CUDA tensors")
    if xk.ndim != 2 or wk.ndim != 3 or int(wk.shape[2]) != int(xk.shape[1]):
        raise ValueError("X (frames, d_in) and W (units, taps, d_in) must share d_in")
    seg = _as_recordings(ctx, seg_or_counts)
    if int(xk.shape[0]) < int(seg.offsets[-1]):
        raise ValueError("fewer rows than the segments have frames")
    units, taps, d_in = int(wk.shape[0]), int(wk.shape[1]), int(wk.shape[2])
    bk, bp = _xv_vec(bias, units, "bias", where)
    sk, sp = _xv_vec(scale, units, "scale", where)
    ok, op = _xv_vec(offset, units, "offset", where)
    Y = ctx._empty((int(xk.shape[0]), units), where)
    lens = np.zeros(seg.n, dtype=np.int64)
    ms = ctx._run(ctx._lib.ssp_tdnn_forward, where, timing, ctx._h, xp, seg._h, d_in, wp, bp, taps, int(dilation), units, 1 if relu else 0, sp, op,
                  _raw_ptr(Y, where), lens.ctypes.data_as(C.POINTER(C.c_int64)), where)
    return (Y, lens, ms) if timing else (Y, lens)


def stats_pool(ctx: Context, X, seg_or_counts, windows=None, var_floor: float = 1e-10, timing: bool = False):
    """Statistics pooling alone (ssp_stats_pool): X (frames, dim) laid out by the segments, windows None (every sequence whole) or a host
    table (n_win, 3) of (sequence, first, end) rows.  -> (n_win or n_seq, 2 dim) of X's kind: means, then deviations [and kernel ms]."""
    xk, xp, where = _as_f32(X, "X")
    if xk.ndim != 2 or int(xk.shape[1]) < 1:
        raise ValueError("X must be (frames, dim)")
    seg = _as_recordings(ctx, seg_or_counts)
    if int(xk.shape[0]) < int(seg.offsets[-1]):
        raise ValueError("fewer rows than the segments have frames")
    wk, wptr, n_out = _xv_windows(windows, seg)
    dim = int(xk.shape[1])
    out = ctx._empty((n_out, 2 * dim), where)
    ms = ctx._run(ctx._lib.ssp_stats_pool, where, timing, ctx._h, xp, seg._h, dim, wptr, n_out if wk is not None else 0, float(var_floor),
                  _raw_ptr(out, where), where)
    return (out, ms) if timing else out


class XVectorForward(_Handle):
    """An x-vector network packed once for the GPU forward pass (ssp_xvector; include/ssp.h has the model).  ``frame_layers``: a list of
    dicts with W (units, taps, d_in) and optionally b, scale, offset (units,), dilation (1) and relu (False); ``segment_layers``: the same
    with W (units, d_in) and no dilation.  ``forward`` returns one embedding per sequence, or per window of a host table."""

    _DESTROY = "ssp_xvector_destroy"

    def __init__(self, ctx: Context, frame_layers, segment_layers=(), var_floor: float = 1e-10):
        super().__init__(ctx)
        if len(frame_layers) < 1:
            raise ValueError("at least one frame layer")
        keep = []

        def pack(layers, ndim, d_in, what):
            n = len(layers)
            units, taps, dil, relu, ptr = [], [], [], [], {k: [] for k in ("W", "b", "scale", "offset")}
            for i, L in enumerate(layers):
                unknown = set(L) - {"W", "b", "scale", "offset", "dilation", "relu"}
                if unknown:
                    raise ValueError("%s layer %d: unknown keys %s" % (what, i, sorted(unknown)))
                W = np.ascontiguousarray(L["W"], dtype=np.float32)
                if W.ndim != ndim or int(W.shape[-1]) != d_in:
                    raise ValueError("%s layer %d: W must be %s with d_in = %d" % (what, i, "(units, taps, d_in)" if ndim == 3 else "(units, d_in)", d_in))
                u = int(W.shape[0])
                keep.append(W)
                ptr["W"].append(W.ctypes.data)
                for k in ("b", "scale", "offset"):
                    a, p = _xv_vec(L.get(k), u, "%s layer %d: %s" % (what, i, k))
                    keep.append(a)
                    ptr[k].append(p)
                units.append(u)
                taps.append(int(W.shape[1]) if ndim == 3 else 1)
                dil.append(int(L.get("dilation", 1)))
                relu.append(1 if L.get("relu", False) else 0)
                d_in = u
            arr = lambda v: (C.c_int32 * max(n, 1))(*v)           # noqa: E731
            vp = lambda v: (C.c_void_p * max(n, 1))(*v)           # noqa: E731
            return n, arr(units), arr(taps), arr(dil), vp(ptr["W"]), vp(ptr["b"]), arr(relu), vp(ptr["scale"]), vp(ptr["offset"]), d_in

        W0 = np.asarray(frame_layers[0]["W"])
        if W0.ndim != 3:
            raise ValueError("frame layer 0: W must be (units, taps, d_in)")
        self.d_in = int(W0.shape[2])
        nf, fu, ft, fd, fw, fb, fr, fs, fo, last = pack(frame_layers, 3, self.d_in, "frame")
        ns, su, _, _, sw, sb, sr, ss, so, _ = pack(segment_layers, 2, 2 * last, "segment")
        self._create(self._lib.ssp_xvector_create, ctx._h, self.d_in, nf, fu, ft, fd, fw, fb, fr, fs, fo, ns, su, sw, sb, sr, ss, so,
                     float(var_floor))   # (keep owns what the pointer arrays point into)
        r, p, e = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self._lib.ssp_xvector_info(self._h, C.byref(r), C.byref(p), C.byref(e)))
        self.receptive_field, self.pooled_width, self.embed_width = r.value, p.value, e.value

    def set_workspace(self, nbytes: int) -> "XVectorForward":
        """cap of the activation workspace one forward call may hold; larger batches run in slabs of whole sequences (same bits)"""
        _lib.check(self._lib.ssp_xvector_set_workspace(self._h, C.c_size_t(int(nbytes))))
        return self

    @property
    def last_slab(self) -> int:
        return _read_int(C.c_int64, self._lib.ssp_xvector_last_slab, self._h)

    def forward(self, feats, seg_or_counts, windows=None, timing: bool = False):
        """feats (frames, d_in) laid out by the segments (an api.Segments or the frames per sequence), numpy (host) or torch CUDA tensor;
        windows: None or a host table (n_win, 3) of (sequence, first, end) input frames.  -> (n_seq or n_win, embed width) of feats'
        kind [and kernel milliseconds]."""
        keep, ptr, where = _as_frames(feats, self.d_in)
        seg = _as_recordings(self.ctx, seg_or_counts)
        if int(keep.shape[0]) < int(seg.offsets[-1]):
            raise ValueError("fewer rows than the segments have frames")
        wk, wptr, n_out = _xv_windows(windows, seg)
        out = self.ctx._empty((n_out, self.embed_width), where)
        ms = self.ctx._run(self._lib.ssp_xvector_forward, where, timing, self._h, ptr, seg._h, wptr, n_out if wk is not None else 0,
                           _raw_ptr(out, where), where)
        return (out, ms) if timing else out


def conv2d_same_out_shape(T: int, D: int, strides):
    """(To, Do) of a `same` convolution: ceil(in / stride)"""
    return -(-int(T) // int(strides[0])), -(-int(D) // int(strides[1]))


def conv2d_same(ctx: Context, X, K, bias=None, strides=(1, 1), timing: bool = False):
    """Conv2D(F, (kh, kw), strides, padding='same') with one input channel, channels last, linear activation (ssp_conv2d_same_forward;
    d_vector.py:216-221) followed by TimeDistributed(Flatten) (:226).  X (N, T, D); K (kh, kw, 1, F) or (kh, kw, F) — the Keras kernel;
    bias (F,) or None; all numpy (host) or all torch CUDA tensors.  Returns (N, To, Do * F) of the same kind, element f_out * F + c."""
    xk, xp, where = _as_f32(X, "X")
    kk, kp, kwhere = _as_f32(K, "K")
    if kwhere != where:
        raise ValueError("X and K must both be numpy arrays or both be torch CUDA tensors")
    if kk.ndim == 4 and int(kk.shape[2]) == 1:
        kk = kk.reshape(kk.shape[0], kk.shape[1], kk.shape[3])
    if xk.ndim != 3 or kk.ndim != 3:
        raise ValueError("X must be (N, T, D) and K (kh, kw, 1, F)")
    N, T, D = (int(v) for v in xk.shape)
    kh, kw, F = (int(v) for v in kk.shape)
    if T < 1 or D < 1:
        raise ValueError("X must be (N, T >= 1, D >= 1)")
    bk, bp = None, None
    if bias is not None:
        bk, bp, bwhere = _as_f32(bias, "bias")
        if bwhere != where or int(np.prod(bk.shape)) != F:
            raise ValueError("bias must have F entries and live where X lives")
    sh, sw = int(strides[0]), int(strides[1])
    if sh < 1 or sw < 1:
        raise ValueError("strides must be >= 1")
    To, Do = conv2d_same_out_shape(T, D, (sh, sw))
    Y = ctx._empty((N, To, Do * F), where)
    ms = ctx._run(ctx._lib.ssp_conv2d_same_forward, where, timing, ctx._h, xp, N, T, D, kp, bp, kh, kw, F, sh, sw, _raw_ptr(Y, where), where)
    return (Y, ms) if timing else Y


def l2_normalize(ctx: Context, X, eps: float = 1e-12, timing: bool = False):
    """K.l2_normalize(X, axis=-1) on rows (ssp_l2_normalize; d_vector.py:243-246): X / sqrt(max(sum X^2, eps)).  X (N, d) numpy or torch
    CUDA tensor -> the same kind."""
    xk, xp, where = _as_f32(X, "X")
    if xk.ndim != 2 or int(xk.shape[1]) < 1:
        raise ValueError("X must be (N, d >= 1)")
    N, d = int(xk.shape[0]), int(xk.shape[1])
    Y = ctx._empty((N, d), where)
    ms = ctx._run(ctx._lib.ssp_l2_normalize, where, timing, ctx._h, xp, N, d, float(eps), _raw_ptr(Y, where), where)
    return (Y, ms) if timing else Y


class GruTrainer(_Trainer):
    """The conv + GRU d-vector network with its gradients and Adam state on the GPU (ssp_gru_trainer): nn_model.inference_gru's spk.fit,
    d_vector.py:213-269 — Conv2D (l2-regularised kernel, lambda 0.01) -> n GRU layers -> mean over time -> Dense(E) -> l2_normalize ->
    Dense(n_class) softmax.  ``conv`` = (K (kh, kw, 1, F), b (F,) or None, strides), ``grus`` = [(W (d_in, 3 units), U (units, 3 units),
    b (3 units,) or None), ...], ``dense`` = (W (units, E), b or None), ``head`` = (W (E, n_class), b or None), all in Keras' layout.
    Both GRU switches are named by the caller; ``reset_after=True`` is not trained (NotImplementedError).  X (N, T, D) and labels are
    numpy arrays (host) or torch CUDA tensors (X float32, labels int32).  Limits (NotImplementedError otherwise): kernels up to 7 x 7, 256
    filters, strides 1 or 2, 1 to 4 GRU layers of units a multiple of 16 up to 1024, d_in up to 4096, n_class in [2, 4096], max_batch
    up to 1024 and a workspace of one step within 4 GiB.  Tensor names for ``read``: conv_K, conv_b, gru{i}_W, gru{i}_U, gru{i}_b,
    dense_W, dense_b, head_W, head_b.  Unpinned against Keras."""

    WHAT = {"": 0, "d": 1, "m": 2, "v": 3}
    MAX_LAYERS = 4
    _PREFIX = "gru"
    _CHANNEL_AXIS = True

    def __init__(self, ctx: Context, conv, grus, dense, head, *, T, D, recurrent_activation, reset_after, max_batch: int = 128):
        if recurrent_activation not in GRU_ACTIVATIONS:
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        if not isinstance(reset_after, (bool, np.bool_)):
            raise ValueError("reset_after must be True or False")
        super().__init__(ctx)
        K, bc, strides = conv
        K = np.ascontiguousarray(K, dtype=np.float32)
        if K.ndim == 4 and K.shape[2] == 1:
            K = K.reshape(K.shape[0], K.shape[1], K.shape[3])
        if K.ndim != 3:
            raise ValueError("the convolution kernel must be (kh, kw, 1, F)")
        kh, kw, F = (int(v) for v in K.shape)
        vec = lambda b, n, what: None if b is None else _gru_vec(b, n, what)  # noqa: E731
        bc = vec(bc, F, "conv bias")
        sh, sw = int(strides[0]), int(strides[1])
        self.T, self.D, self.strides = int(T), int(D), (sh, sw)
        self._row = (self.T, self.D)
        if sh < 1 or sw < 1 or self.D < 1:
            raise ValueError("strides and D must be >= 1")
        To, Do = conv2d_same_out_shape(max(self.T, 1), self.D, (sh, sw))
        if len(grus) < 1:
            raise ValueError("at least one GRU layer")
        layers, d_in = [], Do * F
        for i, (W, U, b) in enumerate(grus):
            W, U, _ = _gru_arrays(W, U, None, False)
            if W.shape[0] != d_in:
                raise ValueError("GRU layer %d must take %d features" % (i, d_in))
            # reset_after=True is refused by create before it reads anything, whichever of the two bias layouts came with it
            if b is not None:
                b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1) if reset_after else _gru_vec(b, U.shape[1], "GRU bias")
            layers.append((W, U, b))
            d_in = int(U.shape[0])
        Wd, bd = np.ascontiguousarray(dense[0], dtype=np.float32), dense[1]
        if Wd.ndim != 2 or Wd.shape[0] != d_in:
            raise ValueError("the Dense kernel must be (units, E)")
        E = int(Wd.shape[1])
        bd = vec(bd, E, "Dense bias")
        Wh, bh = np.ascontiguousarray(head[0], dtype=np.float32), head[1]
        if Wh.ndim != 2 or Wh.shape[0] != E:
            raise ValueError("the head's kernel must be (E, n_class)")
        self.n_class = int(Wh.shape[1])
        bh = vec(bh, self.n_class, "head bias")
        self.units = [int(U.shape[0]) for _, U, _ in layers]
        self.n_gru, self.embedding, self.filters = len(layers), E, F
        self.recurrent_activation, self.reset_after, self.max_batch = recurrent_activation, bool(reset_after), int(max_batch)
        self.TENSOR = {"conv_K": 0, "conv_b": 1, "dense_W": 14, "dense_b": 15, "head_W": 16, "head_b": 17}
        self.shapes = {"conv_K": (kh, kw, 1, F), "conv_b": (F,), "dense_W": tuple(Wd.shape), "dense_b": (E,), "head_W": tuple(Wh.shape),
                       "head_b": (self.n_class,)}
        self.has_bias = {"conv_b": bc is not None, "dense_b": bd is not None, "head_b": bh is not None}
        for i, (W, U, b) in enumerate(layers[:self.MAX_LAYERS]):
            for j, (n, a) in enumerate((("W", W), ("U", U), ("b", b))):
                self.TENSOR["gru%d_%s" % (i, n)] = 2 + 3 * i + j
                self.shapes["gru%d_%s" % (i, n)] = (3 * self.units[i],) if n == "b" else tuple(a.shape)
            self.has_bias["gru%d_b" % i] = b is not None
        n = len(layers)
        c_units = (C.c_int32 * n)(*self.units)
        c_w = (C.c_void_p * n)(*[W.ctypes.data for W, _, _ in layers])
        c_u = (C.c_void_p * n)(*[U.ctypes.data for _, U, _ in layers])
        c_b = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for _, _, b in layers])
        self._create(self._lib.ssp_gru_trainer_create, ctx._h, self.T, self.D, kh, kw, F, sh, sw, K.ctypes.data, _raw_ptr(bc, _lib.HOST), n, c_units,
                     c_w, c_u, c_b, E, Wd.ctypes.data, _raw_ptr(bd, _lib.HOST), self.n_class, Wh.ctypes.data, _raw_ptr(bh, _lib.HOST),
                     GRU_ACTIVATIONS[recurrent_activation], 1 if reset_after else 0, int(max_batch))

    STEP_KINDS = ("conv forward", "mean+dense+l2+head", "loss+regulariser", "head+l2+dense+mean backward", "conv backward", "adam+repack")
    LAYER_KINDS = ("projection", "forward steps", "backward steps", "dW+db", "dU", "dx")

    def step_times(self, X, labels, batch_size: int = 128, lr: float = 1e-4):
        """ONE training step on the first ``batch_size`` rows of torch CUDA tensors with a hipEvent between its launch kinds ->
        {kind: milliseconds}; the 2 To step launches of a layer and direction are one figure, 'gru{i} forward steps' / 'backward steps'
        (a measurement aid: the step counts like any other)"""
        keep, xp, lp, N, where = self._data(X, labels)
        if where != _lib.DEVICE or N < int(batch_size):
            raise ValueError("step_times takes torch CUDA tensors of at least batch_size rows")
        ms = (C.c_float * 30)()
        with self.ctx._ordered(where):
            _lib.check(self._lib.ssp_gru_trainer_step_times(self._h, xp, lp, int(batch_size), float(lr), ms))
        out = dict(zip(self.STEP_KINDS, (float(v) for v in ms[:6])))
        for i in range(self.n_gru):
            for j, k in enumerate(self.LAYER_KINDS):
                out["gru%d %s" % (i, k)] = float(ms[6 + 6 * i + j])
        return out

    def _name(self, what):
        if what in self.TENSOR:
            return "", what
        if what[:1] in ("d", "m", "v") and what[1:] in self.TENSOR:
            return what[:1], what[1:]
        raise ValueError("unknown tensor %r" % (what,))

    def read(self, what: str, out=None):
        """a tensor name (parameters), or one with a prefix 'd' (the last step's gradients), 'm' or 'v' (Adam's moments), e.g. 'dgru0_U',
        'mhead_W' -> numpy; ``out``: a float32 array of the tensor's size to fill instead (it needs 4-byte alignment only)"""
        prefix, name = self._name(what)
        out = self._read_into(name, out)
        _lib.check(self._lib.ssp_gru_trainer_read(self._h, self.WHAT[prefix], self.TENSOR[name], out.ctypes.data))
        return out


def _gru_vec(b, n, what):
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    if b.shape[0] != n:
        raise ValueError("%s must have %d entries" % (what, n))
    return b


def cosine_identify(ctx: Context, X, Cn, dist: bool = False, argmin: bool = True, minval: bool = True,
                    timing: bool = False, precision: int = 0, counts: bool = True) -> dict:
    """dist[i,j] = clip(1 - cos(X[i], C[j]), 0, 2); argmin over j (first index on ties) — d_vector.py:315-319.
    precision 0: fp32 MFMA (parity path).  precision 1: bf16x3 MFMA sweep + fp32 re-scoring of the rows whose two best cosines are
    closer than twice a proven error bound (3.01 * 2^-16 + 4 d 2^-23 1.02 + (d + 8) 2^-24: 1.9e-4 at d = 256; bf16's unit roundoff is
    2^-8) — the arg-min of the fp32 path on every row, about 3x faster; no distance matrix (dist=False); the result then carries
    "rescored" (rows that went through fp32 again).  precision 2: a bf16 sweep in front (bound 2.01 * 2^-8 + 2 d 2^-23 1.01 +
    (d + 8) 2^-24 = 7.9e-3), its close calls to the bf16x3 sweep: same arg-min guarantee, the minimum only within 7.9e-3 on rows the
    first sweep decided.
    precision 3 or "auto": the fp32 path's arg-min at the cost of the cheapest of 2, 1 and 0 — a pilot on the first ~2 % of the rows
    reads how many each sweep would hand on (one host wait); the result carries "auto" (what it chose and saw).
    ``counts=False`` skips the "rescored" / "split_rows" diagnostics: with CUDA tensors the call then returns without waiting for the GPU."""
    if precision == "auto":
        precision = 3
    xk, xp, where = _as_f32(X, "X")
    ck, cp, cwhere = _as_f32(Cn, "C")
    if cwhere != where:
        raise ValueError("X and C must both be numpy arrays or both be torch CUDA tensors")
    if xk.ndim != 2 or ck.ndim != 2 or xk.shape[1] != ck.shape[1]:
        raise ValueError("X (N,d) and C (S,d) must share d")
    N, d = int(xk.shape[0]), int(xk.shape[1])
    S = int(ck.shape[0])
    dm = ctx._empty((N, S), where) if dist else None
    am = ctx._empty((N,), where, "int32") if argmin else None
    mv = ctx._empty((N,), where) if minval else None
    ms = ctx._run(ctx._lib.ssp_cosine_identify2, where, timing, ctx._h, xp, N, d, cp, S, _raw_ptr(dm, where), _raw_ptr(am, where), _raw_ptr(mv, where),
                  where, int(precision))
    res = {}
    if precision == 3:
        a, b, c, e = C.c_int32(-1), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(ctx._lib.ssp_cosine_last_auto(ctx._h, C.byref(a), C.byref(b), C.byref(c), C.byref(e)))
        res["auto"] = {"precision_used": a.value, "pilot_rows": b.value, "pilot_to_bf16x3": c.value, "pilot_to_fp32": e.value}
    if precision >= 1 and counts:
        res["rescored"] = _read_int(C.c_int32, ctx._lib.ssp_cosine_last_rescored, ctx._h)
        res["split_rows"] = _read_int(C.c_int32, ctx._lib.ssp_cosine_last_split_rows, ctx._h)   # precision 2: rows the bf16 sweep handed on
    res.update(_result(timing, ms, dist=dm, argmin=am, min=mv))
    return res
