"""A producer kept in flight across a library call, for the stream-ordering tests (tests/test_gpu_stream_order.py; an ordinary module
like tests/skewed.py).

The other GPU tests hand the library inputs that are at rest, on torch's default stream.  ``Config.race`` makes one call of one entry
point twice on a non-default, non-blocking torch stream S (torch.cuda.Stream()):

  baseline     inputs on the device, torch.cuda.synchronize(), the call, synchronize, outputs to numpy.  The baseline's device outputs stay
               alive until the case ends, so the caching allocator cannot hand the racing run a block that already holds the answer.
  racing run   1. every device input buffer holds POISON, every output the caller owns NaN / an impossible integer; for every output
                  the api allocates itself a tensor of the same size is allocated on S, poisoned and freed again (the allocator
                  most likely returns that block); synchronize
               2. a delay is queued on S (torch.cuda._sleep; without it a chain of matrix products timed with two events)
               3. buf.copy_(real) for every input on S — device to device, from tensors staged before —, then event E is recorded
               4. the library call, with no host wait in between
               5. out.clone() on S for every output, straight after the call has returned
               6. synchronize: the clones equal the baseline bit for bit (np.array_equal, NaN pattern included)

The delay is proven per run, not assumed: E.query() is False immediately before the call and — for a call that returns without a host
wait — still False immediately after it; otherwise the delay doubles and the run is repeated, up to CAP_MS.  Reaching the cap fails
the test ("could not keep the producer in flight").  The delay finally used is printed as ``[measured] ... delay ms``.

Poison never indexes memory: NaN for float data, 12345 for int16 PCM, and for integer inputs that ARE indices (the labels of
``centroids``) the caller passes a wrong but in-range array.  A detected race is a wrong number, nothing more.

Calls that take HOST arrays and move them through torch themselves (the d_vector networks' numpy route) have no device input to hold
back; ``Config.race_host`` keeps the stream the library runs on busy instead and compares the returned arrays with the baseline.

Three configurations (``MODES``):
  owned             api.Context(0): the library's own stream; producer and consumer on S
  borrowed-current  api.Context.for_torch() built while S is current: the library runs on S itself — work the C side queues on any
                    other stream races
  borrowed-stale    api.default_context(torch_stream=True), which borrowed torch's default stream, called while S is current
"""
import numpy as np

MODES = ("owned", "borrowed-current", "borrowed-stale")
START_MS = 5.0
CAP_MS = 200.0
PCM_POISON = 12345
INT_OUT_POISON = {"int32": -7, "uint8": 77, "int16": -7, "int64": -7}

_STREAMS = {}
_DELAY = {}


def stream(which="S"):
    """the side streams of this process: "S" for producers and consumers, "other" for the negative control (and nothing else)"""
    import torch
    if which not in _STREAMS:
        _STREAMS[which] = torch.cuda.Stream()
        assert _STREAMS[which].cuda_stream != torch.cuda.default_stream().cuda_stream
    return _STREAMS[which]


def _calibrate():
    """-> ("sleep", cycles per ms) or ("mm", products per ms, operands): measured once with two events on S"""
    import torch
    if "kind" in _DELAY:
        return
    s = stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)   # (first launch)
            n = 2_000_000
            e0.record(s)
            torch.cuda._sleep(n)
            e1.record(s)
            e1.synchronize()
            _DELAY.update(kind="sleep", per_ms=n / max(e0.elapsed_time(e1), 1e-3))
        else:
            a = torch.full((1024, 1024), 1.0 / 1024, device="cuda")
            b, c = a.clone(), torch.empty_like(a)
            torch.mm(a, b, out=c)
            n = 200
            e0.record(s)
            for _ in range(n):
                torch.mm(a, b, out=c)
            e1.record(s)
            e1.synchronize()
            _DELAY.update(kind="mm", per_ms=n / max(e0.elapsed_time(e1), 1e-3), ops=(a, b, c))
    print("[measured] delay source %s: %.4g units per ms" % (_DELAY["kind"], _DELAY["per_ms"]))


def queue_delay(ms):
    """about ``ms`` milliseconds of work on torch's current stream, queued without a host wait and without an allocation"""
    import torch
    _calibrate()
    n = max(1, int(ms * _DELAY["per_ms"]))
    if _DELAY["kind"] == "sleep":
        torch.cuda._sleep(n)
    else:
        a, b, c = _DELAY["ops"]
        for _ in range(n):
            torch.mm(a, b, out=c)


def poison_like(t, value=None):
    """a fresh tensor of t's shape and type holding poison (inputs: NaN / PCM_POISON / ``value``; outputs: NaN / INT_OUT_POISON)"""
    import torch
    p = torch.empty_like(t)
    if value is not None:
        p.copy_(value)
    elif t.dtype.is_floating_point:
        p.fill_(float("nan"))
    elif t.dtype == torch.int16:
        p.fill_(PCM_POISON)
    else:
        p.fill_(INT_OUT_POISON[str(t.dtype).split(".")[1]])
    return p


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def to_numpy(res):
    return {k: (v.cpu().numpy() if _is_tensor(v) else np.array(v, copy=True)) for k, v in res.items()}


def same_bits(got, base, what):
    assert set(got) == set(base), (what, sorted(got), sorted(base))
    for k in sorted(base):
        g, b = np.asarray(got[k]), np.asarray(base[k])
        assert g.dtype == b.dtype and g.shape == b.shape, (what, k, g.dtype, b.dtype, g.shape, b.shape)
        if not np.array_equal(g, b, equal_nan=g.dtype.kind == "f"):
            bad = np.flatnonzero(~((g == b) | ((g != g) & (b != b))).reshape(-1))
            raise AssertionError("%s: %s differs from the call on inputs at rest on %d of %d elements, the first at flat index %d (%r against %r)" % (
                what, k, bad.size, b.size, bad[0], g.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]]))


class Config:
    """one of MODES: the library context, the stream S and a cache for what is built on that context (plans, scorers, segments)"""

    def __init__(self, mode):
        import torch
        from speech_signal_processing_amd import api, _lib
        assert mode in MODES, mode
        self.mode, self.torch, self.api, self._lib = mode, torch, api, _lib
        self.S = stream()
        self.cache = {}
        self._own_ctx = mode != "borrowed-stale"
        if mode == "owned":
            self.ctx = api.Context(0)
            assert self.ctx.stream is None
        elif mode == "borrowed-current":
            with torch.cuda.stream(self.S):
                self.ctx = api.Context.for_torch()
            assert self.ctx.stream == self.S.cuda_stream
        else:
            assert torch.cuda.current_stream().cuda_stream == torch.cuda.default_stream().cuda_stream
            self.ctx = api.default_context(torch_stream=True)   # (the one the d_vector networks take)
            assert self.ctx.stream == torch.cuda.default_stream().cuda_stream, "the cached context was first made on a side stream"

    def cached(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def close(self):
        self.torch.cuda.synchronize()
        self.cache.clear()
        if self._own_ctx:
            self.ctx.close()

    def library_stream(self):
        """the torch stream object the library's kernels run on, where torch knows it (None for a stream the library owns)"""
        torch = self.torch
        if self.mode == "owned":
            return None
        return self.S if self.mode == "borrowed-current" else torch.cuda.default_stream()

    # ------------------------------------------------------------------------------------------------------------------ device inputs
    def race(self, what, inputs, call, outs=None, poison=None, waits=False):
        """inputs: name -> numpy array (the device inputs of the call); outs: name -> (shape, torch dtype name) for outputs the caller
        owns; poison: name -> numpy array for inputs that must not take the default poison; waits: the call waits on the host (E may
        have fired when it returns).  call(dev_inputs, dev_outs) -> name -> tensor or numpy array.  Returns the baseline as numpy."""
        torch = self.torch
        outs, poison = outs or {}, poison or {}
        what = "%s [%s]" % (what, self.mode)
        with torch.cuda.stream(self.S):
            real = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inputs.items()}
            bad = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in poison.items()}
            for k, v in bad.items():
                assert v.shape == real[k].shape and v.dtype == real[k].dtype and not torch.equal(v, real[k]), (what, k)

            def fresh_outs():
                return {k: poison_like(torch.empty(tuple(shape), dtype=getattr(torch, dt), device="cuda")) for k, (shape, dt) in outs.items()}
            base_in, base_out = {k: v.clone() for k, v in real.items()}, fresh_outs()
            torch.cuda.synchronize()
            base_dev = call(base_in, base_out)
            torch.cuda.synchronize()
            base = to_numpy(base_dev)
            owned_ptrs = {t.data_ptr() for t in base_out.values()}
            delay = START_MS
            while True:
                bufs = {k: poison_like(v, bad.get(k)) for k, v in real.items()}
                run_out = fresh_outs()
                junk = [poison_like(v) for v in base_dev.values() if _is_tensor(v) and v.data_ptr() not in owned_ptrs]
                torch.cuda.synchronize()
                del junk
                queue_delay(delay)
                for k, b in bufs.items():
                    b.copy_(real[k])
                E = torch.cuda.Event()
                E.record(self.S)
                q0 = E.query()
                got_dev = call(bufs, run_out)
                q1 = E.query()
                clones = {k: (v.clone() if _is_tensor(v) else v) for k, v in got_dev.items()}
                torch.cuda.synchronize()
                if not q0 and (waits or not q1):
                    break
                assert delay < CAP_MS, "%s: could not keep the producer in flight: with a delay of %g ms the event had fired %s the call%s" % (
                    what, delay, "before" if q0 else "after", "" if q0 else ", which is held to return without a host wait")
                delay = min(2 * delay, CAP_MS)
                del bufs, run_out, got_dev, clones
            print("[measured] %s: delay %g ms%s" % (what, delay, "" if not q1 else " (the call waited on the host)"))
            same_bits(to_numpy(clones), base, what)
            del base_dev
        return base

    # -------------------------------------------------------------------------------------------------------------------- host inputs
    def race_host(self, what, call, out_sizes):
        """call() takes host arrays, moves them through torch on the current stream (S) and returns numpy arrays (or anything ==
        compares): with the library's stream kept busy for ``delay`` ms, what comes back equals the baseline.  out_sizes: element
        counts of the float32 device outputs the route allocates on S (poisoned and freed before the call)."""
        torch = self.torch
        what = "%s [%s]" % (what, self.mode)
        lib = self.library_stream()
        assert lib is not None and lib.cuda_stream != self.S.cuda_stream, "race_host needs a library stream torch can queue on, other than S"
        with torch.cuda.stream(self.S):
            torch.cuda.synchronize()
            base = call()
            torch.cuda.synchronize()
            delay = START_MS
            while True:
                junk = [torch.full((int(n),), float("nan"), device="cuda") for n in out_sizes]
                torch.cuda.synchronize()
                del junk
                with torch.cuda.stream(lib):
                    queue_delay(delay)
                    E = torch.cuda.Event()
                    E.record(lib)
                q0 = E.query()
                got = call()
                torch.cuda.synchronize()
                if not q0:
                    break
                assert delay < CAP_MS, "%s: could not keep the library's stream busy: %g ms had passed before the call" % (what, delay)
                delay = min(2 * delay, CAP_MS)
            print("[measured] %s: delay %g ms (host route)" % (what, delay))
        return base, got


def negative_control():
    """The racing pattern with no library in it: the consumer is ``buf * 1`` on a second stream that does not wait for S.  It must see
    the poison; returns (saw poison, delay ms).  If it does not, this harness cannot detect a race."""
    import torch
    S, other = stream(), stream("other")
    real = torch.arange(1, 4097, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    delay = START_MS
    while True:
        with torch.cuda.stream(S):
            buf = poison_like(real)
            torch.cuda.synchronize()
            queue_delay(delay)
            buf.copy_(real)
            E = torch.cuda.Event()
            E.record(S)
            q0 = E.query()
        with torch.cuda.stream(other):
            seen = buf * 1
        q1 = E.query()
        torch.cuda.synchronize()
        if not q0 and not q1:
            break
        assert delay < CAP_MS, "negative control: could not keep the producer in flight with a delay of %g ms" % delay
        delay = min(2 * delay, CAP_MS)
    print("[measured] negative control: delay %g ms" % delay)
    assert torch.equal(buf, real)   # (the producer itself did arrive)
    return bool(torch.isnan(seen).all()), delay
