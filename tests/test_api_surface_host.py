"""Host tests of the Python binding layer (speech_signal_processing_amd/api.py): its surface and its plumbing helpers.  No GPU, no library.

The surface: tests/golden/api_surface.json holds, for every module-level name api defines, a function's signature and docstring, a class's
docstring and the kind and signature of its members, a constant's repr — and the destroy symbol every handle class calls.  It was
recorded before the handle base and the call path were factored out; every recorded entry must still be there and equal (new private
helpers may appear).  ``python tests/test_api_surface_host.py --record`` writes the file again: only for a change of the surface that
is meant.

The helpers (_Handle, Context._run, _raw_ptr, _result) run against a stub library that records (symbol, arguments) and returns a
chosen code."""
import ctypes as C
import inspect
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from speech_signal_processing_amd import _lib, api  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "api_surface.json")
HANDLE_CLASSES = ("Context", "Segments", "MfccPlan", "GmmScorer", "GmmFullScorer", "MapScorer", "IvectorExtractor", "PldaScorer",
                  "DnnForward", "LstmForward", "GruForward", "XVectorForward", "DnnTrainer", "LstmTrainer", "GruTrainer")
KEPT_PRIVATE = ("_is_torch", "_as_recordings", "_gru_arrays", "_cfg_struct", "_dtw_direction_bytes", "_raw_ptr")
KEPT_MEMBERS = (("Context", "_empty"), ("Context", "_ordered"))


class StubLib:
    """stands in for the loaded library: every symbol records its call and returns ``rc``; a kernel_ms pointer receives ``ms``"""

    def __init__(self, rc=0, ms=1.5, raises=None):
        self.rc, self.ms, self.raises, self.calls = rc, ms, raises, []

    def ssp_last_error(self):
        return b"stub error"

    def __getattr__(self, symbol):
        def call(*args):
            self.calls.append((symbol, args))
            if self.raises is not None:
                raise self.raises
            if args and hasattr(args[-1], "_obj") and isinstance(args[-1]._obj, C.c_float):   # byref(c_float): the kernel_ms argument
                args[-1]._obj.value = self.ms
            return self.rc
        return call


def _handle(cls, lib, **attrs):
    """an instance made without __init__: the library, a handle and whatever else the test names"""
    obj = object.__new__(cls)
    obj._lib = lib
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


# ------------------------------------------------------------------------------------------------------------------------- the snapshot
def _member(cls, name):
    m = inspect.getattr_static(cls, name)
    if isinstance(m, property):
        return {"kind": "property", "signature": str(inspect.signature(m.fget))}
    if isinstance(m, (classmethod, staticmethod)):
        return {"kind": type(m).__name__, "signature": str(inspect.signature(m.__func__))}
    if inspect.isfunction(m):
        return {"kind": "function", "signature": str(inspect.signature(m))}
    if inspect.ismethoddescriptor(m):
        return None   # (what ``object`` itself gives a class that defines no __init__ / __del__ of its own: not a member of api)
    return {"kind": "constant", "repr": repr(m)}


def _destroy_symbol(cls):
    lib = StubLib()
    _handle(cls, lib, _h=C.c_void_p(1)).close()
    assert len(lib.calls) == 1, (cls.__name__, lib.calls)
    return lib.calls[0][0]


def snapshot():
    entries = {}
    for name, v in sorted(vars(api).items()):
        if name.startswith("__"):
            continue
        if inspect.isfunction(v) and v.__module__ == api.__name__:
            entries[name] = {"type": "function", "signature": str(inspect.signature(v)), "doc": inspect.getdoc(v)}
        elif inspect.isclass(v) and v.__module__ == api.__name__:
            names = [n for n, _ in inspect.getmembers(v) if not (n.startswith("__") and n.endswith("__")) or n in ("__init__", "__del__")]
            members = {n: _member(v, n) for n in names}
            entries[name] = {"type": "class", "doc": inspect.getdoc(v), "members": {n: m for n, m in members.items() if m is not None}}
        elif type(v) in (int, float, str, tuple, dict):
            entries[name] = {"type": "constant", "repr": repr(v)}
    return {"entries": entries, "destroy": {n: _destroy_symbol(getattr(api, n)) for n in HANDLE_CLASSES}}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_recorded_name_is_still_there_and_equal(recorded):
    now = snapshot()["entries"]
    for name, want in recorded["entries"].items():
        assert name in now, "api.%s is gone" % name
        got = now[name]
        if want["type"] == "class":
            assert got["type"] == "class" and got["doc"] == want["doc"], name
            for m, w in want["members"].items():
                assert got["members"].get(m) == w, "api.%s.%s: %r, recorded %r" % (name, m, got["members"].get(m), w)
        else:
            assert got == want, "api.%s: %r, recorded %r" % (name, got, want)


def test_the_fixture_covers_the_names_other_files_use(recorded):
    ent = recorded["entries"]
    for name in KEPT_PRIVATE + HANDLE_CLASSES:
        assert name in ent, name
    for cls, m in KEPT_MEMBERS:
        assert m in ent[cls]["members"], (cls, m)
    assert set(recorded["destroy"]) == set(HANDLE_CLASSES)
    assert len(ent) >= 100 and sum(len(e.get("members", ())) for e in ent.values()) >= 140


# --------------------------------------------------------------------------------------------------------------------------- the handles
@pytest.mark.parametrize("name", HANDLE_CLASSES)
def test_close_calls_the_recorded_destroy_symbol_once(name, recorded):
    lib, h = StubLib(), C.c_void_p(7)
    obj = _handle(getattr(api, name), lib, _h=h)
    obj.close()
    assert [s for s, _ in lib.calls] == [recorded["destroy"][name]] and lib.calls[0][1] == (h,)
    assert recorded["destroy"][name] in _lib.SIGNATURES
    assert obj._h is None
    obj.close()
    assert len(lib.calls) == 1, "a second close() called the library"


@pytest.mark.parametrize("name", HANDLE_CLASSES)
def test_close_on_a_half_constructed_object_calls_nothing(name):
    lib = StubLib()
    obj = _handle(getattr(api, name), lib)   # __init__ raised before the handle was made
    obj.close()
    obj.__del__()
    object.__new__(getattr(api, name)).__del__()   # not even the library: still silent
    assert lib.calls == []


@pytest.mark.parametrize("name", HANDLE_CLASSES)
def test_del_swallows_a_destroy_that_raises(name):
    lib = StubLib(raises=RuntimeError("the context went first"))
    obj = _handle(getattr(api, name), lib, _h=C.c_void_p(7))
    obj.__del__()
    assert len(lib.calls) == 1
    with pytest.raises(RuntimeError):
        obj.close()   # close() itself does not hide it
    obj._h = None     # (nothing left for the collector to do)


def test_a_handle_is_stored_only_when_its_create_call_succeeds(monkeypatch):
    lib = StubLib(rc=-1)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    obj = _handle(api.GmmScorer, lib)
    with pytest.raises(ValueError):
        obj._create(lib.ssp_gmm_pack, 1, 2)
    assert not hasattr(obj, "_h")
    lib.rc = 0
    obj._create(lib.ssp_gmm_pack, 1, 2)
    sym, args = lib.calls[-1]
    assert sym == "ssp_gmm_pack" and args[:2] == (1, 2) and len(args) == 3 and args[2]._obj is obj._h   # byref(h) last
    obj._h = None


# ------------------------------------------------------------------------------------------------------------------------- the call path
def _context(lib):
    return _handle(api.Context, lib, _h=C.c_void_p(3), device=0, stream=None)


def test_run_passes_null_without_timing_and_returns_what_the_library_wrote_with_it():
    lib = StubLib(ms=2.25)
    ctx = _context(lib)
    assert ctx._run(lib.ssp_cmvn, _lib.HOST, False, 1, "a") == 0.0
    assert lib.calls[-1] == ("ssp_cmvn", (1, "a", None))
    assert ctx._run(lib.ssp_cmvn, _lib.HOST, True, 1, "a") == 2.25
    sym, args = lib.calls[-1]
    assert args[:2] == (1, "a") and isinstance(args[2]._obj, C.c_float)
    assert [s for s, _ in lib.calls] == ["ssp_cmvn", "ssp_cmvn"], "a host call needs no stream ordering"
    ctx._h = None


@pytest.mark.parametrize("rc,exc", [(-1, ValueError), (-2, NotImplementedError), (-3, _lib.SspError), (5, _lib.SspError)])
def test_run_raises_by_the_return_code(monkeypatch, rc, exc):
    lib = StubLib(rc=rc)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ctx = _context(lib)
    with pytest.raises(exc, match="stub error"):
        ctx._run(lib.ssp_cmvn, _lib.HOST, True, 1)
    assert [s for s, _ in lib.calls] == ["ssp_cmvn"]
    ctx._h = None


def test_run_signals_the_stream_when_a_device_call_fails(monkeypatch):
    """the check runs inside _ordered: its ``finally`` still hands the results' stream back"""
    lib = StubLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(api, "_current_raw_stream", lambda device: 0x50)
    ctx = _context(lib)   # (owns its stream: ordered against torch's current one)

    def failing(*args):
        lib.calls.append(("ssp_cmvn", args))
        return -1
    with pytest.raises(ValueError):
        ctx._run(failing, _lib.DEVICE, False, 1)
    assert [s for s, _ in lib.calls] == ["ssp_ctx_wait_stream", "ssp_cmvn", "ssp_ctx_signal_stream"]
    ctx._h = None


# -------------------------------------------------------------------------------------------------------- addresses and returned dicts
def test_raw_ptr_of_none_is_none_on_both_sides():
    assert api._raw_ptr(None, _lib.HOST) is None and api._raw_ptr(None, _lib.DEVICE) is None
    import numpy as np
    a = np.zeros(3, dtype=np.float32)
    assert api._raw_ptr(a, _lib.HOST) == a.ctypes.data


def test_result_drops_none_and_adds_kernel_ms_only_when_asked():
    assert api._result(False, 3.0, a=1, b=None, c=0) == {"a": 1, "c": 0}
    r = api._result(True, 3.0, a=1, b=None)
    assert r == {"a": 1, "kernel_ms": 3.0} and list(r) == ["a", "kernel_ms"]
    assert list(api._result(False, 0.0, z=1, y=2, x=3)) == ["z", "y", "x"]


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        with open(FIXTURE, "w") as f:
            json.dump(snapshot(), f, indent=1, sort_keys=True)
            f.write("\n")
        s = snapshot()["entries"]
        print("%d entries, %d class members" % (len(s), sum(len(e.get("members", ())) for e in s.values())))
