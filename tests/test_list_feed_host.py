"""Host side of the list-fed entry points, no GPU: the copying threads' pool (csrc/staging.hpp, WorkPoolT and the copy pieces) under
ThreadSanitizer, and the pointer-table builder api.list_table (dtype rule, keep-alive, contiguity)."""
import os
import platform
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_pool_under_thread_sanitizer(tmp_path):
    """Four threads, each with its own pool resized between batches, run random spans (copies, widening, narrowing) in pieces of random
    size: no report from ThreadSanitizer, every destination byte right, nothing written past a span."""
    exe = str(tmp_path / "gather_pool_tsan")
    src = os.path.join(ROOT, "tests", "native", "gather_pool_threads.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", src, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    cmd = [exe, "4", "300"]
    setarch = shutil.which("setarch")   # (TSan's shadow layout needs the default ASLR entropy: test_host.py's staging-pool test does the same)
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        cmd = [setarch, platform.machine(), "-R", *cmd]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0:report_signal_unsafe=0"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "mismatches 0" in r.stdout


def _addr(a):
    return a.__array_interface__["data"][0]


def test_list_table_samples_dtype_rule_and_keep_alive():
    from speech_signal_processing_amd import api
    rng = np.random.default_rng(0)
    a = rng.integers(-3000, 3000, 1000).astype(np.int16)
    b = rng.integers(-3000, 3000, 1554).astype(np.int16)
    tab, keep, typ = api.list_table([a, b.reshape(-1, 1)])
    assert typ == 1 and tab.dtype == np.uintp and tab.shape == (2,)
    assert tab[0] == _addr(a) and np.shares_memory(keep[1], b)              # int16 arrays are read where they are
    assert [k.shape for k in keep] == [(1000,), (1554,)]
    strided = b[::2]
    tab, keep, typ = api.list_table([a, strided])                           # a non-contiguous array is copied, that one alone
    assert typ == 1 and tab[0] == _addr(a) and keep[1].flags.c_contiguous and not np.shares_memory(keep[1], b)
    assert np.array_equal(keep[1], strided) and tab[1] == _addr(keep[1])
    f64 = rng.standard_normal(777)
    tab, keep, typ = api.list_table([a, f64])                               # mixed: float32 for every array, as flatten_signals
    flat, _ = api.flatten_signals([a, f64])
    assert typ == 0 and all(k.dtype == np.float32 for k in keep)
    assert np.array_equal(np.concatenate(keep), flat)
    assert [_addr(k) for k in keep] == list(tab)                            # the table points into the kept arrays
    tab, keep, typ = api.list_table([])
    assert typ == 0 and tab.shape == (0,) and keep == []
    tab, keep, typ = api.list_table([np.zeros(0, np.int16), a])
    assert typ == 1 and [k.shape[0] for k in keep] == [0, 1000]


def test_list_table_rows_follow_vstack_astype():
    from speech_signal_processing_amd import api
    rng = np.random.default_rng(1)
    f64 = [rng.standard_normal((int(t), 5)) for t in (3, 0, 7)]
    tab, keep, typ = api.list_table(f64, "rows")
    assert typ == 1 and [_addr(k) for k in keep] == [_addr(f) for f in f64]   # float64 rows: narrowed by the library, not copied here
    f32 = [f.astype(np.float32) for f in f64]
    tab, keep, typ = api.list_table(f32, "rows")
    assert typ == 0 and tab[0] == _addr(f32[0])
    tab, keep, typ = api.list_table([f32[0], f64[2]], "rows")               # float32 + float64: float64, as vstack promotes
    assert typ == 1 and all(k.dtype == np.float64 for k in keep)
    ints = [rng.integers(-2**40, 2**40, (4, 5)), rng.integers(-5, 5, (2, 5)).astype(np.int32)]
    tab, keep, typ = api.list_table(ints, "rows")                           # another common type: converted as vstack + astype would
    assert typ == 0 and np.array_equal(np.concatenate(keep), np.vstack(ints).astype(np.float32))
    fortran = np.asfortranarray(rng.standard_normal((6, 5)))
    tab, keep, typ = api.list_table([fortran], "rows")
    assert keep[0].flags.c_contiguous and np.array_equal(keep[0], fortran) and tab[0] == _addr(keep[0])
