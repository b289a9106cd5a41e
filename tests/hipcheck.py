"""Shared helpers for the -m gpu parity tests: run a module through the C-ABI of libansel_hip
on device 0 and through the CPU checkers (tests/checkers.py) on the same seeded input."""
import contextlib
import ctypes as C

import numpy as np

import checkers as ck
from ansel_amd import abi, lib

_state = {}


def hip():
    if "lib" not in _state:
        _state["lib"] = lib.init()  # raises loudly when the .so or the GPU is missing
        pool_fill_default()
    return _state["lib"]


def pool_fill_default():
    """the allocator's poison as the process runs: off, or -- ANSEL_TEST_POOL_FILL=<hex>, read once -- on with that word for
    every test of the process (a one-time pass of the whole suite under poison; lib.init() switches it on from the same
    variable, so a test file that never comes through hip() runs under it as well)"""
    _state["fill"] = lib.env_pool_fill()
    lib.test_pool_fill(0, _state["fill"] is not None, _state["fill"] or 0)


@contextlib.contextmanager
def pool_fill(pattern):
    """every block the runtime's pool hands out inside the `with` holds the 32-bit `pattern` in each word (the modules'
    scratch and lib.DeviceBuffer alike); what held before -- off, or an outer pattern -- is back afterwards"""
    hip()
    before = _state.get("fill")
    was_on = lib.test_pool_fill(0, True, pattern)
    assert was_on == (before is not None)
    _state["fill"] = int(pattern) & 0xFFFFFFFF
    try:
        yield
    finally:
        _state["fill"] = before
        lib.test_pool_fill(0, before is not None, before or 0)


def allocated_bytes():
    """what device 0 holds of the runtime's pool at this moment (lib.DeviceBuffer draws from the same pool)"""
    cur, peak = C.c_size_t(0), C.c_size_t(0)
    hip().dt_hip_memory_statistics(0, C.byref(cur), C.byref(peak))
    return cur.value


def run_hip(fn_name, piece, data, inp, out_shape, out_dtype=np.float32, pre_fill=None):
    """upload `inp`, call dt_hip_iop_<fn>_process(devid 0, piece, data, in, out), download"""
    h = hip()
    din = lib.DeviceBuffer.from_numpy(0, inp)
    out_nbytes = int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize
    if pre_fill is not None:
        dout = lib.DeviceBuffer.from_numpy(0, pre_fill)
    else:
        dout = lib.DeviceBuffer.from_numpy(0, np.zeros(out_shape, dtype=out_dtype))
    fn = getattr(h, fn_name)
    base = allocated_bytes()
    rc = fn(0, C.byref(piece), C.byref(data), din.ptr, dout.ptr)
    finished = h.dt_hip_finish(0)
    # whatever the module took from the runtime's pool is back in it, also where it refuses the call
    left = allocated_bytes() - base
    assert left == 0, "%s (rc %d) holds %d bytes of the pool after it returned" % (fn_name, rc, left)
    lib.check(rc, fn_name)
    assert finished == 1, h.dt_hip_last_error()
    out = dout.to_numpy(out_shape, out_dtype)
    din.release()
    dout.release()
    return out


def run_cpu(which, name, piece, data, inp, out_shape, out_dtype=np.float32, pre_fill=None):
    """which: 'ref' (the reference's own code, oracle/_ref) or 'oracle' (restatement); pre_fill: what the output holds
    before the call, as in run_hip() (default: zeros)"""
    l = ck.ref() if which == "ref" else ck.oracle()
    if l is None:
        return None
    out = np.zeros(out_shape, dtype=out_dtype) if pre_fill is None else np.array(pre_fill, dtype=out_dtype, order="C")
    rc = ck.call(l, ("ref_" if which == "ref" else "oracle_") + name, piece, data, np.ascontiguousarray(inp), out)
    assert rc == 0
    return out


def assert_bit_exact(a, b, what, mask=None):
    d = ck.ulp_diff(a, b) if a.dtype == np.float32 else (a.astype(np.int64) != b.astype(np.int64)).astype(np.int64)
    if mask is not None:
        d = d * (mask == 0)
    n = int((d > 0).sum())
    assert n == 0, "%s: %d of %d values differ, max %d ulp" % (what, n, d.size, int(d.max()))


def checkers_available():
    out = []
    if ck.ref() is not None:
        out.append("ref")
    if ck.oracle() is not None:
        out.append("oracle")
    return out
