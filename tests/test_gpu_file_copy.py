"""-m gpu: dt_hip_read_file_to_host() (file_copy.hip) on synthetic file buffers.

  * for every total of file_copy_ref.TOTALS (8 .. 49, 2^6 .. 2^22 at their -1 / 0 / +1 edges) the pinned host buffer equals
    what the host twin leaves, byte for byte, guards included -- with capacity == host_bytes == T, and with both large
  * a host buffer one byte short gets the true L and nothing else; a device word of UINT64_MAX arrives as UINT64_MAX alone
  * an unpinned buffer, a misaligned one and one of 4 bytes are DT_HIP_INVALID_ARG with a reason, and stay untouched"""
import ctypes as C

import numpy as np
import pytest

import file_copy_ref as fr
import hipcheck as hc
from ansel_amd import abi, lib

pytestmark = pytest.mark.gpu

BIG = max(fr.TOTALS) + 4096  # "both large": more than any total


class _Bench:
    """one device buffer and one pinned buffer for every case: GUARD + BIG + GUARD bytes, the host buffer behind the
    first guard (64 bytes: still 16-byte aligned)"""

    def __init__(self):
        self.l = hc.hip()
        self.dev = lib.DeviceBuffer(0, BIG)
        self.nbytes = fr.GUARD + BIG + fr.GUARD
        self.pin = self.l.dt_hip_alloc_host_pinned(self.nbytes)
        assert self.pin
        self.host = np.ctypeslib.as_array(C.cast(self.pin, C.POINTER(C.c_uint8)), (self.nbytes,))

    def close(self):
        self.dev.release()
        self.l.dt_hip_free_host_pinned(self.pin)

    def read(self, src, capacity, host_bytes):
        """the device's copy of `src` (capacity bytes) into the pinned buffer filled with FILL -> rc, its first
        GUARD + host_bytes + GUARD bytes"""
        n = fr.GUARD + host_bytes + fr.GUARD
        self.host[:n] = fr.FILL
        self.dev.upload(src)
        rc = self.l.dt_hip_read_file_to_host(0, self.dev.ptr, capacity, self.pin + fr.GUARD, host_bytes)
        assert self.l.dt_hip_finish(0) == 1, self.l.dt_hip_last_error()
        return rc, self.host[:n]


@pytest.fixture(scope="module")
def bench():
    b = _Bench()
    yield b
    b.close()


@pytest.mark.parametrize("roomy", [False, True], ids=["exact", "large"])
def test_host_buffer_equals_the_host_twin(bench, roomy):
    src_buf = fr.aligned(BIG)
    for T in fr.TOTALS:
        cap = hb = BIG if roomy else T
        src = src_buf[:cap]
        fr.host().fc_host_pattern(src.ctypes.data, cap, T - 8)
        want, _, outside = fr.run(src, cap, hb, 64 * 256)
        assert outside == 0
        rc, got = bench.read(src, cap, hb)
        assert rc == abi.DT_HIP_SUCCESS, bench.l.dt_hip_last_error()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "T %d: %d bytes differ, the first at %d (the host buffer starts at %d)" % (T, bad.size, bad[0], fr.GUARD)
        # (the twin's own output is judged by tests/test_file_copy_host.py; here at least: it is the file and the fill)
        assert (want[fr.GUARD:fr.GUARD + T] == src[:T]).all() and (want[fr.GUARD + T:] == fr.FILL).all()


@pytest.mark.parametrize("T", [9, 24, 4097, 2 ** 20])
def test_short_host_buffer_gets_the_true_length_alone(bench, T):
    src = fr.pattern(T, T - 8)
    rc, got = bench.read(src, T, T - 1)
    assert rc == abi.DT_HIP_SUCCESS
    assert int(got[fr.GUARD:fr.GUARD + 8].view(np.uint64)[0]) == T - 8
    assert (got[:fr.GUARD] == fr.FILL).all() and (got[fr.GUARD + 8:] == fr.FILL).all()
    assert (got == fr.run(src, T, T - 1, 64 * 256)[0]).all()


@pytest.mark.parametrize("word", fr.NO_LENGTH)
def test_a_word_that_is_no_length_arrives_as_no_file(bench, word):
    for cap in (8, 4096):
        src = fr.pattern(cap, word)
        rc, got = bench.read(src, cap, cap)
        assert rc == abi.DT_HIP_SUCCESS
        assert int(got[fr.GUARD:fr.GUARD + 8].view(np.uint64)[0]) == fr.U64_MAX
        assert (got[:fr.GUARD] == fr.FILL).all() and (got[fr.GUARD + 8:] == fr.FILL).all()


def test_refused_buffers_stay_untouched(bench):
    l = bench.l
    T = 4096
    src = fr.pattern(T, T - 8)
    bench.dev.upload(src)
    bench.host[:] = fr.FILL
    plain = fr.aligned(T, fr.FILL)
    host = bench.pin + fr.GUARD
    for what, ptr, hb, cap in (("unpinned", plain.ctypes.data, T, T), ("misaligned", host + 8, T, T), ("4 bytes", host, 4, T),
                               ("capacity 4", host, T, 4), ("no buffer", None, T, T)):
        assert l.dt_hip_read_file_to_host(0, bench.dev.ptr, cap, ptr, hb) == abi.DT_HIP_INVALID_ARG, what
        assert l.dt_hip_last_error().decode().startswith("dt_hip_read_file_to_host: "), what
        assert l.dt_hip_finish(0) == 1
        assert (bench.host == fr.FILL).all() and (plain == fr.FILL).all(), what
    # and the same buffer is taken once the call is right
    assert l.dt_hip_read_file_to_host(0, bench.dev.ptr, T, host, T) == abi.DT_HIP_SUCCESS
    assert l.dt_hip_finish(0) == 1
    assert (bench.host[fr.GUARD:fr.GUARD + T] == src).all() and (bench.host[fr.GUARD + T:] == fr.FILL).all()
