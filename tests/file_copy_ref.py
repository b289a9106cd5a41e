"""The host twin of the trimmed file download (tests/native/file_copy_host.cpp over ansel_amd/csrc/file_copy_body.h) and
the cases both its CPU test and the device test run: shared by tests/test_file_copy_host.py and tests/test_gpu_file_copy.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")

U64_MAX = 2 ** 64 - 1
GUARD = 64
FILL = 0xA5
# T = 8 + L: every value in 8 .. 49 (the 16-byte body from 0 to 3 words with every tail), and the powers of two 2^6 ..
# 2^22 at their -1 / 0 / +1 edges (4 MiB: many sweeps of a grid of 64 x 256 lanes, and of the four-deep inner loop)
TOTALS = list(range(8, 50)) + [2 ** k + e for k in range(6, 23) for e in (-1, 0, 1)]
LANES = (1, 64, 256, 256 * 16)
# words that are no length: the encoder's refusal, a sum that wraps to 0, and one that is merely huge
NO_LENGTH = (U64_MAX, U64_MAX - 7, 2 ** 63)

_cache = {}


def host():
    """the copy's body compiled for the host"""
    if "host" not in _cache:
        so = os.path.join(tempfile.mkdtemp(prefix="file_copy_ref_"), "libfile_copy_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "ansel_amd", "csrc"),
                               os.path.join(NATIVE, "file_copy_host.cpp"), "-o", so])
        lib = C.CDLL(so)
        u64, vp = C.c_uint64, C.c_void_p
        lib.fc_host_pattern.restype = None
        lib.fc_host_pattern.argtypes = [vp, u64, u64]
        lib.fc_host_total.restype = u64
        lib.fc_host_total.argtypes = [u64, u64, u64]
        lib.fc_host_word_of.restype = u64
        lib.fc_host_word_of.argtypes = [u64, u64]
        lib.fc_host_copy.restype = u64
        lib.fc_host_copy.argtypes = [vp, u64, vp, u64, u64, vp]
        lib.fc_host_run.restype = u64
        lib.fc_host_run.argtypes = [vp, vp, u64, u64, u64, vp]
        _cache["host"] = lib
    return _cache["host"]


def aligned(nbytes, fill=None):
    """nbytes of uint8 on a 64-byte boundary"""
    raw = np.empty(nbytes + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    out = raw[off:off + nbytes]
    if fill is not None:
        out[:] = fill
    return out


def pattern(nbytes, word):
    """a file buffer of nbytes: the length word, then the twin's position-dependent bytes"""
    buf = aligned(nbytes)
    host().fc_host_pattern(buf.ctypes.data, nbytes, word)
    return buf


def expected(word, capacity, host_bytes):
    """(bytes written, the host's word) by the rule of include/ansel_hip.h, in Python's integers: no sum wraps here"""
    is_len = word != U64_MAX and 8 + word <= capacity
    return (8 + word if is_len and 8 + word <= host_bytes else 8), (word if is_len else U64_MAX)


def run(src, capacity, host_bytes, lanes, dst=None, counts=None):
    """the twin's kernel on a destination of GUARD + host_bytes + GUARD bytes of FILL -> (that buffer, the stores per
    byte of the host buffer, the stores that would have left it)"""
    if dst is None:
        dst = aligned(GUARD + host_bytes + GUARD)
    if counts is None:
        counts = np.empty(host_bytes, np.uint8)
    dst[:] = FILL
    outside = host().fc_host_run(dst.ctypes.data + GUARD, src.ctypes.data, capacity, host_bytes, lanes, counts.ctypes.data)
    return dst, counts, outside
