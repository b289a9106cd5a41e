"""The trimmed file download's body on the host (tests/native/file_copy_host.cpp over ansel_amd/csrc/file_copy_body.h): the
functions the kernel file_to_host runs, lane after lane, with every store counted.

  * fc_total() is 8 + L exactly when that is a length both buffers hold, and never more than either buffer
  * for every total in file_copy_ref.TOTALS, the capacities T / T + 1 / T - 1, the host sizes T / T - 1 / 8, the file's own
    word and three words that are no length, by 1, 64, 256 and 4096 lanes: the bytes below the expected total are exact, every
    byte from there on and both guards keep their fill, no store leaves the buffer, every byte is stored exactly once
  * the twin as a program of its own under -fsanitize=address,undefined"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import file_copy_ref as fr


def _variants(T):
    caps = [T, T + 1] + ([T - 1] if T > 8 else [])
    hosts = [T] + ([T - 1] if T > 8 else []) + [8]
    return [(c, h) for c in caps for h in sorted(set(hosts))]


def test_total_is_a_length_both_buffers_hold_or_the_word_alone():
    h = fr.host()
    for T in fr.TOTALS:
        for cap, hb in _variants(T):
            for word in (T - 8,) + fr.NO_LENGTH:
                total = h.fc_host_total(word, cap, hb)
                assert total == fr.expected(word, cap, hb)[0], (word, cap, hb)
                assert 8 <= total <= min(cap, hb)
                assert h.fc_host_word_of(word, cap) == fr.expected(word, cap, hb)[1]
    rng = np.random.default_rng(11)
    for word in [int(x) for x in rng.integers(0, 2 ** 64, 2000, dtype=np.uint64)] + [0, 1, 2 ** 32, fr.U64_MAX - 8]:
        for cap, hb in ((8, 8), (4096, 64), (64, 4096), (2 ** 40, 2 ** 41), (fr.U64_MAX, fr.U64_MAX)):
            total = h.fc_host_total(word, cap, hb)
            assert total == fr.expected(word, cap, hb)[0] and total <= min(cap, hb), (word, cap, hb)


@pytest.mark.parametrize("lanes", fr.LANES)
def test_every_byte_below_the_total_once_and_none_beyond(lanes):
    biggest = max(fr.TOTALS) + 1
    src_buf = fr.aligned(biggest)
    dst_buf = fr.aligned(fr.GUARD + biggest + fr.GUARD)
    counts_buf = np.empty(biggest, np.uint8)
    cases = 0
    for T in fr.TOTALS:
        for cap, hb in _variants(T):
            for word in (T - 8,) + fr.NO_LENGTH:
                src = src_buf[:cap]
                fr.host().fc_host_pattern(src.ctypes.data, cap, word)
                want, want_word = fr.expected(word, cap, hb)
                dst, counts, outside = fr.run(src, cap, hb, lanes, dst_buf[:fr.GUARD + hb + fr.GUARD], counts_buf[:hb])
                what = "T %d word %x capacity %d host_bytes %d" % (T, word, cap, hb)
                assert outside == 0, what
                body = dst[fr.GUARD:fr.GUARD + hb]
                assert int(body[:8].view(np.uint64)[0]) == want_word, what
                assert (body[8:want] == src[8:want]).all(), what
                assert (body[want:] == fr.FILL).all(), what
                assert (dst[:fr.GUARD] == fr.FILL).all() and (dst[fr.GUARD + hb:] == fr.FILL).all(), what
                assert (counts[:want] == 1).all() and not counts[want:].any(), what
                cases += 1
    assert cases > 3000


@pytest.mark.parametrize("lanes", fr.LANES)
def test_the_copy_alone_takes_any_total(lanes):
    """fc_copy() below the kernel's rule: totals under 8 too, which the kernel never asks for"""
    h = fr.host()
    src = fr.pattern(4096 + 64, 0x0123456789abcdef)
    for total in list(range(0, 70)) + [4095, 4096, 4097]:
        dst = fr.aligned(total + 32, fr.FILL)
        counts = np.empty(total + 32, np.uint8)
        assert h.fc_host_copy(dst.ctypes.data, total + 32, src.ctypes.data, total, lanes, counts.ctypes.data) == 0
        assert (dst[:total] == src[:total]).all() and (dst[total:] == fr.FILL).all(), total
        assert (counts[:total] == 1).all() and not counts[total:].any(), total


def test_host_twin_runs_clean_under_sanitizers():
    """file_copy_host.cpp as a program of its own (-DFILE_COPY_HOST_MAIN): source and destination allocated at their exact
    sizes, so a load beyond the capacity is the sanitizer's error and a store beyond the host buffer the program's"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "file_copy_host")
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-DFILE_COPY_HOST_MAIN", "-I" + os.path.join(fr.ROOT, "ansel_amd", "csrc"),
                            os.path.join(fr.NATIVE, "file_copy_host.cpp"), "-o", exe], capture_output=True, text=True)
        if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
            pytest.skip("no sanitizer runtime for g++ here")
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases" in r.stdout
