"""-m gpu: the JPEG encoder on the device (dt_hip_export_jpeg, ansel_amd/csrc/jpeg.hip).

  * every byte of the file equals tests/jpeg_ref.py's, and Pillow's libjpeg(-turbo) where Pillow is installed: sizes
    1x1 .. 1001x777 and ~2 MP, five contents, the three sampling modes, optimize_coding 0 / 1, quality 50 .. 100, ICC
    profiles of 3 KB and 140 KB (3 APP2 chunks), 300 dpi
  * the same frame twice gives the same bytes
  * capacity exactly 8 + L succeeds; one byte less gives the length word UINT64_MAX and leaves the bytes behind the
    capacity untouched
  * a 24 MP frame equals the reference"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import hipcheck as hc
import jpeg_ref as jr
from ansel_amd import abi, lib

pytestmark = pytest.mark.gpu

GUARD = 64


def jdata(quality, subsampling, optimize, icc=None, density=(0, 1, 1)):
    d = abi.JpegData(quality=quality, subsampling=subsampling, optimize_coding=int(optimize), density_unit=density[0],
                     x_density=density[1], y_density=density[2])
    if icc:
        d._icc = C.create_string_buffer(icc, len(icc))
        d.icc = C.cast(d._icc, C.c_void_p)
        d.icc_bytes = len(icc)
    return d


def encode_dev(img, quality, subsampling, optimize, icc=None, density=(0, 1, 1), capacity=None, raw=False):
    """the file from the device; raw: (length word, the whole output buffer incl. GUARD bytes behind capacity)"""
    l = hc.hip()
    h, w = img.shape[:2]
    d = jdata(quality, subsampling, optimize, icc, density)
    bound = l.dt_hip_jpeg_bound(w, h, C.byref(d))
    assert bound > 0
    d.capacity = bound if capacity is None else capacity
    d_in = lib.DeviceBuffer.from_numpy(0, np.ascontiguousarray(img))
    out_init = np.full(d.capacity + GUARD, 0xA5, np.uint8)
    d_out = lib.DeviceBuffer.from_numpy(0, out_init)
    held = hc.allocated_bytes()
    rc = l.dt_hip_export_jpeg(0, w, h, C.byref(d), d_in.ptr, d_out.ptr)
    finished = l.dt_hip_finish(0)
    assert hc.allocated_bytes() == held, "the encoder's scratch is not back in the pool (rc %d)" % rc
    assert rc == abi.DT_HIP_SUCCESS, hc.hip().dt_hip_last_error().decode()
    assert finished == 1
    buf = d_out.to_numpy((d.capacity + GUARD,), np.uint8)
    d_in.release()
    d_out.release()
    n = int(buf[:8].view(np.uint64)[0])
    if raw:
        return n, buf
    assert n != 2 ** 64 - 1 and 8 + n <= d.capacity
    return buf[8:8 + n].tobytes()


def check(img, quality, subsampling, optimize, icc=None, density=(0, 1, 1)):
    got = encode_dev(img, quality, subsampling, optimize, icc, density)
    ref = jr.encode(img, quality, subsampling, optimize, icc, density)
    assert got == ref, "device vs jpeg_ref: %d vs %d bytes, first difference at %s" % (
        len(got), len(ref), next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), "the end"))
    dpi = density[1:] if density[0] == 1 else None
    pil = jr.pillow(img, quality, subsampling, optimize, icc, dpi)
    if pil is not None and density[0] in (0, 1) and (density[0] == 1 or density[1:] == (1, 1)):
        assert got == pil, "device vs Pillow"


SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (1001, 777)]
KINDS = ["gradient", "zero", "full", "primaries", "noise"]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("ss", [0, 1, 2])
@pytest.mark.parametrize("opt", [0, 1])
def test_bytes_equal_reference(w, h, ss, opt):
    for ki, kind in enumerate(KINDS):
        img = jr.frame(kind, w, h, seed=w * 7 + h + ki)
        qs = (50, 80, 90, 92, 95, 100) if w * h < 10000 or kind in ("gradient", "noise") else (90,)
        for q in qs:
            check(img, q, ss, opt)


@pytest.mark.parametrize("ss", [0, 1, 2])
def test_two_megapixel_frame(ss):
    img = jr.frame("gradient", 1733, 1157, seed=3)
    check(img, 95, ss, 1)
    check(img, 92, ss, 0)


@pytest.mark.parametrize("icc_bytes", [3000, 140000])
def test_icc_profiles_and_density(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    img = jr.frame("gradient", 257, 129, seed=5)
    for ss in (0, 2):
        check(img, 95, ss, 1, icc=icc)
        check(img, 90, ss, 0, icc=icc, density=(1, 300, 300))


def test_same_frame_same_bytes():
    img = jr.frame("noise", 999, 555, seed=9)
    a = encode_dev(img, 95, 0, 1)
    b = encode_dev(img, 95, 0, 1)
    assert a == b


def test_capacity_exact_and_one_short():
    img = jr.frame("gradient", 333, 222, seed=11)
    ref = jr.encode(img, 92, 1, 1)
    L = len(ref)
    n, buf = encode_dev(img, 92, 1, 1, capacity=L + 8, raw=True)
    assert n == L and buf[8:8 + L].tobytes() == ref
    assert (buf[L + 8:] == 0xA5).all()
    n, buf = encode_dev(img, 92, 1, 1, capacity=L + 7, raw=True)
    assert n == 2 ** 64 - 1
    assert (buf[L + 7:] == 0xA5).all(), "bytes written past the capacity"


def test_refusals():
    l = hc.hip()
    d_in = lib.DeviceBuffer(0, 4 * 16)
    d_out = lib.DeviceBuffer(0, 1 << 16)
    for w, h, q, ss in [(0, 4, 90, 0), (65536, 4, 90, 0), (4, 4, 0, 0), (4, 4, 101, 0), (4, 4, 90, 3), (4, 4, 90, -1)]:
        d = jdata(q, ss, 1)
        d.capacity = 1 << 16
        assert l.dt_hip_export_jpeg(0, w, h, C.byref(d), d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
        assert hc.hip().dt_hip_last_error().decode()
    d_in.release()
    d_out.release()


@pytest.mark.parametrize("ss", [0, 2])
def test_24mp_frame(ss):
    img = jr.frame("gradient", 6000, 4000, seed=24)
    got = encode_dev(img, 95, ss, 1)
    assert got == jr.encode(img, 95, ss, 1)
