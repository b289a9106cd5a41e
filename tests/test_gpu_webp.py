"""-m gpu: the lossless WebP encoder on the device (dt_hip_export_webp, ansel_amd/csrc/webp.hip).

  * the device file equals the host build of webp_body.h byte for byte (tests/webp_ref.py; tests/test_webp_host.py has
    libwebp judge that file) on the whole corpus webp_ref.CASES at levels 0 / 1 / 6 -- and, independently, libwebp
    decodes the DEVICE's file to the input's pixels
  * ICC profiles of 1 byte and 200 001 bytes
  * capacity exactly 8 + L succeeds; one byte less gives the length word UINT64_MAX and leaves the bytes behind the
    capacity untouched (a guard pattern lies behind the buffer)
  * every refused argument returns DT_HIP_INVALID_ARG and names export_webp
  * two encodes of one frame into buffers pre-filled with different bytes give equal files"""
import ctypes as C

import numpy as np
import pytest

import hipcheck as hc
import webp_ref as wr
from ansel_amd import abi, lib
from test_webp_host import REFUSED

pytestmark = pytest.mark.gpu

GUARD = 64


def encode_dev(img, d, capacity=None, raw=False, fill=0xA5):
    """the file from the device; raw: (length word, the whole output buffer incl. GUARD bytes behind capacity)"""
    l = hc.hip()
    h, w = img.shape[:2]
    bound = l.dt_hip_webp_bound(w, h, C.byref(d))
    assert bound > 0
    d.capacity = bound if capacity is None else capacity
    d_in = lib.DeviceBuffer.from_numpy(0, np.ascontiguousarray(img))
    d_out = lib.DeviceBuffer.from_numpy(0, np.full(d.capacity + GUARD, fill, np.uint8))
    held = hc.allocated_bytes()
    rc = l.dt_hip_export_webp(0, w, h, C.byref(d), d_in.ptr, d_out.ptr)
    finished = l.dt_hip_finish(0)
    assert hc.allocated_bytes() == held, "the encoder's scratch is not back in the pool (rc %d)" % rc
    assert rc == abi.DT_HIP_SUCCESS, l.dt_hip_last_error().decode()
    assert finished == 1
    buf = d_out.to_numpy((d.capacity + GUARD,), np.uint8)
    d_in.release()
    d_out.release()
    n = int(buf[:8].view(np.uint64)[0])
    if raw:
        return n, buf
    assert n != 2 ** 64 - 1 and 8 + n <= d.capacity
    assert (buf[8 + n:] == fill).all(), "bytes behind the file were written"
    return buf[8:8 + n].tobytes()


@pytest.mark.parametrize("name", [c[0] for c in wr.CASES])
def test_device_file_equals_host_build_and_decodes(name):
    img, pb, eb = wr.case(name)
    h, w = img.shape[:2]
    for level in wr.LEVELS:
        got = encode_dev(img, wr.data(level, pb, eb))
        assert got == wr.case_file(name, level)[0], level
        mode, px, _ = wr.decode(got)
        assert mode == "RGB" and (px == img[..., :3]).all(), level


@pytest.mark.parametrize("icc_bytes", [1, 200001])
def test_icc(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    img = wr.frame("mix", 37, 13, 5)
    got = encode_dev(img, wr.data(6, icc=icc))
    assert got == wr.host_file(img, wr.data(6, icc=icc))
    wr.check_layout(got, 37, 13, icc)
    mode, px, info = wr.decode(got)
    assert mode == "RGB" and (px == img[..., :3]).all() and info["icc_profile"] == icc


def test_output_does_not_depend_on_what_the_buffers_held():
    for name in ("two_segments_plus_1", "3x3_tiles_ragged", "rows"):
        img, pb, eb = wr.case(name)
        a = encode_dev(img, wr.data(6, pb, eb), fill=0x00)
        b = encode_dev(img, wr.data(6, pb, eb), fill=0xFF)
        assert a == b == wr.case_file(name, 6)[0]


@pytest.mark.parametrize("name,level", [("3x3_tiles_ragged", 6), ("two_segments", 1), ("1x1", 0), ("noise", 6)])
def test_capacity_short(name, level):
    img, pb, eb = wr.case(name)
    exact = wr.case_file(name, level)[0]
    n, buf = encode_dev(img, wr.data(level, pb, eb), capacity=8 + len(exact), raw=True)
    assert n == len(exact) and buf[8:8 + n].tobytes() == exact
    assert (buf[8 + n:] == 0xA5).all()
    for capacity in (8 + len(exact) - 1, 8 + len(exact) // 2, 8):
        n, buf = encode_dev(img, wr.data(level, pb, eb), capacity=capacity, raw=True)
        assert n == 2 ** 64 - 1
        assert (buf[capacity:] == 0xA5).all(), "written behind a capacity of %d" % capacity
        assert (buf[8:] == 0xA5).all(), "a file that does not fit was written in part"


def test_refused_arguments():
    l = hc.hip()
    d_in = lib.DeviceBuffer(0, 16 * 16 * 4)
    d_out = lib.DeviceBuffer(0, 65536)

    def refused(w, h, d, din=d_in.ptr, dout=d_out.ptr, message=True):
        d.capacity = 65536
        assert l.dt_hip_export_webp(0, w, h, C.byref(d), din, dout) == abi.DT_HIP_INVALID_ARG
        assert not message or "export_webp" in l.dt_hip_last_error().decode()

    for bad in REFUSED:
        refused(16, 16, wr.data(**bad))
        assert l.dt_hip_webp_bound(16, 16, C.byref(wr.data(**bad))) == 0
    for w, h in ((0, 4), (4, 0), (-1, 4), (16384, 1), (1, 16384)):
        refused(w, h, wr.data())
    no_icc = wr.data()
    no_icc.icc_bytes = 4
    refused(16, 16, no_icc)
    refused(16, 16, wr.data(), din=None, message=False)
    refused(16, 16, wr.data(), dout=None, message=False)
    d = wr.data()
    d.capacity = 7
    assert l.dt_hip_export_webp(0, 16, 16, C.byref(d), d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
    assert "export_webp" in l.dt_hip_last_error().decode() and "capacity" in l.dt_hip_last_error().decode()
    assert l.dt_hip_finish(0) == 1
    d_in.release()
    d_out.release()
