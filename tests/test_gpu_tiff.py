"""-m gpu: the TIFF encoder on the device (dt_hip_export_tiff, ansel_amd/csrc/tiff.hip).

  * the device file equals the host build of tiff_body.h / png_deflate.h byte for byte (tests/tiff_ref.py; tests/
    test_tiff_host.py checks that file against libtiff) on the whole corpus tiff_ref.CASES, every entry in every variant
    that fits it: no compression, deflate at levels 0 / 1 / 6 with predictor 1 and the format's own
  * ICC profiles of 1 byte and 200 001 bytes, 300 dpi, strips of odd compressed length
  * capacity exactly 8 + L succeeds; one byte less, and one byte short of the end of the first strip, give the length word
    UINT64_MAX and leave the bytes behind the capacity untouched
  * every refused argument returns DT_HIP_INVALID_ARG with a message
  * the same frame twice gives the same bytes"""
import ctypes as C

import numpy as np
import pytest

import hipcheck as hc
import tiff_ref as tr
from ansel_amd import abi, lib
from test_tiff_host import ODD, REFUSED

pytestmark = pytest.mark.gpu

GUARD = 64


def encode_dev(img, d, capacity=None, raw=False):
    """the file from the device; raw: (length word, the whole output buffer incl. GUARD bytes behind capacity)"""
    l = hc.hip()
    h, w = img.shape[:2]
    bound = l.dt_hip_tiff_bound(w, h, C.byref(d))
    assert bound > 0
    d.capacity = bound if capacity is None else capacity
    d_in = lib.DeviceBuffer.from_numpy(0, np.ascontiguousarray(img))
    d_out = lib.DeviceBuffer.from_numpy(0, np.full(d.capacity + GUARD, 0xA5, np.uint8))
    held = hc.allocated_bytes()
    rc = l.dt_hip_export_tiff(0, w, h, C.byref(d), d_in.ptr, d_out.ptr)
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
    assert (buf[8 + n:] == 0xA5).all(), "bytes behind the file were written"
    return buf[8:8 + n].tobytes()


@pytest.mark.parametrize("name", [c[0] for c in tr.CASES])
def test_device_file_equals_host_build(name):
    img, layers, rps = tr.case(name)
    for v in tr.variants(8 * img.itemsize):
        got = encode_dev(img, tr.data_for(img, layers, v, rps))
        assert got == tr.case_file(name, v), v


@pytest.mark.parametrize("icc_bytes", [1, 200001])
def test_icc_dpi_and_strips_of_odd_length(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    img = tr.frame("mix", 37, 13, 8, seed=5)
    for comp in (abi.DT_HIP_TIFF_DEFLATE, abi.DT_HIP_TIFF_NONE):
        kw = dict(ODD, compression=comp, predictor=2 if comp == abi.DT_HIP_TIFF_DEFLATE else 1, icc=icc)
        got = encode_dev(img, tr.data(**kw))
        assert got == tr.host_file(img, tr.data(**kw))
        tr.check_layout(got)
        assert tr.decode(got).tobytes() == tr.samples(img, 3)


def test_two_runs_are_identical():
    for name in ("three_segments", "many_strips", "special_37x13_rgb"):
        img, layers, rps = tr.case(name)
        v = tr.variants(8 * img.itemsize)[-1]
        assert encode_dev(img, tr.data_for(img, layers, v, rps)) == encode_dev(img, tr.data_for(img, layers, v, rps))


@pytest.mark.parametrize("name,variant", [("37x13_rps5_8_3", 6), ("37x13_rps5_8_3", 0), ("three_segments", 6),
                                          ("37x13_rps5_32_3", 0)])
def test_capacity_short(name, variant):
    img, layers, rps = tr.case(name)
    v = tr.variants(8 * img.itemsize)[variant]
    exact = tr.case_file(name, v)
    n, buf = encode_dev(img, tr.data_for(img, layers, v, rps), capacity=8 + len(exact), raw=True)
    assert n == len(exact) and buf[8:8 + n].tobytes() == exact
    assert (buf[8 + n:] == 0xA5).all()
    off, cnt = tr.strips(exact)[0]
    for capacity in (8 + len(exact) - 1, 8 + off + cnt - 1):
        n, buf = encode_dev(img, tr.data_for(img, layers, v, rps), capacity=capacity, raw=True)
        assert n == 2 ** 64 - 1
        assert (buf[capacity:] == 0xA5).all(), "written behind a capacity of %d" % capacity


def test_refused_arguments():
    l = hc.hip()
    ok = dict(bpp=8, layers=3, compression=abi.DT_HIP_TIFF_DEFLATE, predictor=1, level=6)
    d_in = lib.DeviceBuffer(0, 16 * 16 * 16)
    d_out = lib.DeviceBuffer(0, 65536)

    def refused(w, h, d, din=d_in.ptr, dout=d_out.ptr, message=True):
        d.capacity = 65536
        assert l.dt_hip_export_tiff(0, w, h, C.byref(d), din, dout) == abi.DT_HIP_INVALID_ARG
        assert not message or "export_tiff" in l.dt_hip_last_error().decode()

    for bad in REFUSED:
        refused(16, 16, tr.data(**dict(ok, **bad)))
    for w, h in ((0, 4), (4, 0), (-1, 4)):
        refused(w, h, tr.data(**ok))
    no_icc = tr.data(**ok)
    no_icc.icc_bytes = 4
    refused(16, 16, no_icc)
    refused(32768, 32768, tr.data(32, 1))
    refused(16, 16, tr.data(**ok), din=None, message=False)
    refused(16, 16, tr.data(**ok), dout=None, message=False)
    d = tr.data(**ok)
    d.capacity = 7
    assert l.dt_hip_export_tiff(0, 16, 16, C.byref(d), d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
    assert "capacity" in l.dt_hip_last_error().decode()
    assert l.dt_hip_finish(0) == 1
    d_in.release()
    d_out.release()
