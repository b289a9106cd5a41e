"""-m gpu: the PNG encoder on the device (dt_hip_export_png, ansel_amd/csrc/png.hip).

  * the device file equals the host build of png_deflate.h byte for byte (tests/png_ref.py): sizes 1x1 .. 1001x777,
    five contents, 8 and 16 bits, levels 0 / 1 / 5 / 9, ICC profiles of 1 byte and 200 KB, 300 dpi
  * its inflated IDAT equals libpng's filtered stream, and libpng decodes the input's pixels from it
  * the same frame twice gives the same bytes
  * capacity exactly 8 + L succeeds; one byte less gives the length word UINT64_MAX and leaves the bytes behind the
    capacity untouched; the same with a second IDAT chunk of one byte
  * the designed corpus png_ref.edge_frames() (tests/test_png_host.py shows on the host build which branch of the
    encoder each entry reaches): the device file equals the host build's, inflates to the filtered stream and decodes
    in libpng; the two png_scan frames (257 and 513 segments: 2 and 3 a thread, stored and dynamic blocks inside one
    thread's group) and the all-0xFF frame twice with identical bytes
  * png_tables alone (dt_hip_test_png_tables()) on histograms no frame produces: the 64-lane record equals the one-lane
    host build's, the Kraft sum is 1 and the cost optimal within the limit, all three length limits engaged"""
import ctypes as C

import numpy as np
import pytest

import hipcheck as hc
import png_ref as pr
from ansel_amd import abi, lib, params

pytestmark = pytest.mark.gpu

GUARD = 64


def encode_dev(img, level, icc=None, dpi=None, capacity=None, raw=False):
    """the file from the device; raw: (length word, the whole output buffer incl. GUARD bytes behind capacity)"""
    l = hc.hip()
    h, w = img.shape[:2]
    d = params.png(bpp=8 * img.itemsize, compression=level, icc=icc, dpi=dpi)
    bound = l.dt_hip_png_bound(w, h, C.byref(d))
    assert bound > 0
    d.capacity = bound if capacity is None else capacity
    d_in = lib.DeviceBuffer.from_numpy(0, np.ascontiguousarray(img))
    d_out = lib.DeviceBuffer.from_numpy(0, np.full(d.capacity + GUARD, 0xA5, np.uint8))
    held = hc.allocated_bytes()
    rc = l.dt_hip_export_png(0, w, h, C.byref(d), d_in.ptr, d_out.ptr)
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
    return buf[8:8 + n].tobytes()


@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("w,h", pr.SIZES)
def test_device_file_equals_host_build(w, h, depth):
    for ki, kind in enumerate(pr.KINDS):
        img = pr.frame(kind, w, h, depth, seed=ki + 3 * w)
        stream = pr.filtered(img) if w * h < 10000 else pr.host_filtered(img)
        for level in (0, 1, 5, 9):
            got = encode_dev(img, level)
            assert got == pr.host_file(img, level), (kind, level)
            assert pr.inflate(got) == stream, (kind, level)
            if pr.ref() is not None:
                rgb, _, _ = pr.libpng_read(got, w, h, depth)
                assert np.array_equal(rgb, img[..., :3]), (kind, level)
            else:
                assert np.array_equal(pr.unfilter(pr.inflate(got), w, h, depth), img[..., :3])


def test_filtered_stream_equals_libpng():
    if pr.ref() is None:
        pytest.skip("libpng is not installed")
    for depth in (8, 16):
        for kind in pr.KINDS:
            img = pr.frame(kind, 1001, 777, depth, seed=9)
            assert pr.inflate(encode_dev(img, 5)) == pr.inflate(pr.libpng_file(img, 5)), (depth, kind)


@pytest.mark.parametrize("icc_bytes", [1, 200000])
def test_icc_and_dpi(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    for depth in (8, 16):
        img = pr.frame("gradient", 130, 67, depth, seed=1)
        for level in (0, 5):
            got = encode_dev(img, level, icc=icc, dpi=300)
            assert got == pr.host_file(img, level, icc=icc, dpi=300), (depth, level)
            assert [t for t, _, _ in pr.chunks(got)[:3]] == ["IHDR", "iCCP", "pHYs"]


def test_two_runs_are_identical_with_stored_and_dynamic_blocks():
    img = pr.frame("noise", 1001, 777, 8, seed=4)
    img[200:500, :, :3] = 7  # runs and matches beside the noise: dynamic blocks between stored ones
    for level in (1, 5):
        got = encode_dev(img, level)
        assert got == encode_dev(img, level)
        assert got == pr.host_file(img, level)
        assert pr.inflate(got) == pr.host_filtered(img)


def test_capacity_one_byte_short():
    for depth, kind in ((8, "gradient"), (16, "noise")):
        img = pr.frame(kind, 257, 129, depth, seed=2)
        exact = encode_dev(img, 5)
        n, buf = encode_dev(img, 5, capacity=8 + len(exact), raw=True)
        assert n == len(exact) and buf[8:8 + n].tobytes() == exact
        assert (buf[8 + n:] == 0xA5).all()
        n, buf = encode_dev(img, 5, capacity=8 + len(exact) - 1, raw=True)
        assert n == 2 ** 64 - 1
        assert (buf[8:] == 0xA5).all()


def test_refused_arguments():
    l = hc.hip()
    d_in, d_out = lib.DeviceBuffer(0, 64), lib.DeviceBuffer(0, 4096)
    for bad in (dict(bit_depth=12), dict(compression_level=10), dict(compression_level=-1)):
        d = abi.PngData(bit_depth=8, compression_level=5, capacity=4096)
        for k, v in bad.items():
            setattr(d, k, v)
        assert l.dt_hip_export_png(0, 4, 4, C.byref(d), d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
    d = abi.PngData(bit_depth=8, compression_level=5, capacity=4096)
    assert l.dt_hip_export_png(0, 0, 4, C.byref(d), d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
    assert l.dt_hip_export_png(0, 4, 0, C.byref(d), d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
    assert "4 x 0" in l.dt_hip_last_error().decode()
    d_in.release()
    d_out.release()


# ---------------------------------------------------------------------------------------------------------------------
# the designed corpus (png_ref.edge_frames(); tests/test_png_host.py proves on the host build which branch each reaches)

EDGES = pr.edge_frames()


@pytest.mark.parametrize("name,levels,feats", EDGES, ids=[e[0] for e in EDGES])
def test_edge_frame_device_file_equals_host_build(name, levels, feats):
    img = pr.edge_frame(name)
    h, w = img.shape[:2]
    for level in levels:
        want, _, stream = pr.edge_host(name, level)
        got = encode_dev(img, level)
        assert got == want, level
        assert pr.inflate(got) == stream, level
        if pr.ref() is not None:
            rgb, _, _ = pr.libpng_read(got, w, h, 8 * img.itemsize)
            assert np.array_equal(rgb, img[..., :3]), level
        if name in pr.SCAN_FRAMES or name == "all_ff":
            assert encode_dev(img, level) == got, level


def test_capacity_one_byte_short_at_an_idat_boundary():
    """zlen 65537: the second IDAT chunk holds one byte, the Adler-32's last"""
    img = pr.edge_frame("zlen_65537")
    exact = encode_dev(img, 0)
    assert exact == pr.edge_host("zlen_65537", 0)[0]
    n, buf = encode_dev(img, 0, capacity=8 + len(exact), raw=True)
    assert n == len(exact) and buf[8:8 + n].tobytes() == exact
    assert (buf[8 + n:] == 0xA5).all()
    n, buf = encode_dev(img, 0, capacity=8 + len(exact) - 1, raw=True)
    assert n == 2 ** 64 - 1
    assert (buf[8:] == 0xA5).all()


def test_table_builder_device_equals_host_and_holds_the_code_properties():
    """png_tables alone (dt_hip_test_png_tables()) on png_ref.table_histograms(): each record equals the one-lane host
    build's in every field but the Adler sums -- the 64-lane minimum search breaks ties as the one-lane order does, on
    Fibonacci counts too -- and png_ref.check_tables() holds for the device's record: codes within 15 / 15 / 7 bits, the
    Kraft sum exactly 1, the cost optimal wherever the unadjusted code fits the limit, the block's bits recomputed"""
    l = hc.hip()
    l.dt_hip_test_png_sizeof_seg.restype = C.c_size_t
    assert l.dt_hip_test_png_sizeof_seg() == C.sizeof(pr.Seg)
    l.dt_hip_test_png_tables.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    names, freq = pr.table_histograms()
    n = len(freq)
    host_segs, longest = pr.host_tables(freq)
    segs = (pr.Seg * n)()
    rc = l.dt_hip_test_png_tables(0, freq.ctypes.data, n * pr.SEG, n, 5, C.byref(segs))
    assert rc == abi.DT_HIP_SUCCESS, l.dt_hip_last_error().decode()
    for name, f, s, hs, lg in zip(names, freq, segs, host_segs, longest):
        assert pr.seg_fields(s) == pr.seg_fields(hs), name
        pr.check_tables(f, s, lg)
    stored = (pr.Seg * 3)()
    rc = l.dt_hip_test_png_tables(0, freq.ctypes.data, 3 * pr.SEG, 3, 0, C.byref(stored))
    assert rc == abi.DT_HIP_SUCCESS
    assert all(pr.seg_fields(s) == (0, pr.SEG, 0, 0, 0, 0, bytes(316), bytes(19)) for s in stored)
    assert l.dt_hip_test_png_tables(0, freq.ctypes.data, 3 * pr.SEG + 1, 3, 5, C.byref(segs)) == abi.DT_HIP_INVALID_ARG
    assert l.dt_hip_test_png_tables(0, freq.ctypes.data, 65537 * pr.SEG, 65537, 5, C.byref(segs)) == abi.DT_HIP_INVALID_ARG
    by = dict(zip(names, segs))
    for name in pr.LARGE_FEW_SYMBOLS:  # the dynamic block wins: check_tables() saw the lengths pd_lengths() raised
        assert by[name].type == 2, name
