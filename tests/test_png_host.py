"""not gpu: the PNG encoder's pieces that run without a device (tests/png_ref.py holds the checkers).

  * the numpy restatement of libpng's filter choice equals the filtered stream inflated from libpng's own file, and
    the host build of ansel_amd/csrc/png_deflate.h gives the same stream: sizes 1x1 .. 1001x777, five contents, 8 and
    16 bits
  * the host build's zlib stream inflates (zlib) to that stream at levels 0 / 1 / 5 / 9; its file opens in libpng with
    identical pixels at both depths and in Pillow at 8 bits; every chunk CRC is valid; iCCP and pHYs read back
  * dt_hip_png_bound() is at least the stored-only file for uniform noise, and refuses what the encoder refuses
  * abi.PngData matches the library's struct; params.png(); pipe.with_png()"""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import png_ref as pr
from ansel_amd import abi, lib, params, pipe

needs_libpng = pytest.mark.skipif(pr.libpng_prefix() is None, reason="libpng (headers and library) is not installed")


@needs_libpng
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("w,h", pr.SIZES)
def test_filter_choice_equals_libpng(w, h, depth):
    for ki, kind in enumerate(pr.KINDS):
        img = pr.frame(kind, w, h, depth, seed=ki + w)
        ref = pr.inflate(pr.libpng_file(img, 5))
        assert pr.filtered(img) == ref, kind
        assert pr.host_filtered(img) == ref, kind


@needs_libpng
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("w,h", pr.SIZES)
def test_host_file_inflates_and_decodes(w, h, depth):
    for ki, kind in enumerate(pr.KINDS):
        img = pr.frame(kind, w, h, depth, seed=ki + 7 * w)
        stream = pr.filtered(img)
        for level in (0, 1, 5, 9):
            f = pr.host_file(img, level)
            cs = pr.chunks(f)
            assert [t for t, _, _ in cs][0] == "IHDR" and cs[-1][0] == "IEND"
            assert all(ok for _, _, ok in cs), (kind, level)
            z = pr.idat_stream(f)
            assert z[0] == 0x78 and ((z[0] << 8) | z[1]) % 31 == 0
            assert zlib.decompress(z) == stream, (kind, level)
            rgb, _, _ = pr.libpng_read(f, w, h, depth)
            assert np.array_equal(rgb, img[..., :3]), (kind, level)


def test_host_file_opens_in_pillow_at_8_bits():
    Image = pytest.importorskip("PIL.Image")
    for kind in pr.KINDS:
        img = pr.frame(kind, 130, 67, 8, seed=3)
        for level in (0, 5):
            got = np.asarray(Image.open(io.BytesIO(pr.host_file(img, level))).convert("RGB"))
            assert np.array_equal(got, img[..., :3]), (kind, level)


@needs_libpng
@pytest.mark.parametrize("icc_bytes", [1, 200000])
def test_host_file_icc_and_dpi(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    img = pr.frame("gradient", 65, 47, 16, seed=1)
    f = pr.host_file(img, 5, icc=icc, dpi=300)
    cs = pr.chunks(f)
    assert [t for t, _, _ in cs[:3]] == ["IHDR", "iCCP", "pHYs"]
    name, rest = cs[1][1].split(b"\0", 1)
    assert name == b"icc" and rest[0] == 0 and zlib.decompress(rest[1:]) == icc
    rgb, _, ppm = pr.libpng_read(f, 65, 47, 16)  # (libpng drops random bytes as a profile: zlib checked it above)
    assert np.array_equal(rgb, img[..., :3]) and ppm == 11811


def test_long_runs_and_repeats_round_trip():
    """matches across segment borders, the longest matches, distances up to the window"""
    rng = np.random.default_rng(5)
    tile = rng.integers(0, 256, (40, 700, 4), dtype=np.uint8)
    img = np.concatenate([tile, tile, np.zeros((30, 700, 4), np.uint8), tile], axis=0)
    stream = pr.filtered(img)
    for level in (1, 4, 9):
        f = pr.host_file(img, level)
        assert zlib.decompress(pr.idat_stream(f)) == stream
        assert len(f) < len(pr.host_file(img, 0))


def _data(**kw):
    d = abi.PngData(bit_depth=kw.get("bit_depth", 8), compression_level=kw.get("level", 5), dpi=kw.get("dpi", 0))
    return d


def test_bound_holds_the_level_0_noise_file_and_refuses():
    l = lib.load()
    for depth in (8, 16):
        for (w, h) in [(1, 1), (17, 33), (1001, 777)]:
            img = pr.frame("noise", w, h, depth, seed=w)
            d = _data(bit_depth=depth, level=0)
            stored = pr.host_file(img, 0)
            assert l.dt_hip_png_bound(w, h, C.byref(d)) >= 8 + len(stored)
            for level in (1, 9):
                d.compression_level = level
                assert l.dt_hip_png_bound(w, h, C.byref(d)) >= 8 + len(pr.host_file(img, level))
    icc = params.png(icc=b"x" * 200000)
    assert l.dt_hip_png_bound(65, 47, C.byref(icc)) >= 8 + len(pr.host_file(pr.frame("noise", 65, 47, 8), 0,
                                                                            icc=b"x" * 200000))
    for bad in (dict(bit_depth=12), dict(bit_depth=0), dict(level=-1), dict(level=10), dict(dpi=-1)):
        assert l.dt_hip_png_bound(16, 16, C.byref(_data(**bad))) == 0, bad
    assert l.dt_hip_png_bound(0, 16, C.byref(_data())) == 0
    assert l.dt_hip_png_bound(16, 0, C.byref(_data())) == 0
    assert l.dt_hip_png_bound(2 ** 31 - 1, 2 ** 31 - 1, C.byref(_data(bit_depth=16))) == 0  # row beyond 2^32 bytes
    assert l.dt_hip_png_bound(1431655765, 1, C.byref(_data())) == 0  # a row of 2^32 - 1 bytes


def test_struct_layout_params_and_with_png():
    l = lib.load()
    assert l.dt_hip_abi_sizeof(b"png") == C.sizeof(abi.PngData)
    assert [n for n, _ in abi.PngData._fields_] == ["bit_depth", "compression_level", "dpi", "capacity", "icc",
                                                     "icc_bytes"]
    assert abi.PngData.capacity.offset == 16 and abi.PngData.icc_bytes.offset == 32
    d = params.png()
    assert (d.bit_depth, d.compression_level, d.dpi, d.icc_bytes) == (8, 5, 0, 0)
    d = params.png(bpp=16, compression=9, icc=b"abc", dpi=300)
    assert (d.bit_depth, d.compression_level, d.dpi, d.icc_bytes) == (16, 9, 300, 3)
    assert C.string_at(d.icc, 3) == b"abc"
    for bad in (dict(bpp=12), dict(compression=10), dict(compression=-1), dict(dpi=0)):
        with pytest.raises(ValueError):
            params.png(**bad)
    piece = abi.Piece.make(64, 48, channels=4)
    nodes = [pipe.Node("colorout", None, piece), pipe.Node("export_u16", None, piece)]
    n8 = pipe.with_png(nodes, params.png())
    assert [n.op for n in n8] == ["colorout", "export_u8", "export_png"]
    n16 = pipe.with_png(nodes, params.png(bpp=16))
    assert [n.op for n in n16] == ["colorout", "export_u16", "export_png"]
    assert n16[-1].piece.roi_out.width == 64 and n16[-1].piece.roi_out.height == 48
    with pytest.raises(ValueError):
        pipe.with_png(nodes[:1], params.png())
    assert pipe.node_bytes_per_px(n8[-1]) == 4 and pipe.node_bytes_per_px(n16[-1]) == 8
