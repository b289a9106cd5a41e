"""not gpu: the TIFF encoder's body compiled for the host (tests/native/tiff_host.cpp, loaded by tests/tiff_ref.py) -- the
file the device must reproduce byte for byte (tests/test_gpu_tiff.py), checked here against libtiff itself.

On every entry of tiff_ref.CASES in every variant that fits it (no compression; deflate at levels 0, 1 and 6, each with
predictor 1 and with the format's own):
  * libtiff (TIFFReadEncodedStrip through ctypes) returns the input's samples bit for bit -- compared as bytes, so NaN
    payloads count -- and so does Pillow where it is exact (8-bit RGB, 8 / 16-bit gray, float gray)
  * every strip inflates on its own (zlib checks its Adler-32) to the strip of the file libtiff writes from the same frame
    with the same settings, and to the numpy restatement's rows
  * every tag's value equals the one in libtiff's file (StripOffsets exempt, StripByteCounts under deflate)
  * the strips do not overlap, ascend, start even and end at L; without compression their bytes are libtiff's
  * two encodes are identical; rows_per_strip 0 follows TIFFDefaultStripSize; dt_hip_tiff_bound() is at least L and 0 for
    every refused setting
  * at level 6 with the predictor the compressible frames' strips take the measured multiple of libtiff's (DESIGN.md
    section 4.8), guarded at + 2 %
Without a loadable libtiff the libtiff tests skip; the restatement tests run regardless."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import tiff_ref as tr
from ansel_amd import abi, lib

NAMES = [c[0] for c in tr.CASES]
needs_libtiff = pytest.mark.skipif(tr.libtiff() is None, reason="no libtiff can be loaded")


def each_variant(name):
    img, layers, rps = tr.case(name)
    for v in tr.variants(8 * img.itemsize):
        yield img, layers, rps, v, tr.case_file(name, v)


def test_the_libtiff_in_use():
    print("libtiff:", tr.libtiff_name())


@needs_libtiff
@pytest.mark.parametrize("name", NAMES)
def test_libtiff_reads_the_samples_back(name):
    for img, layers, rps, v, f in each_variant(name):
        assert tr.libtiff_read(f) == tr.samples(img, layers), v


@pytest.mark.parametrize("name", NAMES)
def test_pillow_reads_the_samples_back_where_it_is_exact(name):
    Image = pytest.importorskip("PIL.Image")
    img, layers, rps = tr.case(name)
    bpp = 8 * img.itemsize
    if not ((bpp == 8 and layers == 3) or layers == 1):
        return  # Pillow reduces 16-bit RGB to 8 bits and refuses float RGB
    Image.MAX_IMAGE_PIXELS = None
    for img, layers, rps, v, f in each_variant(name):
        got = np.asarray(Image.open(io.BytesIO(f)))
        assert got.tobytes() == tr.samples(img, layers), v


@pytest.mark.parametrize("name", NAMES)
def test_every_strip_inflates_alone_to_the_restatement(name):
    for img, layers, rps, v, f in each_variant(name):
        tags, _ = tr.parse(f)
        rows = tr.payload_rows(img, layers, v[1])
        per = tags[tr.T_RPS][0]
        want = [rows[y:y + per].tobytes() for y in range(0, img.shape[0], per)]
        assert tr.strip_payloads(f) == want, v
        assert b"".join(want) == tr.host_payload(img, tr.data_for(img, layers, v, rps)), v
        assert tr.decode(f).tobytes() == tr.samples(img, layers), v
        if v[0] == abi.DT_HIP_TIFF_DEFLATE:
            for off, cnt in tr.strips(f):
                z = zlib.decompressobj()
                z.decompress(f[off:off + cnt])
                assert z.eof and not z.unused_data, v  # the byte count is the stream, no more and no less


@needs_libtiff
@pytest.mark.parametrize("name", NAMES)
def test_strips_and_tags_equal_libtiffs_file(name):
    for img, layers, rps, v, f in each_variant(name):
        ref = tr.case_file(name, v, "libtiff")
        assert tr.strip_payloads(f) == tr.strip_payloads(ref), v
        ours, _ = tr.parse(f)
        theirs, _ = tr.parse(ref)
        assert sorted(ours) == sorted(theirs), v
        for tag in ours:
            if tag == tr.T_OFFSETS or (tag == tr.T_COUNTS and v[0] == abi.DT_HIP_TIFF_DEFLATE):
                continue
            assert tuple(ours[tag]) == tuple(theirs[tag]), (v, tag)
        if v[0] == abi.DT_HIP_TIFF_NONE:
            assert [f[o:o + c] for o, c in tr.strips(f)] == [ref[o:o + c] for o, c in tr.strips(ref)]


@pytest.mark.parametrize("name", NAMES)
def test_layout_bound_and_determinism(name):
    l = lib.load()
    for img, layers, rps, v, f in each_variant(name):
        tr.check_layout(f)
        d = tr.data_for(img, layers, v, rps)
        h, w = img.shape[:2]
        bound = l.dt_hip_tiff_bound(w, h, C.byref(d))
        assert bound == tr.host().tiff_host_bound(w, h, C.byref(d))
        assert bound >= 8 + len(f), v
        if v[0] == abi.DT_HIP_TIFF_NONE:
            assert bound == 8 + len(f)
        assert tr.host_file(img, d) == f, v


@needs_libtiff
@pytest.mark.parametrize("w,bpp,layers,row_bytes,rows", [(1, 8, 1, 1, 8192), (100, 8, 3, 300, 27), (1365, 16, 3, 8190, 1),
                                                         (2048, 32, 1, 8192, 1), (2731, 8, 3, 8193, 1), (683, 32, 3, 8196, 1)])
def test_default_rows_per_strip_is_libtiffs_rule(w, bpp, layers, row_bytes, rows):
    assert w * layers * bpp // 8 == row_bytes
    assert tr.default_rows(w, bpp, layers) == rows
    img = tr.frame("noise", w, 5, bpp, seed=w)
    tags, _ = tr.parse(tr.host_file(img, tr.data(bpp, layers)))
    assert tags[tr.T_RPS][0] == rows  # the tag keeps the rule's value even where the frame has fewer rows
    assert len(tags[tr.T_OFFSETS]) == (5 + rows - 1) // rows


ODD = dict(bpp=8, layers=3, compression=abi.DT_HIP_TIFF_DEFLATE, predictor=2, level=6, rps=5, dpi=300)


@pytest.mark.parametrize("icc_bytes", [1, 200001])
def test_icc_dpi_and_strips_of_odd_length(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    img = tr.frame("mix", 37, 13, 8, seed=5)
    seen_odd = False
    for comp in (abi.DT_HIP_TIFF_DEFLATE, abi.DT_HIP_TIFF_NONE):
        d = tr.data(**dict(ODD, compression=comp, predictor=2 if comp == abi.DT_HIP_TIFF_DEFLATE else 1, icc=icc))
        f = tr.host_file(img, d)
        tr.check_layout(f)
        tags, _ = tr.parse(f)
        assert tags[tr.T_ICC] == icc and tags[tr.T_XRES] == ((300, 1),) and tags[tr.T_YRES] == ((300, 1),)
        assert tags[tr.T_RESUNIT] == (2,)
        seen_odd = seen_odd or any(c & 1 for c in tags[tr.T_COUNTS][:-1])
        assert tr.decode(f).tobytes() == tr.samples(img, 3)
        if tr.libtiff() is not None:
            assert tr.libtiff_read(f) == tr.samples(img, 3)
            theirs, _ = tr.parse(tr.libtiff_file(img, d))
            for tag in (tr.T_ICC, tr.T_XRES, tr.T_YRES, tr.T_RESUNIT):
                assert tuple(theirs[tag]) == tuple(tags[tag]), tag
    assert seen_odd, "no strip of odd length in front of another: the pad byte is not exercised"


def test_numpy_writer_is_the_same_format():
    """the restatement's own file: the same head as the host build's without compression, and read back by libtiff"""
    for name in ("37x13_rps5_16_3", "special_37x13_rgb", "default_rows_300"):
        img, layers, rps = tr.case(name)
        for v in tr.variants(8 * img.itemsize):
            d = tr.data_for(img, layers, v, rps)
            f = tr.numpy_file(img, d)
            tr.check_layout(f)
            if v[0] == abi.DT_HIP_TIFF_NONE:
                assert f == tr.case_file(name, v)
            if tr.libtiff() is not None:
                assert tr.libtiff_read(f) == tr.samples(img, layers), (name, v)


REFUSED = [dict(bpp=12), dict(bpp=0), dict(layers=2), dict(layers=4), dict(compression=5), dict(compression=0),
           dict(predictor=0), dict(predictor=4), dict(bpp=32, predictor=2), dict(bpp=8, predictor=3), dict(bpp=16, predictor=3),
           dict(compression=abi.DT_HIP_TIFF_NONE, predictor=2), dict(level=-1), dict(level=10), dict(rps=-1), dict(dpi=-1)]


def test_bound_is_zero_for_every_refused_setting():
    l = lib.load()
    ok = dict(bpp=8, layers=3, compression=abi.DT_HIP_TIFF_DEFLATE, predictor=1, level=6)
    assert l.dt_hip_tiff_bound(16, 16, C.byref(tr.data(**ok))) > 0
    for bad in REFUSED:
        d = tr.data(**dict(ok, **bad))
        assert l.dt_hip_tiff_bound(16, 16, C.byref(d)) == 0, bad
        assert b"dt_hip_tiff_bound" in l.dt_hip_last_error(), bad
        assert tr.host().tiff_host_bound(16, 16, C.byref(d)) == 0, bad
    for w, h in ((0, 4), (4, 0), (-1, 4)):
        assert l.dt_hip_tiff_bound(w, h, C.byref(tr.data(**ok))) == 0
    no_icc = tr.data(**ok)
    no_icc.icc_bytes = 4
    assert l.dt_hip_tiff_bound(16, 16, C.byref(no_icc)) == 0
    # classic TIFF only: 2^32 bytes of rows do not fit 32-bit offsets
    assert l.dt_hip_tiff_bound(32768, 32768, C.byref(tr.data(32, 1))) == 0
    assert l.dt_hip_tiff_bound(32768, 32768, C.byref(tr.data(8, 3))) > 0


# sum of StripByteCounts at level 6 with the format's predictor, over libtiff's (zlib level 6) for the same strips: MEASURED
# on the host build, which is deterministic and equals the device (DESIGN.md section 4.8 has the table and why the smooth
# ramps cost so much more than a photograph: one candidate per hash and no chain, against zlib's search)
MEASURED_RATIO = {"default_rows_300": 2.0996, "default_rows_8190": 2.7132, "default_rows_8192": 7.8067,
                  "default_rows_8193": 3.7848, "default_rows_8196": 3.6311, "three_segments": 1.0257, "equal_rows_u8": 1.0000}
MEASURED_TOTAL = 1.1544


@needs_libtiff
def test_level_6_size_against_libtiff():
    ours_all = theirs_all = 0
    for name in tr.COMPRESSIBLE:
        img, layers, rps = tr.case(name)
        v = (abi.DT_HIP_TIFF_DEFLATE, 3 if img.itemsize == 4 else 2, 6)
        ours = sum(c for _, c in tr.strips(tr.case_file(name, v)))
        theirs = sum(c for _, c in tr.strips(tr.case_file(name, v, "libtiff")))
        print("%-20s %7d B, libtiff %7d B, ratio %.4f" % (name, ours, theirs, ours / theirs))
        assert ours / theirs <= MEASURED_RATIO[name] + 0.02, name
        ours_all += ours
        theirs_all += theirs
    print("all: ratio %.4f" % (ours_all / theirs_all))
    assert ours_all / theirs_all <= MEASURED_TOTAL + 0.02


def test_ctypes_mirror_of_the_struct():
    assert lib.load().dt_hip_abi_sizeof(b"tiff") == C.sizeof(abi.TiffData)
