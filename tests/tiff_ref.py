"""The TIFF encoder's checkers (tests/test_tiff_host.py, tests/test_gpu_tiff.py, tests/test_gpu_tiff_pipe.py).

  * host() / host_file() / host_payload(): the encoder's body compiled for the host (tests/native/tiff_host.cpp over
    ansel_amd/csrc/tiff_body.h and png_deflate.h)
  * libtiff(): libtiff itself through ctypes (ctypes.util.find_library("tiff"), else the shared object inside Pillow's
    pillow.libs; None if there is none) -- libtiff_read() decodes a file strip by strip with TIFFReadEncodedStrip,
    libtiff_file() writes the same frame with the same settings, default_rows() is TIFFDefaultStripSize
  * payload_rows() / numpy_file() / parse() / check_layout() / decode(): a numpy restatement of the format -- the
    predictors, a writer (zlib's deflate), a reader of any little-endian classic TIFF in strips
  * frame() / CASES / variants(): the corpus, one table for the CPU and the GPU suite

Frames are (h, w, 4) arrays of uint8, uint16 or uint32; a 32-bit frame holds the floats' BITS, so that NaN payloads
compare."""
import ctypes as C
import ctypes.util
import glob
import os
import struct
import subprocess
import tempfile
import threading
import zlib

import numpy as np

from ansel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
DTYPES = {8: np.uint8, 16: np.uint16, 32: np.uint32}

_cache = {}


def _build_dir():
    if "dir" not in _cache:
        _cache["dir"] = tempfile.mkdtemp(prefix="tiff_ref_")
    return _cache["dir"]


def host():
    """the encoder's body compiled for the host"""
    if "host" not in _cache:
        so = os.path.join(_build_dir(), "libtiff_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-I" + os.path.join(ROOT, "ansel_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                               os.path.join(NATIVE, "tiff_host.cpp"), "-o", so])
        lib = C.CDLL(so)
        P = C.POINTER(abi.TiffData)
        lib.tiff_host_encode.restype = C.c_size_t
        lib.tiff_host_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, P]
        lib.tiff_host_copy.argtypes = [C.c_void_p]
        lib.tiff_host_payload.restype = C.c_size_t
        lib.tiff_host_payload.argtypes = [C.c_void_p, C.c_int, C.c_int, P, C.c_void_p]
        lib.tiff_host_bound.restype = C.c_size_t
        lib.tiff_host_bound.argtypes = [C.c_int, C.c_int, P]
        _cache["host"] = lib
    return _cache["host"]


def data(bpp, layers=3, compression=abi.DT_HIP_TIFF_NONE, predictor=1, level=6, rps=0, dpi=0, icc=None):
    d = abi.TiffData(bpp=bpp, layers=layers, compression=compression, predictor=predictor, compression_level=level,
                     rows_per_strip=rps, dpi=dpi)
    if icc:
        d._icc = C.create_string_buffer(bytes(icc), len(icc))
        d.icc = C.cast(d._icc, C.c_void_p)
        d.icc_bytes = len(icc)
    return d


def data_for(img, layers, variant, rps=0, dpi=0, icc=None):
    comp, pred, level = variant
    return data(8 * img.itemsize, layers, comp, pred, level, rps, dpi, icc)


def host_file(img, d):
    h, w = img.shape[:2]
    img = np.ascontiguousarray(img)
    n = host().tiff_host_encode(img.ctypes.data, w, h, C.byref(d))
    assert n > 0, "the host build refused the frame or disagrees with itself"
    out = np.empty(n, np.uint8)
    host().tiff_host_copy(out.ctypes.data)
    return out.tobytes()


def host_payload(img, d):
    h, w = img.shape[:2]
    img = np.ascontiguousarray(img)
    n = host().tiff_host_payload(img.ctypes.data, w, h, C.byref(d), None)
    out = np.empty(n, np.uint8)
    host().tiff_host_payload(img.ctypes.data, w, h, C.byref(d), out.ctypes.data)
    return out.tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# libtiff through ctypes

T_WIDTH, T_LENGTH, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_OFFSETS, T_ORIENTATION, T_SPP, T_RPS, T_COUNTS = (
    256, 257, 258, 259, 262, 273, 274, 277, 278, 279)
T_XRES, T_YRES, T_PLANAR, T_RESUNIT, T_PREDICTOR, T_SAMPLEFORMAT, T_ICC, T_ZIPQUALITY = (
    282, 283, 284, 296, 317, 339, 34675, 65557)


def _libtiff_candidates():
    name = ctypes.util.find_library("tiff")
    if name:
        yield name
    try:
        import PIL
        for so in sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs", "libtiff*.so*"))):
            yield so
    except ImportError:
        pass


def libtiff():
    """libtiff, or None where there is none; libtiff_name() says which"""
    if "tiff" not in _cache:
        lib = None
        for cand in _libtiff_candidates():
            try:
                lib = C.CDLL(cand)
                _cache["tiff_name"] = cand
                break
            except OSError:
                continue
        if lib is not None:
            lib.TIFFOpen.restype = C.c_void_p
            lib.TIFFOpen.argtypes = [C.c_char_p, C.c_char_p]
            lib.TIFFClose.argtypes = [C.c_void_p]
            lib.TIFFNumberOfStrips.restype = C.c_uint32
            lib.TIFFNumberOfStrips.argtypes = [C.c_void_p]
            lib.TIFFStripSize.restype = C.c_ssize_t
            lib.TIFFStripSize.argtypes = [C.c_void_p]
            lib.TIFFDefaultStripSize.restype = C.c_uint32
            lib.TIFFDefaultStripSize.argtypes = [C.c_void_p, C.c_uint32]
            lib.TIFFReadEncodedStrip.restype = C.c_ssize_t
            lib.TIFFReadEncodedStrip.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_ssize_t]
            lib.TIFFWriteEncodedStrip.restype = C.c_ssize_t
            lib.TIFFWriteEncodedStrip.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_ssize_t]
            lib.TIFFGetVersion.restype = C.c_char_p
            lib.TIFFSetField.restype = C.c_int  # variadic: every call converts its own arguments
            # warnings (an ICC profile that is no profile) go to stderr otherwise
            lib.TIFFSetWarningHandler.argtypes = [C.c_void_p]
            lib.TIFFSetWarningHandler(None)
        _cache["tiff"] = lib
    return _cache["tiff"]


def libtiff_name():
    l = libtiff()
    return None if l is None else "%s (%s)" % (_cache["tiff_name"], l.TIFFGetVersion().decode().split("\n")[0])


def _tmp(name):
    return os.path.join(_build_dir(), name).encode()


def libtiff_read(file_bytes):
    """every strip through TIFFReadEncodedStrip (libtiff undoes the predictor): the strips' samples as bytes, one
    after the other, in the machine's byte order"""
    l = libtiff()
    path = _tmp("read.tif")
    with open(path, "wb") as f:
        f.write(file_bytes)
    tif = l.TIFFOpen(path, b"r")
    assert tif, "libtiff does not open the file"
    try:
        size = l.TIFFStripSize(tif)
        buf = C.create_string_buffer(size)
        out = []
        for s in range(l.TIFFNumberOfStrips(tif)):
            n = l.TIFFReadEncodedStrip(tif, s, buf, size)
            assert n > 0, "libtiff does not read strip %d" % s
            out.append(buf.raw[:n])
        return b"".join(out)
    finally:
        l.TIFFClose(tif)


def _set(l, tif, tag, *args):
    assert l.TIFFSetField(C.c_void_p(tif), C.c_uint32(tag), *args) == 1, tag


def _libtiff_setup(l, tif, w, h, d):
    _set(l, tif, T_WIDTH, C.c_uint32(w))
    _set(l, tif, T_LENGTH, C.c_uint32(h))
    _set(l, tif, T_BITS, C.c_int(d.bpp))
    _set(l, tif, T_COMPRESSION, C.c_int(d.compression))
    _set(l, tif, T_PHOTOMETRIC, C.c_int(2 if d.layers == 3 else 1))
    _set(l, tif, T_ORIENTATION, C.c_int(1))
    _set(l, tif, T_SPP, C.c_int(d.layers))
    _set(l, tif, T_PLANAR, C.c_int(1))
    _set(l, tif, T_SAMPLEFORMAT, C.c_int(3 if d.bpp == 32 else 1))
    if d.dpi:
        _set(l, tif, T_XRES, C.c_double(d.dpi))
        _set(l, tif, T_YRES, C.c_double(d.dpi))
        _set(l, tif, T_RESUNIT, C.c_int(2))
    if d.compression == abi.DT_HIP_TIFF_DEFLATE:
        _set(l, tif, T_ZIPQUALITY, C.c_int(d.compression_level))
        if d.predictor != 1:
            _set(l, tif, T_PREDICTOR, C.c_int(d.predictor))
    if d.icc_bytes:
        _set(l, tif, T_ICC, C.c_uint32(d.icc_bytes), C.c_void_p(d.icc))
    rps = d.rows_per_strip or l.TIFFDefaultStripSize(tif, 0)
    _set(l, tif, T_RPS, C.c_uint32(rps))
    return rps


def libtiff_file(img, d):
    """the file libtiff writes from the same frame with the same settings (TIFFWriteEncodedStrip per strip; libtiff
    differences the buffer it is handed in place, so every strip is a copy)"""
    l = libtiff()
    h, w = img.shape[:2]
    rows = np.ascontiguousarray(img[..., :d.layers])
    path = _tmp("write_%d.tif" % threading.get_ident())  # tools/bench_tiff.py writes from several threads
    tif = l.TIFFOpen(path, b"w")
    assert tif
    try:
        rps = _libtiff_setup(l, tif, w, h, d)
        for s, y in enumerate(range(0, h, rps)):
            b = rows[y:y + rps].tobytes()
            buf = C.create_string_buffer(b, len(b))
            assert l.TIFFWriteEncodedStrip(tif, s, buf, len(b)) == len(b)
    finally:
        l.TIFFClose(tif)
    with open(path, "rb") as f:
        return f.read()


def default_rows(w, bpp, layers):
    """TIFFDefaultStripSize(tif, 0) of a frame this wide"""
    l = libtiff()
    tif = l.TIFFOpen(_tmp("rows.tif"), b"w")
    assert tif
    try:
        _set(l, tif, T_WIDTH, C.c_uint32(w))
        _set(l, tif, T_BITS, C.c_int(bpp))
        _set(l, tif, T_SPP, C.c_int(layers))
        _set(l, tif, T_PLANAR, C.c_int(1))
        return int(l.TIFFDefaultStripSize(tif, 0))
    finally:
        l.TIFFClose(tif)


# ----------------------------------------------------------------------------------------------------------------------
# the numpy restatement

def payload_rows(img, layers, predictor):
    """(h, row bytes) uint8: what a strip holds before compression"""
    rows = np.ascontiguousarray(img[..., :layers]).reshape(img.shape[0], -1)
    h, n = rows.shape
    if predictor == 2:
        d = rows.copy()
        d[:, layers:] = rows[:, layers:] - rows[:, :-layers]
        rows = d
    if predictor == 3:
        planes = rows.astype(">u4").view(np.uint8).reshape(h, n, 4).transpose(0, 2, 1).reshape(h, 4 * n)
        d = planes.copy()
        d[:, layers:] = planes[:, layers:] - planes[:, :-layers]
        return d
    return rows.astype(rows.dtype.newbyteorder("<")).view(np.uint8).reshape(h, -1)


def unpredict(rows_u8, w, layers, bpp, predictor):
    """payload_rows() undone: (h, w, layers) samples"""
    h = rows_u8.shape[0]
    if predictor == 3:
        planes = np.cumsum(rows_u8.reshape(h, -1, layers), axis=1, dtype=np.uint8).reshape(h, 4, w * layers)
        return np.ascontiguousarray(planes.transpose(0, 2, 1)).view(">u4").astype(np.uint32).reshape(h, w, layers)
    dt = np.dtype(DTYPES[bpp]).newbyteorder("<")
    s = np.ascontiguousarray(rows_u8).view(dt).astype(DTYPES[bpp]).reshape(h, w, layers)
    return np.cumsum(s, axis=1, dtype=DTYPES[bpp]) if predictor == 2 else s


TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 7: 1, 16: 8}


def parse(f):
    """a little-endian classic TIFF: {tag: values} (a tuple of ints; RATIONAL as (num, den) pairs; UNDEFINED as bytes), and
    where the IFD and its out-of-line values stand: [(offset, bytes)]"""
    assert f[:4] == b"II*\0"
    ifd, = struct.unpack_from("<I", f, 4)
    n, = struct.unpack_from("<H", f, ifd)
    tags, spans, last = {}, [(0, 8), (ifd, 2 + 12 * n + 4)], 0
    for k in range(n):
        tag, typ, count = struct.unpack_from("<HHI", f, ifd + 2 + 12 * k)
        assert tag > last, "tags are not ascending"
        last = tag
        size = TYPE_SIZE[typ] * count
        at = ifd + 2 + 12 * k + 8
        if size > 4:
            at, = struct.unpack_from("<I", f, at)
            assert at % 2 == 0, "tag %d's value stands on an odd offset" % tag
            spans.append((at, size))
        raw = f[at:at + size]
        assert len(raw) == size
        if typ == 3:
            v = struct.unpack("<%dH" % count, raw)
        elif typ == 4:
            v = struct.unpack("<%dI" % count, raw)
        elif typ == 5:
            v = tuple(struct.unpack("<II", raw[8 * i:8 * i + 8]) for i in range(count))
        else:
            v = raw
        tags[tag] = v
    assert struct.unpack_from("<I", f, ifd + 2 + 12 * n)[0] == 0, "a second IFD"
    return tags, spans


def strips(f):
    tags, _ = parse(f)
    return list(zip(tags[T_OFFSETS], tags[T_COUNTS]))


def check_layout(f):
    """head and values do not overlap, the strips follow them in ascending order without overlap, each on an even
    offset at most one zero byte behind the one before, and the last one ends the file"""
    tags, spans = parse(f)
    spans.sort()
    for (a, n), (b, _) in zip(spans, spans[1:]):
        assert a + n <= b, "values overlap"
        assert b - (a + n) <= 1 and not any(f[a + n:b]), "more than a zero pad byte between values"
    at = spans[-1][0] + spans[-1][1]
    for off, cnt in zip(tags[T_OFFSETS], tags[T_COUNTS]):
        assert off % 2 == 0 and cnt > 0
        assert off == at + (at & 1), "strip at %d, expected %d" % (off, at + (at & 1))
        assert not any(f[at:off])
        at = off + cnt
    assert at == len(f), "the strips end at %d, the file at %d" % (at, len(f))


def strip_payloads(f):
    """every strip's bytes before compression (each strip inflated on its own: zlib checks its Adler-32)"""
    tags, _ = parse(f)
    out = []
    for off, cnt in zip(tags[T_OFFSETS], tags[T_COUNTS]):
        b = f[off:off + cnt]
        out.append(zlib.decompress(b) if tags[T_COMPRESSION][0] == 8 else b)
    return out


def decode(f):
    """the numpy reader: (h, w, layers) samples (32 bits: the floats' bits)"""
    tags, _ = parse(f)
    w, h, bpp, layers = tags[T_WIDTH][0], tags[T_LENGTH][0], tags[T_BITS][0], tags[T_SPP][0]
    pred = tags.get(T_PREDICTOR, (1,))[0]
    rows = np.frombuffer(b"".join(strip_payloads(f)), np.uint8).reshape(h, -1)
    return unpredict(rows, w, layers, bpp, pred)


def numpy_file(img, d):
    """the numpy writer of the same format (zlib's deflate): what the issue's restatement is"""
    h, w = img.shape[:2]
    rb = w * d.layers * d.bpp // 8
    rps = d.rows_per_strip or max(1, 8192 // rb)
    rows = payload_rows(img, d.layers, d.predictor)
    blobs = []
    for y in range(0, h, rps):
        b = rows[y:y + rps].tobytes()
        blobs.append(zlib.compress(b, d.compression_level) if d.compression == 8 else b)
    ns = len(blobs)
    icc = C.string_at(d.icc, d.icc_bytes) if d.icc_bytes else b""
    e = [(256, 4, [w]), (257, 4, [h]), (258, 3, [d.bpp] * d.layers), (259, 3, [d.compression]),
         (262, 3, [2 if d.layers == 3 else 1]), (273, 4, [0] * ns), (274, 3, [1]), (277, 3, [d.layers]), (278, 4, [rps]),
         (279, 4, [len(b) for b in blobs])]
    if d.dpi:
        e += [(282, 5, [(d.dpi, 1)]), (283, 5, [(d.dpi, 1)])]
    e += [(284, 3, [1])]
    if d.dpi:
        e += [(296, 3, [2])]
    if d.predictor != 1:
        e += [(317, 3, [d.predictor])]
    e += [(339, 3, [3 if d.bpp == 32 else 1] * d.layers)]
    if icc:
        e += [(34675, 7, icc)]

    def pack(typ, v):
        if typ == 7:
            return bytes(v)
        if typ == 5:
            return b"".join(struct.pack("<II", *p) for p in v)
        return struct.pack("<%d%s" % (len(v), "H" if typ == 3 else "I"), *v)
    at = 8 + 2 + 12 * len(e) + 4
    where = []
    for tag, typ, v in e:
        size = len(pack(typ, v))
        if size <= 4:
            where.append(None)
            continue
        at += at & 1
        where.append(at)
        at += size
    offs = []
    for b in blobs:
        at += at & 1
        offs.append(at)
        at += len(b)
    e[5] = (273, 4, offs)
    out = bytearray(at)
    out[:8] = b"II*\0" + struct.pack("<I", 8)
    struct.pack_into("<H", out, 8, len(e))
    for k, (tag, typ, v) in enumerate(e):
        raw = pack(typ, v)
        count = len(raw) // TYPE_SIZE[typ]
        struct.pack_into("<HHI", out, 10 + 12 * k, tag, typ, count)
        if where[k] is None:
            out[10 + 12 * k + 8:10 + 12 * k + 8 + len(raw)] = raw
        else:
            struct.pack_into("<I", out, 10 + 12 * k + 8, where[k])
            out[where[k]:where[k] + len(raw)] = raw
    for o, b in zip(offs, blobs):
        out[o:o + len(b)] = b
    return bytes(out)


# ----------------------------------------------------------------------------------------------------------------------
# the corpus

SPECIAL_FLOATS = np.array([0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x7fbfffff, 0x00000000, 0x80000000, 0x00000001,
                           0x807fffff, 0x00400000, 0x7f800000, 0xff800000, 0x3f800000, 0xbf800000, 0x7f7fffff, 0x00800000],
                          np.uint32)


def frame(kind, w, h, bpp, seed=0):
    """RGBA (alpha random: the encoder ignores it); 32 bits: floats in [0, 1) as bits, or the special values"""
    rng = np.random.default_rng(seed)
    dt = DTYPES[bpp]
    top = {8: 255, 16: 65535, 32: 1}[bpp]
    x = np.arange(w)[None, :, None] / max(w - 1, 1)
    y = np.arange(h)[:, None, None] / max(h - 1, 1)
    c = np.arange(4)[None, None, :]
    if kind == "noise":
        v = rng.random((h, w, 4))
    elif kind == "gradient":  # smooth: it compresses, and the predictors make it compress better
        v = (x * (1 + c) / 4 + y * (4 - c) / 4) / 2
    elif kind == "mix":  # smooth on the left, noise on the right
        v = np.where(x < 0.5, (x + y) / 2 + 0 * c, rng.random((h, w, 4)))
    elif kind == "rows":  # every row equal: a window that crossed a strip would find the row above
        v = np.broadcast_to(rng.random((1, w, 4)), (h, w, 4))
    elif kind == "period":  # a pattern that repeats every 1000 pixels: long matches, also across a segment's border
        v = np.broadcast_to(rng.random((1, 1000, 4)), (h, 1000, 4))
        v = np.tile(v, (1, (w + 999) // 1000, 1))[:, :w]
    elif kind == "special":
        assert bpp == 32
        img = SPECIAL_FLOATS[rng.integers(0, len(SPECIAL_FLOATS), (h, w, 4))]
        img[0, 0, :3] = SPECIAL_FLOATS[:3]
        return np.ascontiguousarray(img)
    else:
        raise ValueError(kind)
    if bpp == 32:
        img = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
    else:
        img = np.ascontiguousarray(np.floor(v * top + 0.5), dt)
    img[..., 3] = rng.integers(0, 256, (h, w)).astype(dt)
    return np.ascontiguousarray(img)


def variants(bpp):
    """(compression, predictor, level): none; deflate at levels 0, 1 and 6 with predictor 1 and the format's own"""
    own = 3 if bpp == 32 else 2
    return [(abi.DT_HIP_TIFF_NONE, 1, 0)] + [(abi.DT_HIP_TIFF_DEFLATE, p, lv) for lv in (0, 1, 6) for p in (1, own)]


def _cases():
    out = []
    # the general shapes in all six formats
    for (w, h, rps) in [(1, 1, 5), (1, 5, 5), (2, 1, 5), (37, 13, 5), (37, 13, 13), (37, 13, 100), (37, 13, 1)]:
        for bpp in (8, 16, 32):
            for layers in (3, 1):
                out.append(("%dx%d_rps%d_%d_%d" % (w, h, rps, bpp, layers), "mix" if w > 2 else "noise", w, h, bpp, layers, rps))
    out += [
        ("one_segment", "mix", 32768, 2, 8, 1, 1),            # a strip of exactly one segment
        ("one_byte_over", "mix", 10923, 3, 8, 3, 1),          # 32 769 B: one byte into a second segment
        ("two_bytes_over", "mix", 16385, 2, 16, 1, 0),        # 32 770 B
        ("three_segments", "period", 2000, 16, 16, 3, 7),     # strips of 84 000, 84 000, 24 000 B: matches across a border
        ("many_strips", "mix", 3, 1025, 8, 3, 1),             # 1 025 strips: more than threads in the scan
        ("equal_rows_u8", "rows", 300, 40, 8, 3, 1),
        ("equal_rows_f32", "rows", 300, 40, 32, 3, 1),
        ("special_37x13_rgb", "special", 37, 13, 32, 3, 5),
        ("special_37x13_gray", "special", 37, 13, 32, 1, 5),
        ("special_1x3_rgb", "special", 1, 3, 32, 3, 1),
        ("special_1x3_gray", "special", 1, 3, 32, 1, 0),
        # rows_per_strip 0: row bytes 1, 300, 8190, 8192, 8193, 8196
        ("default_rows_1", "noise", 1, 5, 8, 1, 0),
        ("default_rows_300", "gradient", 100, 60, 8, 3, 0),
        ("default_rows_8190", "gradient", 1365, 3, 16, 3, 0),
        ("default_rows_8192", "gradient", 2048, 3, 32, 1, 0),
        ("default_rows_8193", "gradient", 2731, 3, 8, 3, 0),
        ("default_rows_8196", "gradient", 683, 3, 32, 3, 0),
    ]
    return out


CASES = _cases()
COMPRESSIBLE = ["default_rows_300", "default_rows_8190", "default_rows_8192", "default_rows_8193", "default_rows_8196",
                "three_segments", "equal_rows_u8"]


def case(name):
    """(frame, layers, rows_per_strip) of a CASES entry; the frame is made once"""
    key = ("case", name)
    if key not in _cache:
        _, kind, w, h, bpp, layers, rps = next(c for c in CASES if c[0] == name)
        img = frame(kind, w, h, bpp, seed=len(name) + w)
        img.setflags(write=False)
        _cache[key] = (img, layers, rps)
    return _cache[key]


def case_file(name, variant, who="host"):
    """the host build's (who "host") or libtiff's ("libtiff") file of a CASES entry in one variant, made once"""
    key = (who, name, variant)
    if key not in _cache:
        img, layers, rps = case(name)
        d = data_for(img, layers, variant, rps)
        _cache[key] = host_file(img, d) if who == "host" else libtiff_file(img, d)
    return _cache[key]


def samples(img, layers):
    """the bytes a reader must return: `layers` samples a pixel, row by row"""
    return np.ascontiguousarray(img[..., :layers]).tobytes()
