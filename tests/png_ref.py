"""The PNG encoder's checkers (tests/test_png_host.py, tests/test_gpu_png.py, tests/test_gpu_png_pipe.py).

  * ref():    libpng 1.6 with Ansel's settings (tests/native/png_ref.c, compiled here against the libpng found on
              the machine; None if there is none): the reference file, and a reader for the encoder's files
  * host():   the encoder's body compiled for the host (tests/native/png_host.cpp over ansel_amd/csrc/png_deflate.h)
  * filtered(): a numpy restatement of libpng's filter choice (png_write_find_filter)
  * chunks() / idat_stream() / unfilter(): the file taken apart"""
import ctypes as C
import os
import subprocess
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
PNG_PREFIXES = ["/opt/conda", "/usr", "/usr/local"]

SIZES = [(1, 1), (2, 3), (7, 9), (16, 16), (17, 33), (130, 67), (1001, 777)]
KINDS = ["gradient", "zero", "full", "noise", "primaries"]

_cache = {}


def _build_dir():
    if "dir" not in _cache:
        _cache["dir"] = tempfile.mkdtemp(prefix="png_ref_")
    return _cache["dir"]


def libpng_prefix():
    for p in PNG_PREFIXES:
        if os.path.exists(os.path.join(p, "include", "png.h")) and any(
                os.path.exists(os.path.join(p, "lib", n)) for n in ("libpng16.so", "libpng.so")):
            return p
    return None


def ref():
    """the libpng harness, or None where libpng is absent"""
    if "ref" not in _cache:
        p = libpng_prefix()
        lib = None
        if p is not None:
            so = os.path.join(_build_dir(), "libpng_ref.so")
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I" + os.path.join(p, "include"),
                                   os.path.join(NATIVE, "png_ref.c"), "-o", so, "-L" + os.path.join(p, "lib"),
                                   "-lpng16", "-Wl,-rpath," + os.path.join(p, "lib")])
            lib = C.CDLL(so)
            lib.ref_write.restype = C.c_size_t
            lib.ref_write.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
            lib.ref_free.argtypes = [C.c_void_p]
            lib.ref_read.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        _cache["ref"] = lib
    return _cache["ref"]


def host():
    """the encoder's body compiled for the host"""
    if "host" not in _cache:
        so = os.path.join(_build_dir(), "libpng_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-I" + os.path.join(ROOT, "ansel_amd", "csrc"), os.path.join(NATIVE, "png_host.cpp"),
                               "-o", so])
        lib = C.CDLL(so)
        lib.png_host_filtered.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.png_host_encode.restype = C.c_size_t
        lib.png_host_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.c_int]
        lib.png_host_copy.argtypes = [C.c_void_p]
        _cache["host"] = lib
    return _cache["host"]


def frame(kind, w, h, depth, seed=0):
    """RGBA u8 or u16 (alpha random: the encoder ignores it)"""
    rng = np.random.default_rng(seed)
    top = 255 if depth == 8 else 65535
    dt = np.uint8 if depth == 8 else np.uint16
    img = np.empty((h, w, 4), dt)
    if kind == "gradient":
        x = np.linspace(0, top, w)[None, :]
        y = np.linspace(0, top, h)[:, None]
        img[..., 0] = x
        img[..., 1] = y
        img[..., 2] = (x + y) / 2
    elif kind == "zero":
        img[..., :3] = 0
    elif kind == "full":
        img[..., :3] = top
    elif kind == "noise":
        img[..., :3] = rng.integers(0, top + 1, (h, w, 3))
    elif kind == "primaries":
        k = (np.arange(w)[None, :] // 5 + np.arange(h)[:, None] // 3) % 3
        img[..., :3] = 0
        for c in range(3):
            img[..., c][k == c] = top
    else:
        raise ValueError(kind)
    img[..., 3] = rng.integers(0, top + 1, (h, w))
    return img


def rgb_bytes(img):
    """the RGB samples in libpng's row order, native byte order"""
    return np.ascontiguousarray(img[..., :3])


def raw_rows(img):
    """the PNG raw rows (h, w * bpp) as uint8: RGB, 16-bit samples big-endian"""
    rgb = rgb_bytes(img)
    if rgb.dtype == np.uint16:
        rgb = rgb.astype(">u2")
    h = rgb.shape[0]
    return np.frombuffer(rgb.tobytes(), np.uint8).reshape(h, -1)


def filtered(img):
    """libpng 1.6 png_write_find_filter(): per row the smallest sum of |signed byte| of None, Sub, Up, Average, Paeth
    (in this order, strict <), against a zero row above the first"""
    raw = raw_rows(img).astype(np.int32)
    h, rb = raw.shape
    bpp = 3 if img.dtype == np.uint8 else 6
    prev = np.zeros(rb, np.int32)
    out = np.empty((h, rb + 1), np.uint8)
    for y in range(h):
        x = raw[y]
        a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        b = prev
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        p = b - c
        pc = a - c
        pa, pb, pcc = np.abs(p), np.abs(pc), np.abs(p + pc)
        pr = np.where((pa <= pb) & (pa <= pcc), a, np.where(pb <= pcc, b, c))
        cands = [x, x - a, x - b, x - (a + b) // 2, x - pr]
        best, bsum = None, None
        for f, r in enumerate(cands):
            r = r & 255
            s = int(np.where(r < 128, r, 256 - r).sum())
            if bsum is None or s < bsum:
                best, bsum = (f, r), s
        out[y, 0] = best[0]
        out[y, 1:] = best[1]
        prev = x
    return out.tobytes()


def unfilter(stream, w, h, depth):
    """the raw rows back from a filtered stream (numpy), as RGB u8 or native u16"""
    bpp = 3 if depth == 8 else 6
    rb = w * bpp
    f = np.frombuffer(stream, np.uint8).reshape(h, rb + 1)
    prev = np.zeros(rb, np.int32)
    rows = np.empty((h, rb), np.uint8)
    for y in range(h):
        t, d = int(f[y, 0]), f[y, 1:].astype(np.int32)
        cur = np.zeros(rb, np.int32)
        for j in range(rb):
            a = cur[j - bpp] if j >= bpp else 0
            b = prev[j]
            c = prev[j - bpp] if j >= bpp else 0
            if t == 0:
                pr = 0
            elif t == 1:
                pr = a
            elif t == 2:
                pr = b
            elif t == 3:
                pr = (a + b) // 2
            else:
                p = b - c
                pa, pb, pcc = abs(p), abs(a - c), abs(p + a - c)
                pr = a if (pa <= pb and pa <= pcc) else b if pb <= pcc else c
            cur[j] = (d[j] + pr) & 255
        rows[y] = cur
        prev = cur
    if depth == 8:
        return rows.reshape(h, w, 3)
    return np.frombuffer(rows.tobytes(), ">u2").astype(np.uint16).reshape(h, w, 3)


def chunks(data):
    """[(type, payload, crc_ok)]; asserts the signature"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, i = [], 8
    while i < len(data):
        n = int.from_bytes(data[i:i + 4], "big")
        t = data[i + 4:i + 8]
        p = data[i + 8:i + 8 + n]
        crc = int.from_bytes(data[i + 8 + n:i + 12 + n], "big")
        out.append((t.decode("latin1"), p, crc == zlib.crc32(t + p)))
        i += 12 + n
    assert i == len(data)
    return out


def idat_stream(data):
    """the zlib stream of the IDAT chunks"""
    return b"".join(p for t, p, _ in chunks(data) if t == "IDAT")


def inflate(data):
    return zlib.decompress(idat_stream(data))


def libpng_file(img, level):
    """libpng's file for the frame at `level`"""
    lib = ref()
    rgb = rgb_bytes(img)
    h, w = rgb.shape[:2]
    p = C.c_void_p()
    n = lib.ref_write(rgb.ctypes.data, w, h, 8 * rgb.itemsize, level, C.byref(p))
    assert n > 0
    out = C.string_at(p, n)
    lib.ref_free(p)
    return out


def libpng_read(data, w, h, depth):
    """(rgb, icc_bytes, ppm) as libpng decodes the file; None if it refuses it"""
    rgb = np.empty((h, w, 3), np.uint8 if depth == 8 else np.uint16)
    ib, ppm = C.c_uint(), C.c_uint()
    if ref().ref_read(data, len(data), w, h, depth, rgb.ctypes.data, C.byref(ib), C.byref(ppm)) != 0:
        return None
    return rgb, ib.value, ppm.value


def host_filtered(img):
    h, w = img.shape[:2]
    depth = 8 * img.itemsize
    n = h * (1 + w * 3 * img.itemsize)
    out = np.empty(n, np.uint8)
    host().png_host_filtered(np.ascontiguousarray(img).ctypes.data, w, h, depth, out.ctypes.data)
    return out.tobytes()


def host_file(img, level, icc=None, dpi=0):
    """the host build's file"""
    lib = host()
    h, w = img.shape[:2]
    img = np.ascontiguousarray(img)
    n = lib.png_host_encode(img.ctypes.data, w, h, 8 * img.itemsize, level, icc, len(icc) if icc else 0, dpi or 0)
    assert n > 0, "host build: counted and written bits disagree"
    out = np.empty(n, np.uint8)
    lib.png_host_copy(out.ctypes.data)
    return out.tobytes()
