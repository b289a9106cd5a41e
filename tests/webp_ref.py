"""The WebP encoder's checkers (tests/test_webp_host.py, tests/test_gpu_webp.py, tests/test_gpu_webp_pipe.py).

  * host() / host_file() / host_stats(): the encoder's body compiled for the host (tests/native/webp_host.cpp over
    ansel_amd/csrc/webp_body.h); host_stats() is what the last encode did, the tests' proof that a frame reached a branch
  * decode() / check_layout(): the judge is libwebp's decoder as Pillow ships it; check_layout() walks the RIFF chunks
  * predict() / synth(): a Python restatement of the 14 predictors and of SUBTRACT_GREEN, run BACKWARDS: a frame built
    from chosen residuals and chosen modes, so that a frame's symbol counts and its blocks' modes are what a test wants
  * CASES / case() / case_file(): the corpus, one table for the CPU and the GPU suite; every entry is (name, builder,
    predictor_bits, entropy_bits); FEATURES / UNREACHED: the branches the corpus must reach, and the ones no frame can

Frames are (h, w, 4) uint8 arrays, RGBA; alpha is ignored by the encoder."""
import ctypes as C
import io
import json
import os
import struct
import subprocess
import tempfile

import numpy as np

from ansel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")

WIN = 8192     # WP_WIN
MAXLEN = 4096  # WP_MAXLEN
LEVELS = (0, 1, 6)

_cache = {}


def _build_dir():
    if "dir" not in _cache:
        _cache["dir"] = tempfile.mkdtemp(prefix="webp_ref_")
    return _cache["dir"]


def host():
    """the encoder's body compiled for the host"""
    if "host" not in _cache:
        so = os.path.join(_build_dir(), "libwebp_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-I" + os.path.join(ROOT, "ansel_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                               os.path.join(NATIVE, "webp_host.cpp"), "-o", so])
        lib = C.CDLL(so)
        P = C.POINTER(abi.WebpData)
        lib.webp_host_encode.restype = C.c_size_t
        lib.webp_host_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, P]
        lib.webp_host_copy.argtypes = [C.c_void_p]
        lib.webp_host_bound.restype = C.c_size_t
        lib.webp_host_bound.argtypes = [C.c_int, C.c_int, P]
        lib.webp_host_stats.restype = C.c_size_t
        lib.webp_host_stats.argtypes = [C.c_void_p]
        lib.webp_host_rle.restype = C.c_size_t
        lib.webp_host_rle.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _cache["host"] = lib
    return _cache["host"]


def data(level=6, predictor_bits=0, entropy_bits=0, icc=None, lossless=1):
    d = abi.WebpData(lossless=lossless, level=level, predictor_bits=predictor_bits, entropy_bits=entropy_bits)
    if icc:
        d._icc = C.create_string_buffer(bytes(icc), len(icc))
        d.icc = C.cast(d._icc, C.c_void_p)
        d.icc_bytes = len(icc)
    return d


def host_file(img, d):
    h, w = img.shape[:2]
    img = np.ascontiguousarray(img)
    n = host().webp_host_encode(img.ctypes.data, w, h, C.byref(d))
    assert n > 0, "the host build refused the frame or disagrees with itself"
    out = np.empty(n, np.uint8)
    host().webp_host_copy(out.ctypes.data)
    return out.tobytes()


def host_stats():
    """what the last host_file() did (webp_host_stats())"""
    s = C.create_string_buffer(host().webp_host_stats(None))
    host().webp_host_stats(s)
    return json.loads(s.raw.decode())


def host_rle(lens):
    """wp_rle() on a list of code lengths: [(symbol, extra), ...]"""
    a = np.asarray(lens, np.uint8)
    out = np.zeros(2 * len(a) + 2, np.uint32)
    k = host().webp_host_rle(a.ctypes.data, len(a), out.ctypes.data)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(k)]


def decode(f):
    """libwebp's decoder: (mode, (h, w, 3) pixels, info)"""
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    im.load()
    return im.mode, np.asarray(im), im.info


def check_layout(f, w, h, icc=None):
    """RIFF size, chunk order, chunk sizes, even lengths, the VP8L signature and dimensions"""
    assert f[:4] == b"RIFF" and f[8:12] == b"WEBP" and len(f) % 2 == 0
    assert struct.unpack("<I", f[4:8])[0] == len(f) - 8
    at, order = 12, []
    while at + 8 <= len(f):
        name, n = f[at:at + 4], struct.unpack("<I", f[at + 4:at + 8])[0]
        order.append(name)
        body = f[at + 8:at + 8 + n]
        assert len(body) == n, "chunk %r runs past the file" % name
        if name == b"VP8X":
            assert n == 10 and body[0] == 0x20 and body[1:4] == b"\0\0\0"
            assert int.from_bytes(body[4:7], "little") == w - 1 and int.from_bytes(body[7:10], "little") == h - 1
        if name == b"ICCP":
            assert body == icc
        if name == b"VP8L":
            bits = struct.unpack("<I", body[1:5])[0]
            assert body[0] == 0x2f and (bits & 0x3fff) == w - 1 and ((bits >> 14) & 0x3fff) == h - 1 and bits >> 28 == 0
        if n & 1:
            assert f[at + 8 + n] == 0, "the padding byte is not zero"
        at += 8 + n + (n & 1)
    assert at == len(f)
    assert order == ([b"VP8X", b"ICCP", b"VP8L"] if icc else [b"VP8L"]), order


# ----------------------------------------------------------------------------------------------------------------------
# the format, restated

def _avg(a, b):
    return tuple((x + y) >> 1 for x, y in zip(a, b))


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def predict(mode, L, T, TL, TR):
    """the prediction of mode 0..13; pixels are (a, r, g, b) tuples"""
    if mode == 0:
        return (255, 0, 0, 0)
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:
        p = tuple(l + t - tl for l, t, tl in zip(L, T, TL))
        pl = sum(abs(a - b) for a, b in zip(p, L))
        pt = sum(abs(a - b) for a, b in zip(p, T))
        return L if pl < pt else T
    if mode == 12:
        return tuple(_clip(l + t - tl) for l, t, tl in zip(L, T, TL))
    a = _avg(L, T)
    return tuple(_clip(x + int((x - tl) / 2)) for x, tl in zip(a, TL))


def synth(w, h, residual, mode_of_block, predictor_bits):
    """the frame whose residual under the modes mode_of_block(bx, by) is residual(x, y) -> (r, g, b) (alpha's is 0):
    the decoder's inverse transforms, predictor then add-green"""
    px = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            if y == 0:
                pred = (255, 0, 0, 0) if x == 0 else px[0][x - 1]
            elif x == 0:
                pred = px[y - 1][0]
            else:
                TR = px[y - 1][x + 1] if x + 1 < w else px[y][0]
                pred = predict(mode_of_block(x >> predictor_bits, y >> predictor_bits), px[y][x - 1], px[y - 1][x],
                               px[y - 1][x - 1], TR)
            r = residual(x, y)
            px[y][x] = (pred[0], (pred[1] + r[0]) & 255, (pred[2] + r[1]) & 255, (pred[3] + r[2]) & 255)
    img = np.zeros((h, w, 4), np.uint8)
    for y in range(h):
        for x in range(w):
            _, r, g, b = px[y][x]
            img[y, x] = ((r + g) & 255, g, (b + g) & 255, (x * 7 + y) & 255)
    return img


# ----------------------------------------------------------------------------------------------------------------------
# the corpus

def frame(kind, w, h, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "const":
        img = np.empty((h, w, 4), np.uint8)
        img[:] = (200, 77, 13, 5)
    elif kind == "black":  # the top-left pixel's prediction itself: every residual is zero
        img = np.zeros((h, w, 4), np.uint8)
    elif kind == "two":
        img = np.where(((x // 3 + y // 2) % 2)[..., None] == 0, np.uint8(40), np.uint8(210)) * np.ones((1, 1, 4), np.uint8)
    elif kind == "noise":
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    elif kind == "hramp":
        img = np.stack([x * 3, x, 255 - x, 0 * x], -1).astype(np.uint8)
    elif kind == "vramp":
        img = np.stack([y * 2, 255 - y * 5, y, 0 * x], -1).astype(np.uint8)
    elif kind == "rows":  # one row of small residuals under mode 2 (top), the same in every row: matches at distance = width
        row = rng.integers(-3, 4, (w, 3))
        img = synth(w, h, lambda x, y: tuple(int(v) for v in row[x]), lambda bx, by: 2, 5)
    elif kind == "photo":  # smooth shading plus noise of sigma 2
        base = np.stack([128 + 90 * np.sin(x / 97.0 + y / 181.0), 120 + 80 * np.cos(y / 71.0) * np.sin(x / 233.0),
                         100 + 60 * np.sin((x + 2 * y) / 140.0), 0 * x], -1)
        img = np.clip(np.rint(base + rng.normal(0, 2, base.shape)), 0, 255).astype(np.uint8)
    else:  # "mix": smooth, flat and noisy parts
        img = np.stack([(x * 5 + y) % 256, (x // 4) * 9 % 256, (y * 3) % 256, 0 * x], -1).astype(np.uint8)
        img[h // 2:, : w // 2] = (9, 200, 100, 0)
        noisy = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        img[: h // 3, w // 2:] = noisy[: h // 3, w // 2:]
    return np.ascontiguousarray(img)


def _stripes():
    """14 stripes of 8 rows, each built so that its blocks' residual under ONE mode is sparse"""
    rng = np.random.default_rng(14)
    w, h = 40, 14 * 8
    imp = rng.integers(-20, 21, (h, w, 3)) * (rng.random((h, w, 1)) < 0.3)
    return synth(w, h, lambda x, y: tuple(int(v) for v in imp[y, x]), lambda bx, by: by, 3)


def _far(dist):
    """one row of noise in which 12 pixels repeat `dist` pixels later: a row's residual is the difference from the pixel
    to the left, so the residuals of 11 of them repeat"""
    img = frame("noise", 16383, 1, seed=dist)
    img[0, 9000:9012] = img[0, 9000 - dist:9012 - dist]
    return img


def _fibonacci():
    """one block, one tile: green residuals under mode 1 (left) with Fibonacci counts, 19 symbols -- a code of 18 bits
    before the limit.  The more frequent a residual, the smaller it is, so that mode 1 is the cheapest"""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    value = lambda rank: (rank + 1) // 2 * (1 if rank % 2 else -1)  # 0, 1, -1, 2, -2, ...
    seq = np.concatenate([np.full(f, value(18 - i), np.int64) for i, f in enumerate(fib)])
    rng = np.random.default_rng(19)
    rng.shuffle(seq)
    w, h = 105, 105  # 11025 >= 10945
    seq = np.concatenate([seq, np.zeros(w * h - len(seq), np.int64)])
    return synth(w, h, lambda x, y: (0, int(seq[y * w + x]), 0), lambda bx, by: 1, 9)


def _lengths():
    """one row (predicted from the left whatever the mode), 16 tiles of 512 pixels, literals: in every tile the green
    residuals are uniform over 0..255 (256 codes of 8 bits: the header starts with a repeat of the initial 8) and the red
    residuals uniform over 32 symbols whose gaps and runs sit on the edges of the repeat codes: runs of used symbols 4
    (1 + 3), 7 (1 + 6), 8, 13, gaps of 3, 10, 11, 138 unused ones"""
    runs = [(4, 3), (7, 10), (8, 11), (13, 138)]
    used, at = [], 0
    for r, gap in runs:
        used += list(range(at, at + r))
        at += r + gap
    assert len(used) == 32 and at <= 256
    rng = np.random.default_rng(8)
    g = np.concatenate([rng.permutation(np.repeat(np.arange(256), 2)) for _ in range(16)])
    r = np.concatenate([rng.permutation(np.repeat(np.array(used), 16)) for _ in range(16)])
    return synth(8192, 1, lambda x, y: (int(r[x]), int(g[x]), 0), lambda bx, by: 1, 9)


def _deep_header():
    """one block, one tile, literals: red residuals under mode 1 (left) on 86 symbols whose counts are powers of two, so
    that their code lengths are 6, 7, 10, 13, 5, 9, 3, 8 with 34, 21, 13, 8, 5, 3, 1, 1 symbols each (Kraft sum 1), no two
    equal lengths next to each other; with the two runs of zeros behind them (18 twice) the header's code length symbols
    have the counts 1 1 2 3 5 8 13 21 34, and its code length code is 8 bits deep before the limit of 7"""
    n_of = {6: 34, 7: 21, 10: 13, 13: 8, 5: 5, 9: 3, 3: 1, 8: 1}
    assert sum(n * 2 ** (13 - l) for l, n in n_of.items()) == 8192
    left, order, prev = dict(n_of), [], None
    while any(left.values()):
        l = max((k for k in left if left[k] and k != prev), key=lambda k: left[k])
        order.append(l)
        left[l] -= 1
        prev = l
    # symbols 0 .. 42 and 213 .. 255 (residuals -43 .. 42, centred so that mode 1 is the cheapest), 170 unused between
    seq = np.concatenate([np.full(2 ** (13 - l), i if i < 43 else i + 170, np.int64) for i, l in enumerate(order)])
    np.random.default_rng(7).shuffle(seq)
    return synth(128, 64, lambda x, y: (int(seq[y * 128 + x]), 0, 0), lambda bx, by: 1, 9)


# (name, builder, predictor_bits, entropy_bits)
CASES = [
    ("1x1", lambda: frame("mix", 1, 1), 0, 0),
    ("1x7", lambda: frame("mix", 1, 7), 0, 0),
    ("7x1", lambda: frame("mix", 7, 1), 0, 0),
    ("2x2", lambda: frame("mix", 2, 2), 0, 0),
    # 2^b - 1, 2^b, 2^b + 1 for the predictor block and the entropy tile
    ("3x5_b2", lambda: frame("mix", 3, 5, 1), 2, 2),
    ("4x4_b2", lambda: frame("mix", 4, 4, 2), 2, 2),
    ("5x3_b2", lambda: frame("mix", 5, 3, 3), 2, 2),
    ("7x9_b3", lambda: frame("mix", 7, 9, 4), 3, 3),
    ("8x8_b3", lambda: frame("noise", 8, 8, 5), 3, 3),
    ("9x7_b3", lambda: frame("mix", 9, 7, 6), 3, 3),
    ("3x3_tiles_ragged", lambda: frame("mix", 19, 21, 7), 2, 3),
    ("two_segments", lambda: frame("mix", 128, 128, 8), 0, 0),            # 16384 pixels
    ("two_segments_plus_1", lambda: frame("mix", 145, 113, 9), 0, 0),     # 16385 pixels
    ("16383x1", lambda: frame("mix", 16383, 1, 10), 0, 0),
    ("1x16383", lambda: frame("mix", 1, 16383, 11), 0, 0),
    ("black", lambda: frame("black", 33, 17), 0, 0),                      # every code has one symbol
    ("const", lambda: frame("const", 33, 17), 0, 0),                      # the first pixel and zeros: two symbols
    ("two_colours", lambda: frame("two", 33, 17), 0, 0),
    ("hramp", lambda: frame("hramp", 256, 9), 0, 0),
    ("vramp", lambda: frame("vramp", 9, 51), 0, 0),
    ("stripes", _stripes, 3, 0),
    ("noise", lambda: frame("noise", 67, 45, 12), 0, 0),
    ("rows", lambda: frame("rows", 61, 33, 13), 0, 0),
    ("long_run", lambda: frame("const", 128, 80), 0, 0),                  # 10240 equal residuals: lengths split at 4096
    ("far_%d" % WIN, lambda: _far(WIN), 0, 9),
    ("far_%d" % (WIN + 1), lambda: _far(WIN + 1), 0, 9),
    ("fibonacci", _fibonacci, 9, 9),
    ("lengths", _lengths, 9, 9),
    ("deep_header", _deep_header, 9, 9),
]
NOISE_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (4, 4), (5, 3), (7, 9), (8, 8), (9, 7), (19, 21), (128, 128), (145, 113),
               (16383, 1), (1, 16383)]


def case(name):
    """(frame, predictor_bits, entropy_bits), built once"""
    if ("case", name) not in _cache:
        for n, build, pb, eb in CASES:
            if n == name:
                _cache["case", name] = (build(), pb, eb)
    return _cache["case", name]


def case_file(name, level):
    """(the host build's file, its stats), built once"""
    if ("file", name, level) not in _cache:
        img, pb, eb = case(name)
        f = host_file(img, data(level, pb, eb))
        _cache["file", name, level] = (f, host_stats())
    return _cache["file", name, level]


def features(st):
    """the branches one encode reached, from its stats"""
    out = {"mode_%d" % m for m in range(14) if st["modes"][m]}
    out |= {k for k, n in zip(("simple1", "simple2", "normal", "normal1"), st["kinds"]) if n}
    out |= {"rle_%d" % s for s in (16, 17, 18) if st["rle"][s]}
    for key, name in (("rep_first", "repeat_of_initial_8"), ("matches", "match"), ("dist_one", "dist_left"),
                      ("dist_row", "dist_above"), ("dist_other", "dist_hashed"), ("lazy", "lazy_step"),
                      ("two_near", "match_of_2")):
        if st[key]:
            out.add(name)
    if max(st["longest"]) > 15:
        out.add("limit_15")
    if max(st["cl_longest"]) > 7:
        out.add("code_length_code_limit_7")
    if st["len_max"] == MAXLEN:
        out.add("length_split")
    if st["dist_max"] == WIN:
        out.add("farthest")
    if st["tiles"] > 1:
        out.add("entropy_image")
    if st["nseg"] > 1:
        out.add("segments")
    return out


FEATURES = sorted({"mode_%d" % m for m in range(14)} | {
    "simple1", "simple2", "normal", "normal1", "rle_16", "rle_17", "rle_18", "repeat_of_initial_8", "match", "dist_left",
    "dist_above", "dist_hashed", "lazy_step", "match_of_2", "limit_15", "code_length_code_limit_7", "length_split",
    "farthest", "entropy_image", "segments"})
# what no frame reaches: nothing is known to be out of reach (the code length code's limit of 7 bits, once listed here,
# is reached by "deep_header"); a branch that turns out to be unreachable is named here with the reason
UNREACHED = []
