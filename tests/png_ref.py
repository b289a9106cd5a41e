"""The PNG encoder's checkers (tests/test_png_host.py, tests/test_gpu_png.py, tests/test_gpu_png_pipe.py).

  * ref():    libpng 1.6 with Ansel's settings (tests/native/png_ref.c, compiled here against the libpng found on
              the machine; None if there is none): the reference file, and a reader for the encoder's files
  * host():   the encoder's body compiled for the host (tests/native/png_host.cpp over ansel_amd/csrc/png_deflate.h)
  * filtered(): a numpy restatement of libpng's filter choice (png_write_find_filter)
  * chunks() / idat_stream() / unfilter(): the file taken apart
  * host_stats() / features(): what an encode of the host build did, as the names of the encoder's branches (FEATURES)
  * edge_frames() / edge_frame() / edge_host(): the corpus designed to reach every branch from a frame, each entry with
    its levels and the branches it must reach; UNREACHED: the branches no frame reaches, and why
  * table_histograms() / host_tables() / check_tables(): the table builder alone on histograms no frame produces, and
    what must hold for a record whoever built it (Kraft sum, optimal cost, the block's bits)"""
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


# ---------------------------------------------------------------------------------------------------------------------
# the encoder's branches: what an encode did (png_host_stats()), and frames designed to reach each branch

def host_stats():
    """what the last host_file() did: png_host_stats()'s JSON as a dict (tests/native/png_host.cpp)"""
    import json
    lib = host()
    lib.png_host_stats.restype = C.c_size_t
    lib.png_host_stats.argtypes = [C.c_void_p]
    buf = C.create_string_buffer(lib.png_host_stats(None))
    lib.png_host_stats(buf)
    return json.loads(buf.raw.decode())


def host_file_stats(img, level):
    f = host_file(img, level)
    return f, host_stats()


def host_rle(lens, nlit, ndist):
    """pd_rle() on 316 code lengths: [(symbol, extra)]"""
    lib = host()
    lib.png_host_rle.restype = C.c_size_t
    lib.png_host_rle.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lens = np.ascontiguousarray(lens, np.uint8)
    out = np.zeros(2 * 316, np.uint32)
    n = lib.png_host_rle(lens.ctypes.data, nlit, ndist, out.ctypes.data)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def rle_decode(pairs):
    """RFC 1951 section 3.2.7: the code length sequence that (symbol, extra) pairs of the code length alphabet stand for"""
    out = []
    for sym, extra in pairs:
        if sym < 16:
            assert extra == 0
            out.append(sym)
        elif sym == 16:
            assert out and 0 <= extra <= 3
            out += [out[-1]] * (3 + extra)
        elif sym == 17:
            assert 0 <= extra <= 7
            out += [0] * (3 + extra)
        else:
            assert sym == 18 and 0 <= extra <= 127
            out += [0] * (11 + extra)
    return out


def runs(seq):
    """[(value, run length, start)] of a sequence"""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        out.append((seq[i], j - i, i))
        i = j
    return out


SEG = 32768
ZRUNS = (2, 3, 10, 11, 138, 139, 149)
REPS = (3, 4, 7, 8)
IDAT_ZLEN = (65536, 65537, 65540, 65541, 131072)
IDAT_LAST = (255, 256, 257)


def scan_groups(types):
    """png_scan's share of the segments: 256 threads, ceil(nseg / 256) consecutive segments each"""
    per = (len(types) + 255) // 256
    return [types[i:i + per] for i in range(0, len(types), per)]


def features(img, level, st):
    """the names of the branches that encoding img at level reached, from the host build's stats st"""
    f = set()
    h, w = img.shape[:2]
    depth = 8 * img.itemsize
    bl = st["blocks"]
    nseg = len(bl)
    N = st["N"]
    if w == 1 and h >= 20000:
        f.add("shape_1xH")
    if h == 1 and w >= 20000:
        f.add("shape_Wx1")
    if depth == 16 and w * 6 > 2 * SEG:
        f.add("row16_gt_2seg")
    if N % SEG == 0:
        f.add("N_multiple_of_seg")
    if N % SEG == 1 and nseg > 1:
        f.add("N_multiple_of_seg_plus_1")
    if level > 0 and nseg > 1 and bl[-1]["nbytes"] in (1, 2):
        f.add("last_seg_%d" % bl[-1]["nbytes"])
    if level == 0:
        assert st["zlen"] == 2 + 5 * nseg + N + 4
        if st["zlen"] in IDAT_ZLEN:
            f.add("zlen_%d" % st["zlen"])
        if st["nidat"] > 1 and st["last_idat"] in IDAT_LAST:
            f.add("last_idat_%d" % st["last_idat"])
    types = [b["type"] for b in bl]
    for k, b in enumerate(bl):
        full = b["nbytes"] == SEG
        if level > 0 and b["type"] == 0 and k > 0 and bl[k - 1]["type"] != 0:
            f.add("stored_phase_%d" % b["phase"])
        if b["type"] == 1 and 0 < k < nseg - 1:
            f.add("fixed_middle")
        if b["type"] != 0 and b["matches"]:
            if b["dist_min"] == 1:
                f.add("dist_1")
            if b["dist_max"] == 32768:
                f.add("dist_32768")
            if b["len_max"] == 257:
                f.add("len_257")
            if b["far3_taken"] == 4096:
                f.add("far3_4096_taken")
        if b["type"] != 0 and b["far3_refused"] == 4097:
            f.add("far3_4097_refused")
        if b["type"] != 2:
            continue
        if b["longest"][0] > 15:
            f.add("lit_limit")
        if b["longest"][1] > 15:
            f.add("dist_limit")
        if b["longest"][2] > 7:
            f.add("cl_limit")
        f.add("hclen_%d" % b["ncl"])
        if full and b["matches"] == 0:
            f.add("dyn_no_match_full_seg")
        if full and b["dist_used"] == 1:
            f.add("dyn_one_dist_full_seg")
        seq = b["len"][:b["nlit"]] + b["len"][286:286 + b["ndist"]]
        pairs = list(zip(b["rle"][0::2], b["rle"][1::2]))
        assert rle_decode(pairs) == seq, "pd_rle()'s symbols do not decode to the code lengths"
        for v, r, at in runs(seq):
            if v == 0 and r in ZRUNS:
                f.add("zrun_%d" % r)
            if v != 0 and r in REPS:
                f.add("rep_%d" % r)
            if at < b["nlit"] < at + r:
                f.add("rle_crosses_border")
    if level > 0 and nseg > 256:
        groups = scan_groups(types)
        pairs = set()
        for g in groups:
            for a, b in zip(g, g[1:]):
                pairs.add((a == 0, b == 0))
        per = (nseg + 255) // 256
        behind = any(bl[k]["type"] == 0 and bl[k]["phase"] != 0 for k in range(per, nseg, per))
        if len(pairs) == 4 and behind:
            f.add("scan_%d" % (257 if nseg < 513 else 513))
    if level in (0, 5) and nseg >= 4:
        s = np.frombuffer(host_filtered(img), np.uint8)
        if (s == 255).sum() >= 3 * SEG and (s == 255).sum() > 0.98 * N:
            f.add("adler_ff_level_%d" % level)
    return f


# every branch the corpus must reach from a frame
FEATURES = (["lit_limit", "cl_limit", "hclen_19", "hclen_17", "hclen_below_16_twice"]
            + ["zrun_%d" % r for r in ZRUNS] + ["rep_%d" % r for r in REPS] + ["rle_crosses_border"]
            + ["dyn_no_match_full_seg", "dyn_one_dist_full_seg"]
            + ["dist_1", "dist_32768", "len_257", "far3_4096_taken", "far3_4097_refused"]
            + ["last_seg_1", "last_seg_2", "N_multiple_of_seg", "N_multiple_of_seg_plus_1"]
            + ["shape_1xH", "shape_Wx1", "row16_gt_2seg", "adler_ff_level_0", "adler_ff_level_5"]
            + ["stored_phase_%d" % p for p in range(8)]
            + ["zlen_%d" % z for z in IDAT_ZLEN] + ["last_idat_%d" % n for n in IDAT_LAST]
            + ["scan_257", "scan_513"])

# branches no frame reaches, each with its reason; tests/test_png_tables.py reaches them through the table builder alone
UNREACHED = {
    "fixed_middle": "a block that is neither first nor last holds PD_SEG bytes, hence at least 128 tokens; a dynamic code "
                    "saves more on those than its header costs, so the fixed block is never the smaller one there",
    "dist_limit": "a code deeper than 15 bits needs 17 distance codes with Fibonacci-like counts, 4 180 matches at the "
                  "least in one segment; a step's 256 positions look the tables up before any of them enters, so a "
                  "distance below 256 is seen only across a step's border, a 3-byte match stops at 4 096, and a slot "
                  "keeps its last position only: of 4 180 planted matches on 17 codes the parse took about 300, and the "
                  "longest distance code of any frame tried was 12 bits unadjusted",
}

# bytes with a small |signed byte| (0, -1, 1, -2, ...: any prefix is symmetric): on a single row of them libpng's choice
# is filter None, so the row's bytes are the filtered stream's (behind the filter byte 0)
LOW = np.stack([np.arange(0, 64), 255 - np.arange(0, 64)], axis=1).reshape(-1).astype(np.uint8)
SKEW = (1, 1, 3, 5, 9, 15, 25, 41, 67, 109, 177)  # a[k] = a[k-1] + a[k-2] + 1: no ties, the deepest Huffman tree


def from_raw(raw, seed=0):
    """the RGBA u8 frame of raw rows (h, 3 w); alpha random"""
    raw = np.asarray(raw, np.uint8)
    h, rb = raw.shape
    img = np.empty((h, rb // 3, 4), np.uint8)
    img[..., :3] = raw.reshape(h, rb // 3, 3)
    img[..., 3] = np.random.default_rng(seed).integers(0, 256, (h, rb // 3))
    return img


def from_raw16(raw, seed=0):
    """the RGBA u16 frame of raw rows (h, 6 w) of big-endian samples; alpha random"""
    raw = np.asarray(raw, np.uint8)
    h, rb = raw.shape
    v = np.frombuffer(raw.tobytes(), ">u2").astype(np.uint16).reshape(h, rb // 6, 3)
    img = np.empty((h, rb // 6, 4), np.uint16)
    img[..., :3] = v
    img[..., 3] = np.random.default_rng(seed).integers(0, 65536, (h, rb // 6))
    return img


def one_row(stream):
    """the w x 1 frame whose filtered stream is `stream` (its first byte 0: filter None wins, or this asserts)"""
    stream = np.asarray(stream, np.uint8)
    assert stream[0] == 0 and (len(stream) - 1) % 3 == 0
    img = from_raw(stream[None, 1:])
    assert host_filtered(img) == stream.tobytes(), "one_row: libpng's choice is not filter None"
    return img


def no_repeat(n, values, rng, plant=None):
    """n bytes drawn from values in which no three consecutive bytes occur twice: a stream without a match -- but for
    plant = {position: distance}: the three bytes there repeat those `distance` back, and the fourth differs (where the
    bytes around a plant would repeat another triple, the plant is dropped)"""
    seen, out = set(), []
    values = [int(v) for v in values]
    plant = plant or {}

    def fresh(v):
        key = tuple(out[-2:] + [v])
        return len(key) < 3 or key not in seen

    def push(v):
        if len(out) >= 2:
            seen.add(tuple(out[-2:] + [v]))
        out.append(v)

    differ = None
    while len(out) < n:
        d = plant.get(len(out))
        if d and len(out) + 4 <= n:
            c = out[len(out) - d:len(out) - d + 4]
            if len(out) >= 2 and tuple(out[-2:] + c[:1]) not in seen and tuple(out[-1:] + c[:2]) not in seen:
                seen.add(tuple(out[-2:] + c[:1]))
                seen.add(tuple(out[-1:] + c[:2]))
                out += c[:3]
                differ = c[3]
                continue
        for _ in range(256):
            v = values[int(rng.integers(len(values)))]
            if fresh(v) and v != differ:
                break
        else:
            raise ValueError("no_repeat: stuck")
        differ = None
        push(v)
    return np.array(out, np.uint8)


def skewed_row(ncommon, seed, n=32766):
    """n bytes: SKEW's counts of eleven rare values among uniform draws from ncommon of LOW's values, shuffled"""
    rng = np.random.default_rng(seed)
    rare = np.concatenate([np.full(c, 64 + i, np.uint8) for i, c in enumerate(SKEW)])
    common = LOW[rng.integers(0, ncommon, n - len(rare))]
    raw = np.concatenate([rare, common])
    rng.shuffle(raw)
    return raw


def geometric_frame(w, h, nvalues, ratio, seed):
    """w x h, 8 bits: samples drawn from nvalues of LOW's values with probabilities ratio^k"""
    rng = np.random.default_rng(seed)
    p = ratio ** np.arange(nvalues)
    vals = LOW[rng.permutation(len(LOW))[:nvalues]]
    return from_raw(vals[rng.choice(nvalues, (h, 3 * w), p=p / p.sum())], seed)


def banded(w, h, depth, seed, lo=3, hi=40):
    """rows in bands of lo..hi rows: noise (stored blocks), zeros, a gradient, a few values (dynamic blocks)"""
    rng = np.random.default_rng(seed)
    top = 255 if depth == 8 else 65535
    img = np.zeros((h, w, 4), np.uint8 if depth == 8 else np.uint16)
    y, kind = 0, 0
    while y < h:
        n = int(rng.integers(lo, hi + 1))
        rows = img[y:y + n, :, :3]
        if kind % 2 == 0:
            rows[...] = rng.integers(0, top + 1, rows.shape)
        elif kind % 4 == 1:
            rows[...] = 0 if kind % 8 == 1 else (np.arange(w) * (top // max(w, 1)))[None, :, None]
        else:
            rows[...] = rng.integers(0, 3, rows.shape) * (top // 2)
        y += n
        kind += 1
    img[..., 3] = rng.integers(0, top + 1, (h, w))
    return img


def gap_row(gap, seed, n=3000):
    """one row whose bytes are 0 .. k and 255 - m .. 255 with `gap` unused values between: a zero run of `gap` code lengths"""
    k = (254 - gap) // 2
    m = 254 - gap - k
    v = np.concatenate([np.arange(0, k + 1), np.arange(255 - m, 256)]).astype(np.uint8)
    assert 255 - m - (k + 1) == gap
    rng = np.random.default_rng(seed)
    return one_row(np.concatenate([[0], v, v[rng.integers(0, len(v), n - len(v))]]))


def phase_frame(seed):
    """100 x 218, 8 bits: a first segment of skewed samples (a dynamic block whose length depends on the seed), then noise
    (stored blocks, the first one behind the dynamic block's last bit)"""
    img = geometric_frame(100, 218, 24, 0.8, seed)
    img[109:, :, :3] = np.random.default_rng(seed).integers(0, 256, (109, 100, 3))
    return img


def ff_frame(w=256, h=130):
    """x(i, y) = -(i + y) mod 256 in every channel: Sub, Up, Average and Paeth all give 0xFF, the largest Adler-32 sums"""
    i, y = np.arange(w)[None, :], np.arange(h)[:, None]
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = ((-(i + y)) % 256)[..., None]
    return img


# the seeds of phase_frame() whose first stored block starts at bit phase 0 .. 7 (found by search; the closing test of
# tests/test_png_host.py fails when the encoder's parse or tables change and they no longer do)
PHASE_SEEDS = (1, 0, 35, 7, 3, 5, 2, 23)


def _far_row():
    """65536 bytes whose second half repeats the first: matches at distance 32768 where a slot kept the far position"""
    s = np.zeros(2 * SEG, np.uint8)
    s[1:SEG] = LOW[np.random.default_rng(7).integers(0, 128, SEG - 1)]
    s[SEG:] = s[:SEG]
    return one_row(s)


def _planted_row(n, values, seed, plant=None):
    s = no_repeat(n, values, np.random.default_rng(seed), plant)
    s[0] = 0
    return one_row(s)


def _last1_row():
    s = np.zeros(3 * SEG + 1, np.uint8)
    s[1:] = LOW[np.random.default_rng(8).integers(0, 40, 3 * SEG)]
    return one_row(s)


def _edge_list():
    e = [
        ("lit_limit", lambda: one_row(np.concatenate([[0], skewed_row(128, 1)])), (1, 5), {"lit_limit", "hclen_19"}),
        ("skew_32_values", lambda: one_row(np.concatenate([[0], skewed_row(32, 1)])), (1,), {"hclen_17"}),
        ("cl_limit", lambda: geometric_frame(104, 26, 60, 0.93, 0), (1,), {"cl_limit"}),
        ("hclen_14", lambda: geometric_frame(146, 7, 19, 0.6, 0), (1,), {"hclen_14", "zrun_2", "zrun_3", "zrun_11",
                                                                        "rep_3"}),
        ("hclen_15", lambda: geometric_frame(104, 26, 19, 0.6, 3), (1,), {"hclen_15", "cl_limit"}),
        ("zrun_10", lambda: geometric_frame(146, 7, 37, 0.75, 0), (1,), {"zrun_10"}),
        ("rep_4", lambda: geometric_frame(146, 7, 60, 0.93, 0), (1,), {"rep_4"}),
        ("rep_7", lambda: geometric_frame(146, 7, 37, 0.93, 8), (1,), {"rep_7"}),
        ("rle_border", lambda: geometric_frame(60, 11, 19, 0.6, 9), (1,), {"rle_crosses_border"}),
        ("zrun_138", lambda: gap_row(138, 1), (1,), {"zrun_138"}),
        ("zrun_139", lambda: gap_row(139, 2), (1,), {"zrun_139"}),
        ("zrun_149", lambda: gap_row(149, 3), (1,), {"zrun_149"}),
        ("bands_n_multiple", lambda: banded(341, 96, 8, 3, 3, 12), (1,), {"N_multiple_of_seg", "rep_8"}),
        ("no_match", lambda: _planted_row(SEG + 2, LOW[:64], 4), (1, 5), {"dyn_no_match_full_seg", "last_seg_2"}),
        ("one_distance", lambda: _planted_row(SEG + 2, LOW[:64], 4, {p: 100 for p in range(500, 32000, 900)}), (1, 5), {"dyn_one_dist_full_seg"}),
        ("distance_32768", _far_row, (1, 5), {"dist_32768", "N_multiple_of_seg", "shape_Wx1"}),
        ("too_far", lambda: _planted_row(16384, LOW, 3, {p: 4096 + (i & 1) for i, p in enumerate(range(4200, 16000, 300))}), (1, 5), {"far3_4096_taken", "far3_4097_refused"}),
        ("last_segment_1", _last1_row, (1,), {"last_seg_1", "N_multiple_of_seg_plus_1"}),
        ("all_ff", ff_frame, (0, 5), {"adler_ff_level_0", "adler_ff_level_5", "dist_1", "len_257"}),
        ("shape_1x20000", lambda: banded(1, 20000, 8, 1, 50, 400), (5,), {"shape_1xH"}),
        ("row16_two_segments", lambda: banded(11000, 2, 16, 3, 1, 1), (5,), {"row16_gt_2seg"}),
    ]
    for p, seed in enumerate(PHASE_SEEDS):
        e.append(("stored_phase_%d" % p, (lambda s=seed: phase_frame(s)), (5,), {"stored_phase_%d" % p}))
    # level 0: zlen = 2 + 5 nseg + N + 4 exactly
    for feat, (w, h, d) in (("zlen_65536", (173, 126, 8)), ("zlen_65537", (10920, 1, 16)), ("zlen_65540", (2730, 4, 16)),
                            ("zlen_65541", (8, 2621, 8)), ("zlen_131072", (3640, 6, 16)),
                            ("last_idat_255", (1096, 10, 16)), ("last_idat_256", (123, 89, 16)),
                            ("last_idat_257", (135, 162, 8))):
        e.append((feat, (lambda w=w, h=h, d=d: frame("noise", w, h, d, seed=w)), (0,), {feat}))
    e.append(("scan_257", lambda: banded(836, 1673, 16, 1, 3, 40), (5,), {"scan_257"}))
    e.append(("scan_513", lambda: banded(1672, 1675, 16, 1, 3, 40), (5,), {"scan_513"}))
    return e


SCAN_FRAMES = ("scan_257", "scan_513")


def edge_frames():
    """[(name, levels, features)]: the designed corpus; edge_frame(name) builds a frame, edge_host(name, level) encodes it"""
    if "edges" not in _cache:
        _cache["edges"] = _edge_list()
    return [(n, lv, ft) for n, _, lv, ft in _cache["edges"]]


def edge_frame(name):
    edge_frames()
    fr = _cache.setdefault("edge_frame", {})
    if name not in fr:
        fr[name] = next(b for n, b, _, _ in _cache["edges"] if n == name)()
    return fr[name]


def edge_host(name, level):
    """(the host build's file, its stats, the filtered stream) of a corpus frame: computed once a process"""
    done = _cache.setdefault("edge_host", {})
    if (name, level) not in done:
        img = edge_frame(name)
        f, st = host_file_stats(img, level)
        done[name, level] = (f, st, host_filtered(img))
    return done[name, level]


# ---------------------------------------------------------------------------------------------------------------------
# the table builder alone (pd_tables(): png_host_tables() here, dt_hip_test_png_tables() on the device)

NLIT, NDIST, NCL = 286, 30, 19
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class Seg(C.Structure):
    """pd_seg_t of ansel_amd/csrc/png_deflate.h"""
    _fields_ = [("type", C.c_uint32), ("nbytes", C.c_uint32), ("bits", C.c_uint64), ("nlit", C.c_uint32),
                ("ndist", C.c_uint32), ("ncl", C.c_uint32), ("adler_s", C.c_uint32), ("adler_t", C.c_uint32),
                ("len", C.c_uint8 * (NLIT + NDIST)), ("cl_len", C.c_uint8 * NCL)]


def seg_fields(s):
    """a record's fields but the Adler sums"""
    return (s.type, s.nbytes, s.bits, s.nlit, s.ndist, s.ncl, bytes(s.len), bytes(s.cl_len))


def skew_series(n):
    """a[k] = a[k-1] + a[k-2] + 1 from 1, 1: n tie-free counts whose Huffman tree is n - 1 deep"""
    a = [1, 1]
    while len(a) < n:
        a.append(a[-1] + a[-2] + 1)
    return a[:n]


def fibonacci(n):
    a = [1, 1]
    while len(a) < n:
        a.append(a[-1] + a[-2])
    return a[:n]


def table_histograms():
    """(names, counts[n, 316]): histograms no frame produces.  Every one counts the end-of-block symbol, as every
    segment does, so the literal / length alphabet's "exactly one" is the end of block alone and its "exactly two" the
    end of block and one more symbol; each such shape comes with few counts (a fixed block wins and replaces the
    lengths in the record) and with thousands (the dynamic block wins, and its raised lengths are checked)"""
    names, rows = [], []

    def add(name, lit=None, dist=None):
        f = np.zeros(NLIT + NDIST, np.uint32)
        for k, v in (lit or {}).items():
            f[k] = v
        for k, v in (dist or {}).items():
            f[NLIT + k] = v
        f[256] = max(int(f[256]), 1)
        names.append(name)
        rows.append(f)

    rng = np.random.default_rng(11)
    lit_syms = [int(s) for s in rng.permutation(256)[:20]] + [284]
    dist_syms = [int(s) for s in rng.permutation(NDIST)]
    for n in (17, 18, 21):
        s = skew_series(n)
        add("skew_lit_%d" % n, lit=dict(zip(lit_syms, s)))
        add("skew_dist_%d" % n, lit={5: 40, 7: 30, 260: sum(s)}, dist=dict(zip(dist_syms, s)))
        add("skew_both_%d" % n, lit=dict(zip(lit_syms, s)), dist=dict(zip(dist_syms, s)))
    s = skew_series(18)
    k = 32768 // sum(s)
    big = [v * k for v in s]
    big[-1] += 32768 - 1 - sum(big)
    add("skew_lit_32768", lit=dict(zip(lit_syms, big)))
    add("skew_dist_32768", lit={5: 1, 260: 16383, 270: 16383}, dist=dict(zip(dist_syms, [v * k for v in s])))
    add("skew_both_32768", lit=dict(zip(lit_syms, big)), dist=dict(zip(dist_syms, [v * k for v in s])))
    add("equal", lit={i: 100 for i in range(NLIT)}, dist={i: 100 for i in range(NDIST)})
    add("equal_ones", lit={i: 1 for i in range(NLIT)}, dist={i: 1 for i in range(NDIST)})
    add("eob_and_one_length", lit={257: 9}, dist={0: 9})
    add("eob_and_one_length_5000", lit={285: 5000}, dist={29: 5000})
    add("eob_and_two", lit={0: 7, 285: 3}, dist={3: 2, 29: 8})
    add("eob_and_two_10000", lit={0: 7000, 285: 3000}, dist={3: 600, 29: 2400})
    add("eob_only")
    add("eob_only_5000", lit={256: 5000})
    add("one_each_5000", lit={256: 5000}, dist={29: 5000})
    add("one_each_5000_first_symbols", lit={256: 5000}, dist={0: 5000})
    add("eob_and_one_literal", lit={65: 1})
    add("two_each_10000", lit={0: 7000, 256: 3000}, dist={3: 2000, 29: 8000})
    add("two_each_10000_first_symbols", lit={0: 7000, 256: 3000}, dist={0: 2000, 1: 8000})
    for n in (16, 20, 24):
        add("fibonacci_lit_%d" % n, lit=dict(zip(lit_syms + [1, 2, 3], fibonacci(n))))
        add("fibonacci_both_%d" % n, lit=dict(zip(lit_syms + [1, 2, 3], fibonacci(n))),
            dist=dict(zip(dist_syms, fibonacci(n))))
    for i in range(200):
        nl, nd = int(rng.integers(1, NLIT + 1)), int(rng.integers(0, NDIST + 1))
        rl, rd = rng.uniform(0.3, 0.99), rng.uniform(0.3, 0.99)
        tot = int(rng.integers(10, 32768))
        pl = rl ** np.arange(nl)
        lit = dict(zip([int(v) for v in rng.permutation(NLIT)[:nl]], rng.multinomial(tot, pl / pl.sum())))
        dist = {}
        if nd:
            pdist = rd ** np.arange(nd)
            dist = dict(zip([int(v) for v in rng.permutation(NDIST)[:nd]],
                            rng.multinomial(tot // 3, pdist / pdist.sum())))
        add("random_%d" % i, lit=lit, dist=dist)
    return names, np.ascontiguousarray(np.stack(rows))


def host_tables(freq, level=5):
    """pd_tables() with one lane on each histogram: ([Seg], longest[n, 3])"""
    lib = host()
    lib.png_host_sizeof_seg.restype = C.c_size_t
    assert lib.png_host_sizeof_seg() == C.sizeof(Seg)
    lib.png_host_tables.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    n = len(freq)
    segs = (Seg * n)()
    longest = np.zeros((n, 3), np.int32)
    lib.png_host_tables(freq.ctypes.data, n * SEG, n, level, C.byref(segs), longest.ctypes.data)
    return list(segs), longest


def huffman_cost(counts):
    """the bits of a plain (unlimited) Huffman code for the non-zero counts: sum of the merged weights, by a heap"""
    import heapq
    h = [int(c) for c in counts if c]
    if len(h) == 1:
        return h[0]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


def lit_extra(s):
    return (s - 261) // 4 if 265 <= s < 285 else 0


def dist_extra(s):
    return s // 2 - 1 if s >= 4 else 0


def fixed_lit_len(s):
    return 8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8


def check_tables(freq, seg, longest):
    """what must hold for one record, whoever built it; returns (K.3 cost / optimal cost per alphabet, dynamic bits), or
    None for a fixed block: its record holds the fixed code's lengths in place of the dynamic ones, so its bits are
    recomputed and held against the stored block's, and the dynamic code it was weighed against is checked on the
    histograms of the same shapes with counts large enough for the dynamic block to win (table_histograms())"""
    freq = [int(v) for v in freq]
    lens = list(seg.len)
    fix = 3 + sum(freq[s] * (fixed_lit_len(s) + lit_extra(s)) for s in range(NLIT))
    fix += sum(freq[NLIT + s] * (5 + dist_extra(s)) for s in range(NDIST))
    sto = 3 + 7 + 32 + 8 * seg.nbytes
    if seg.type == 1:
        assert lens[:NLIT] == [fixed_lit_len(s) for s in range(NLIT)] and lens[NLIT:] == [5] * NDIST
        assert seg.bits == fix and fix <= sto
        assert 257 <= seg.nlit <= NLIT and 1 <= seg.ndist <= NDIST and 4 <= seg.ncl <= NCL
        return None
    lit, dist = lens[:NLIT], lens[NLIT:]
    assert seg.nlit == max(257, max(i + 1 for i in range(NLIT) if lit[i]))
    assert seg.ndist == max([1] + [i + 1 for i in range(NDIST) if dist[i]])
    pairs = host_rle(lens, seg.nlit, seg.ndist)
    assert rle_decode(pairs) == lit[:seg.nlit] + dist[:seg.ndist]
    clfreq = [sum(1 for s, _ in pairs if s == k) for k in range(NCL)]
    cl = list(seg.cl_len)
    assert seg.ncl == max([4] + [i + 1 for i in range(NCL) if cl[CL_ORDER[i]]])
    ratios = []
    for counts, ln, limit, lg in ((freq[:NLIT], lit, 15, longest[0]), (freq[NLIT:], dist, 15, longest[1]),
                                  (clfreq, cl, 7, longest[2])):
        assert all(1 <= l <= limit for c, l in zip(counts, ln) if c), "a counted symbol without a code"
        assert all(0 <= l <= limit for l in ln)
        assert sum(1 << (limit - l) for l in ln if l) == 1 << limit, "the Kraft sum is not 1"
        cost, best = sum(c * l for c, l in zip(counts, ln)), huffman_cost(counts)
        assert cost >= best
        if lg <= limit:
            assert cost == best, "within the limit and not optimal"
        ratios.append(cost / best if best else 1.0)
    dyn = 3 + 5 + 5 + 4 + 3 * seg.ncl + sum(clfreq[s] * (cl[s] + {16: 2, 17: 3, 18: 7}.get(s, 0)) for s in range(NCL))
    dyn += sum(freq[s] * (lit[s] + lit_extra(s)) for s in range(NLIT))
    dyn += sum(freq[NLIT + s] * (dist[s] + dist_extra(s)) for s in range(NDIST))
    if seg.type == 2:
        assert seg.bits == dyn and dyn <= fix and dyn <= sto and dyn < 8 * seg.nbytes
    else:
        assert seg.type == 0 and seg.bits == 0 and sto < dyn and sto < fix
    return ratios, dyn


# table_histograms() with one or two counted symbols an alphabet and counts large enough for a dynamic block
LARGE_FEW_SYMBOLS = ("eob_and_one_length_5000", "eob_and_two_10000", "eob_only_5000", "one_each_5000",
                     "one_each_5000_first_symbols", "two_each_10000", "two_each_10000_first_symbols")
