"""not gpu: the PNG encoder's pieces that run without a device (tests/png_ref.py holds the checkers).

  * the numpy restatement of libpng's filter choice equals the filtered stream inflated from libpng's own file, and
    the host build of ansel_amd/csrc/png_deflate.h gives the same stream: sizes 1x1 .. 1001x777, five contents, 8 and
    16 bits
  * the host build's zlib stream inflates (zlib) to that stream at levels 0 / 1 / 5 / 9; its file opens in libpng with
    identical pixels at both depths and in Pillow at 8 bits; every chunk CRC is valid; iCCP and pHYs read back
  * dt_hip_png_bound() is at least the stored-only file for uniform noise, and refuses what the encoder refuses
  * abi.PngData matches the library's struct; params.png(); pipe.with_png()
  * the designed corpus png_ref.edge_frames(): each frame's file inflates (zlib) to the filtered stream, has valid chunk
    CRCs and IDAT chunks of 65 536 bytes, decodes in libpng, and the host build's stats (png_host_stats()) show that it
    reached the branches it was built for -- both length limits of jh_build() (15 literal / length, 7 code length),
    HCLEN 14 / 15 / 17 / 19, pd_rle()'s run edges, dynamic blocks without a match and with one distance code, distances 1
    and 32 768, length 257, a 3-byte match at 4 096 taken and at 4 097 refused, last segments of 1 and 2 bytes, N a
    multiple of the segment, 1 x 20 000 and 21 845 x 1, a 16-bit row of two segments, the all-0xFF stream, stored blocks
    at all eight bit phases, the IDAT split at zlen 65 536 / 65 537 / 65 540 / 65 541 / 131 072 and last chunks of 255 /
    256 / 257 bytes, png_scan's groups of 2 and 3 segments a thread; a closing test holds the union against
    png_ref.FEATURES, and png_ref.UNREACHED names what no frame reaches (a fixed block in the middle, the distance
    alphabet's limit)
  * pd_rle() alone against an RFC 1951 3.2.7 reader; pd_tables() alone on histograms no frame produces: Kraft sum 1,
    optimal cost within the limit, the block's bits recomputed, all three limits engaged"""
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


# ---------------------------------------------------------------------------------------------------------------------
# the designed corpus (png_ref.edge_frames()): every branch of the encoder reached from a frame, and the stats prove it

EDGES = pr.edge_frames()


@pytest.mark.parametrize("name,levels,feats", EDGES, ids=[e[0] for e in EDGES])
def test_edge_frame_inflates_and_reaches_its_branches(name, levels, feats):
    img = pr.edge_frame(name)
    h, w = img.shape[:2]
    depth = 8 * img.itemsize
    got = set()
    for level in levels:
        f, st, stream = pr.edge_host(name, level)  # host_file() asserts that the counted and written bits agree
        cs = pr.chunks(f)
        assert cs[0][0] == "IHDR" and cs[-1][0] == "IEND" and all(ok for _, _, ok in cs), level
        idat = [p for t, p, _ in cs if t == "IDAT"]
        assert len(idat) == st["nidat"] and len(idat[-1]) == st["last_idat"] and sum(map(len, idat)) == st["zlen"]
        assert all(len(p) == 65536 for p in idat[:-1])
        assert zlib.decompress(b"".join(idat)) == stream, level
        if w * h < 40000:
            assert stream == pr.filtered(img)
        if pr.ref() is not None:
            rgb, _, _ = pr.libpng_read(f, w, h, depth)
            assert np.array_equal(rgb, img[..., :3]), level
        got |= pr.features(img, level, st)
    assert feats <= got, sorted(feats - got)


def test_scan_frames_put_every_pair_of_block_kinds_into_one_thread():
    """png_scan gives each of its 256 threads ceil(nseg / 256) consecutive segments and composes their offset maps:
    inside one thread's group stored follows stored, stored follows dynamic, dynamic follows stored and dynamic follows
    dynamic, and behind a group's border a stored block starts at a bit phase other than 0"""
    for name, nseg in (("scan_257", 257), ("scan_513", 513)):
        _, st, _ = pr.edge_host(name, 5)
        bl = st["blocks"]
        assert len(bl) == nseg
        per = (nseg + 255) // 256
        assert per == (2 if nseg == 257 else 3)
        groups = pr.scan_groups([b["type"] == 0 for b in bl])
        assert len(groups) <= 256 and all(len(g) == per for g in groups[:-1])
        pairs = {(a, b) for g in groups for a, b in zip(g, g[1:])}
        assert pairs == {(False, False), (False, True), (True, False), (True, True)}
        assert any(bl[k]["type"] == 0 and bl[k]["phase"] != 0 for k in range(per, nseg, per))


def test_corpus_reaches_every_branch():
    """the union over the corpus holds every branch of png_ref.FEATURES; what no frame reaches is named in
    png_ref.UNREACHED with its reason and is reached through the table builder alone (the tests below)"""
    got = set()
    for name, levels, _ in EDGES:
        for level in levels:
            got |= pr.features(pr.edge_frame(name), level, pr.edge_host(name, level)[1])
    if len([k for k in range(4, 16) if "hclen_%d" % k in got]) >= 2:
        got.add("hclen_below_16_twice")
    assert not [f for f in pr.FEATURES if f not in got]
    assert not (set(pr.UNREACHED) & got), "a frame reaches it now: move it to FEATURES"
    assert set(pr.UNREACHED) == {"fixed_middle", "dist_limit"}


def test_rle_edges_alone():
    """pd_rle() on code lengths built for its edges, decoded by RFC 1951 3.2.7's rules: zero runs of 1 .. 300 and
    repeats of 1 .. 20, each alone, across the literal / distance border and at the sequence's end"""
    for r in list(range(1, 160)) + [275, 276, 277, 286, 300]:
        for v in (0, 5):
            for at in (0, 286 - r, 286 - r // 2, 316 - r):
                if at < 0 or at + r > 316:
                    continue
                lens = np.full(316, 9, np.uint8)
                lens[at:at + r] = v
                if at > 0:
                    lens[at - 1] = 7
                pairs = pr.host_rle(lens, 286, 30)
                assert pr.rle_decode(pairs) == list(lens), (r, v, at)
                if v == 0 and at == 0:
                    n18, rest = (r // 138, r % 138) if r >= 11 else (0, r)
                    want = [18] * n18 + ([18] if rest >= 11 else [17] if rest >= 3 else [0] * rest)
                    assert [s for s, _ in pairs][:len(want)] == want, (r, pairs[:4])
                if v == 5 and at == 0:
                    n16 = (r - 1) // 6 + (1 if (r - 1) % 6 >= 3 else 0)
                    assert [s for s, _ in pairs[:r]].count(16) >= n16


# ---------------------------------------------------------------------------------------------------------------------
# the table builder alone, on histograms no frame produces

def test_table_builder_on_designed_histograms():
    """pd_tables() with one lane (png_host_tables()) on png_ref.table_histograms(): the tie-free skewed series on each
    alphabet and both, the same at 32768 tokens, equal counts, one and two symbols, the end of block alone, Fibonacci
    counts and 200 random geometric ones.  png_ref.check_tables() holds for each: every counted symbol has a code within
    the limit, the Kraft sum is exactly 1, the cost is at least a heap-built Huffman code's and equal to it wherever the
    unadjusted code fits the limit, and the block's bits are the recomputed ones and the smallest of the three kinds.
    All three limits (15 / 15 / 7) engage, the distance alphabet's among them, which no frame reaches.

    How far the Annex K.3 code lands above the unlimited optimum (cost / optimal, literal, distance, code length
    alphabet; the longest unadjusted lengths in brackets):
      skew_lit_17 [17 1 5] 1.0002 1 1; skew_dist_17 [3 16 6] 1 1.0001 1; skew_both_17 [17 16 5] 1.0002 1.0001 1;
      skew_lit_18 [18 1 5] 1.0004 1 1; skew_dist_18 [3 17 5] 1 1.0002 1; skew_lit_21 [21 1 6] 1.0007 1 1;
      skew_dist_21 [3 20 6] 1 1.0005 1; skew_lit_32768 [18 1 5] 1.0004 1 1; fibonacci_both_24 [16 23 6] 1 1.0012 1;
      the largest over all histograms: 1.0175.
    zlib (Z_HUFFMAN_ONLY, one block, its own length limiting) on the literal streams: skew_lit_17 22 006 bits here,
    22 008 (rounded up to bytes) there, 66 744 stored; skew_lit_18 35 536 here and there, 108 080 stored."""
    names, freq = pr.table_histograms()
    segs, longest = pr.host_tables(freq)
    engaged = [0, 0, 0]
    kinds = set()
    worst = 1.0
    for n, f, s, lg in zip(names, freq, segs, longest):
        kinds.add(s.type)
        assert s.nbytes == pr.SEG
        r = pr.check_tables(f, s, lg)
        if r is None:
            continue
        for a, limit in enumerate((15, 15, 7)):
            engaged[a] += lg[a] > limit
        worst = max([worst] + r[0])
        if s.type == 2 and n in ("skew_lit_17", "skew_lit_18"):
            rng = np.random.default_rng(1)
            data = np.repeat(np.arange(256), f[:256]).astype(np.uint8)
            rng.shuffle(data)
            co = zlib.compressobj(9, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
            z = co.compress(data.tobytes()) + co.flush()
            assert zlib.decompress(z) == data.tobytes()
            print("%s: %d bits, zlib's Huffman-only block %d bits (byte-rounded), stored %d" %
                  (n, r[1], 8 * (len(z) - 6), 8 * len(data)))
            assert r[1] < 8 * len(data)
    print("K.3 cost / optimal, the largest: %.4f; limits engaged lit %d dist %d cl %d" % ((worst,) + tuple(engaged)))
    assert all(engaged), engaged
    assert kinds == {0, 1, 2}
    by = dict(zip(names, segs))
    assert by["eob_only"].type == 1  # ten bits: the smallest block is a fixed one
    for n in pr.LARGE_FEW_SYMBOLS:  # the dynamic block wins: check_tables() saw the lengths pd_lengths() raised
        assert by[n].type == 2, n
    assert by["equal"].type == 0  # 31 600 tokens of 8 bits and more in a segment of 32 768 bytes


def test_table_builder_level_0_is_stored():
    names, freq = pr.table_histograms()
    segs, _ = pr.host_tables(freq[:3], level=0)
    assert all(pr.seg_fields(s) == (0, pr.SEG, 0, 0, 0, 0, bytes(316), bytes(19)) for s in segs)
