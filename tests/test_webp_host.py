"""The lossless WebP encoder's body on the host (tests/native/webp_host.cpp over ansel_amd/csrc/webp_body.h), judged by
libwebp's decoder as Pillow ships it -- not by our own code.

  * every corpus frame (webp_ref.CASES) at levels 0 / 1 / 6 decodes to mode RGB and to the input's RGB, every pixel; the
    RIFF and chunk sizes are consistent and even
  * ICC profiles of 1 byte, an odd length and 200 000 bytes come back through Pillow's info["icc_profile"]
  * the corpus reaches every branch named in webp_ref.FEATURES (all 14 predictor modes among them)
  * wp_rle() at the edges of the repeat codes, and the "previous length starts as 8" rule
  * the bound holds for noise at every corpus size; what the encoder refuses, the bound refuses
  * abi.WebpData, params.webp(), pipe.with_webp()
  * the size against libwebp on a photo-like frame
  * the host twin as a program of its own under -fsanitize=address,undefined"""
import ctypes as C
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest

import webp_ref as wr
from ansel_amd import abi, params, pipe

NAMES = [c[0] for c in wr.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_libwebp_decodes_the_file_to_the_input(name):
    img, pb, eb = wr.case(name)
    h, w = img.shape[:2]
    for level in wr.LEVELS:
        f, st = wr.case_file(name, level)
        wr.check_layout(f, w, h)
        mode, got, _ = wr.decode(f)
        assert mode == "RGB"
        assert got.shape == (h, w, 3) and (got == img[..., :3]).all(), (level, st)
        assert 8 + len(f) <= wr.host().webp_host_bound(w, h, C.byref(wr.data(level, pb, eb)))


@pytest.mark.parametrize("icc_bytes", [1, 477, 200000])
def test_icc_profile_comes_back(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    img = wr.frame("mix", 37, 13, 5)
    f = wr.host_file(img, wr.data(6, icc=icc))
    assert f[:4] == b"RIFF" and f[8:16] == b"WEBPVP8X"
    wr.check_layout(f, 37, 13, icc)
    mode, got, info = wr.decode(f)
    assert mode == "RGB" and (got == img[..., :3]).all()
    assert info["icc_profile"] == icc


def test_the_corpus_reaches_every_named_branch():
    reached = set()
    for name in NAMES:
        for level in wr.LEVELS:
            reached |= wr.features(wr.case_file(name, level)[1])
    missing = sorted(set(wr.FEATURES) - reached)
    assert not missing, "no corpus frame reaches %s" % missing
    assert not set(wr.UNREACHED) & reached


def test_branches_where_they_are_meant_to_be_reached():
    st = wr.case_file("stripes", 0)[1]
    assert all(st["modes"]), st["modes"]  # all 14 modes in one frame
    assert wr.case_file("black", 0)[1]["kinds"] == [5, 0, 0, 0]  # every code has one symbol and costs no bits
    assert wr.case_file("black", 0)[1]["token_bits"] == 0
    assert wr.case_file("const", 0)[1]["kinds"] == [2, 3, 0, 0]  # the first pixel's residual and zero: two symbols
    assert wr.case_file("two_colours", 0)[1]["kinds"][2] > 0
    assert max(wr.case_file("fibonacci", 0)[1]["longest"]) > 15 and wr.case_file("fibonacci", 0)[1]["len_used_max"] == 15
    assert wr.case_file("lengths", 0)[1]["rep_first"] > 0
    st = wr.case_file("deep_header", 0)[1]
    assert max(st["cl_longest"]) == 8 and st["cl_max"] == 7  # the code length code: 8 bits deep, limited to 7
    assert wr.case_file("noise", 6)[1]["matches"] == 0
    st = wr.case_file("rows", 6)[1]
    assert st["dist_row"] > 0
    st = wr.case_file("long_run", 1)[1]
    assert st["len_max"] == wr.MAXLEN and st["nseg"] == 2
    assert wr.case_file("far_%d" % wr.WIN, 1)[1]["dist_max"] == wr.WIN
    assert wr.case_file("far_%d" % (wr.WIN + 1), 1)[1]["dist_max"] < wr.WIN
    assert wr.case_file("3x3_tiles_ragged", 0)[1]["tiles"] == 9
    assert wr.case_file("two_segments", 0)[1]["nseg"] == 2 and wr.case_file("two_segments_plus_1", 0)[1]["nseg"] == 3


def _expand(pairs):
    """the code lengths a decoder reads from (symbol, extra) pairs: 16 repeats the last non-zero length, which starts as 8"""
    out, prev = [], 8
    for s, e in pairs:
        if s < 16:
            out.append(s)
            prev = s or prev
        elif s == 16:
            assert 0 <= e <= 3
            out += [prev] * (3 + e)
        elif s == 17:
            assert 0 <= e <= 7
            out += [0] * (3 + e)
        else:
            assert 0 <= e <= 127
            out += [0] * (11 + e)
    return out


def test_run_length_code_at_its_edges():
    cases = {
        (8, 8, 8): [(16, 0)],                           # a repeat before any non-zero length: the initial 8
        (8, 8): [(8, 0), (8, 0)],
        (0, 0, 8, 8, 8): [(0, 0), (0, 0), (16, 0)],
        (5,) * 4: [(5, 0), (16, 0)],
        (5,) * 7: [(5, 0), (16, 3)],
        (5,) * 8: [(5, 0), (16, 3), (5, 0)],
        (5,) * 10: [(5, 0), (16, 3), (16, 0)],
        (5, 0, 0, 0, 5, 5, 5): [(5, 0), (17, 0), (16, 0)],  # 16 repeats the last NON-ZERO length
        (0,) * 2: [(0, 0), (0, 0)],
        (0,) * 3: [(17, 0)],
        (0,) * 10: [(17, 7)],
        (0,) * 11: [(18, 0)],
        (0,) * 138: [(18, 127)],
        (0,) * 139: [(18, 127), (0, 0)],
        (0,) * 141: [(18, 127), (17, 0)],
        (0,) * 280: [(18, 127), (18, 127), (17, 1)],
    }
    for lens, want in cases.items():
        got = wr.host_rle(lens)
        assert got == want, (lens[:8], len(lens), got)
        assert _expand(got) == list(lens)
    rng = np.random.default_rng(3)
    for _ in range(200):
        lens = np.repeat(rng.integers(0, 16, 40), rng.integers(1, 30, 40))[:280].tolist()
        assert _expand(wr.host_rle(lens)) == lens


@pytest.mark.parametrize("size", wr.NOISE_SIZES)
def test_bound_holds_for_noise(size):
    w, h = size
    img = wr.frame("noise", w, h, seed=w * 31 + h)
    for bits in (0, 2, 9):
        d = wr.data(6, bits, bits)
        bound = wr.host().webp_host_bound(w, h, C.byref(d))
        assert bound > 0
        f = wr.host_file(img, d)
        assert 8 + len(f) <= bound
        assert (wr.decode(f)[1] == img[..., :3]).all()


REFUSED = [dict(lossless=0), dict(lossless=2), dict(predictor_bits=1), dict(predictor_bits=10), dict(entropy_bits=1),
           dict(entropy_bits=10), dict(level=-1), dict(level=10)]


def test_bound_refuses_what_the_encoder_refuses():
    img = wr.frame("mix", 16, 16)
    for bad in REFUSED:
        d = wr.data(**bad)
        assert wr.host().webp_host_bound(16, 16, C.byref(d)) == 0, bad
        assert wr.host().webp_host_encode(img.ctypes.data, 16, 16, C.byref(d)) == 0, bad
    for w, h in ((16384, 1), (1, 16384), (0, 4), (4, 0), (-1, 4)):
        assert wr.host().webp_host_bound(w, h, C.byref(wr.data())) == 0
    assert wr.host().webp_host_bound(16383, 16383, C.byref(wr.data())) > 0
    assert wr.host().webp_host_bound(16383, 16383, C.byref(wr.data(entropy_bits=2))) == 0  # 16 M tiles, a 16-bit index
    no_icc = wr.data()
    no_icc.icc_bytes = 4
    assert wr.host().webp_host_bound(16, 16, C.byref(no_icc)) == 0
    big = wr.data(icc=b"x")  # the bound reads the profile's size alone
    big.icc_bytes = 16 << 20
    assert wr.host().webp_host_bound(16, 16, C.byref(big)) > 16 << 20
    big.icc_bytes = (16 << 20) + 1
    assert wr.host().webp_host_bound(16, 16, C.byref(big)) == 0


def test_python_side():
    from ansel_amd import lib
    l = lib.load()
    assert C.sizeof(abi.WebpData) == 40
    assert l.dt_hip_abi_sizeof(b"webp") == C.sizeof(abi.WebpData)
    d = params.webp()
    assert l.dt_hip_webp_bound(100, 50, C.byref(d)) == wr.host().webp_host_bound(100, 50, C.byref(d)) > 0
    assert l.dt_hip_webp_bound(16384, 50, C.byref(d)) == 0
    d = params.webp(comp_type=1, quality=80, hint=2, level=4, icc=b"abc")
    assert (d.lossless, d.level, d.predictor_bits, d.entropy_bits, d.capacity, d.icc_bytes) == (1, 4, 0, 0, 0, 3)
    assert C.string_at(d.icc, 3) == b"abc"
    assert params.webp().level == 6 and not params.webp().icc
    for bad in (dict(comp_type=0), dict(level=10), dict(level=-1), dict(predictor_bits=1), dict(entropy_bits=10),
                dict(quality=101), dict(hint=4)):
        with pytest.raises(ValueError):
            params.webp(**bad)
    nodes = pipe.light_pipe_nodes(64, 48, 0, 0.0, params.unbounded_coeffs(params.srgb_encode_lut()), with_filmic=False)
    out = pipe.with_webp(nodes, d)
    assert [n.op for n in out[-2:]] == ["export_u8", "export_webp"] and out[:-2] == nodes[:-1]
    assert out[-1].data is d and out[-1].piece.roi_out.width == 64 and out[-1].piece.roi_out.height == 48
    assert pipe.MODULE_BPP["export_webp"] == (4, 0) and pipe.node_bytes_per_px(out[-1]) == 4
    with pytest.raises(ValueError):
        pipe.with_webp(out, d)


# the host file at level 6 on the 1001 x 777 photo-like frame, measured when the encoder was written (libwebp 1.6.0):
# 1 099 502 bytes = 1.137 x libwebp's lossless default (quality 75, method 4: 967 306 bytes) and 0.933 x its fastest
# setting (quality 0, method 0: 1 178 016 bytes).  The encoder is deterministic; the bound is the measured ratio to the
# default rounded up to the next 0.05, the margin being for another libwebp build
PHOTO_RATIO = 1.15


def test_size_against_libwebp_on_a_photo_like_frame():
    from PIL import Image
    w, h = 1001, 777
    img = wr.frame("photo", w, h, seed=1)
    f = wr.host_file(img, wr.data(6))
    assert (wr.decode(f)[1] == img[..., :3]).all()
    sizes = {}
    for name, kw in (("default", dict(quality=75, method=4)), ("fastest", dict(quality=0, method=0))):
        b = io.BytesIO()
        Image.fromarray(img[..., :3]).save(b, "WEBP", lossless=True, **kw)
        sizes[name] = len(b.getvalue())
    print("webp photo %d x %d: ours %d, libwebp default %d (%.3f), fastest %d (%.3f)"
          % (w, h, len(f), sizes["default"], len(f) / sizes["default"], sizes["fastest"], len(f) / sizes["fastest"]))
    assert len(f) < 3 * w * h
    assert len(f) <= PHOTO_RATIO * sizes["default"]


def test_host_twin_runs_clean_under_sanitizers():
    """webp_host.cpp as a program of its own (-DWEBP_HOST_MAIN): a small corpus, each file's layout checked"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "webp_host")
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-DWEBP_HOST_MAIN", "-I" + os.path.join(wr.ROOT, "ansel_amd", "csrc"),
                            "-I" + os.path.join(wr.ROOT, "include"), os.path.join(wr.NATIVE, "webp_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
        if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
            pytest.skip("no sanitizer runtime for g++ here")
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "files" in r.stdout
