"""not gpu: the JPEG encoder's pieces that run without a device.

  * tests/jpeg_ref.py (the device's checker) is byte-identical to Pillow's libjpeg(-turbo) over sizes, contents,
    qualities, the three sampling modes, optimize on / off, ICC profiles (1 and 3 APP2 chunks) and dpi
  * the table builder of ansel_amd/csrc/jpeg_huff.h, compiled for the host, gives Pillow's four DHT markers from
    jpeg_ref's symbol counts
  * dt_hip_jpeg_bound() is at least the file Pillow writes for uniform noise at quality 100, and refuses what the
    encoder refuses
  * abi.JpegData matches the library's struct; params.jpeg() maps Ansel's export quality and refuses 80 > q > 95
  * pipe.with_jpeg() swaps the trailing export_u16 for export_u8 + export_jpeg"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_ref as jr
from ansel_amd import abi, lib, params, pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL = pytest.importorskip("PIL")

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (1001, 777)]
KINDS = ["gradient", "zero", "full", "primaries", "noise"]


def markers(data):
    """[(marker, payload)] up to SOS"""
    out, i = [], 2
    while i < len(data):
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, data[i + 4:i + 2 + n]))
        if m == 0xDA:
            break
        i += 2 + n
    return out


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("ss", [0, 1, 2])
def test_reference_equals_pillow(w, h, ss):
    for ki, kind in enumerate(KINDS):
        img = jr.frame(kind, w, h, seed=ki + w)
        for opt in (0, 1):
            for q in ((50, 80, 90, 92, 95, 100) if w * h < 10000 else (80, 95)):
                assert jr.encode(img, q, ss, opt) == jr.pillow(img, q, ss, opt), (kind, opt, q)


def test_reference_equals_pillow_two_megapixels():
    img = jr.frame("gradient", 1733, 1157, seed=3)
    for ss in (0, 1, 2):
        assert jr.encode(img, 95, ss, 1) == jr.pillow(img, 95, ss, 1), ss


@pytest.mark.parametrize("icc_bytes", [3000, 140000])
def test_reference_equals_pillow_icc_and_dpi(icc_bytes):
    icc = np.random.default_rng(icc_bytes).integers(0, 256, icc_bytes, dtype=np.uint8).tobytes()
    img = jr.frame("gradient", 65, 47, seed=1)
    for ss in (0, 2):
        for opt in (0, 1):
            ref = jr.encode(img, 92, ss, opt, icc=icc, density=(1, 300, 300))
            assert ref == jr.pillow(img, 92, ss, opt, icc=icc, dpi=(300, 300))
    n = sum(1 for m, _ in markers(ref) if m == 0xE2)
    assert n == -(-icc_bytes // jr.ICC_CHUNK)


@pytest.fixture(scope="module")
def huff_host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("jpeg_huff") / "libjpeg_huff_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "ansel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "jpeg_huff_host.cpp"), "-o", so])
    l = C.CDLL(so)
    l.jh_host_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return l


@pytest.mark.parametrize("kind,ss,q", [("gradient", 0, 95), ("noise", 2, 90), ("primaries", 1, 92), ("zero", 2, 80),
                                       ("gradient", 2, 100)])
def test_host_table_builder_gives_pillows_tables(huff_host, kind, ss, q):
    img = jr.frame(kind, 333, 211, seed=7)
    coefs, comp = jr.coefficients(img[..., :3], q, ss)
    tabs, syms, _, _ = jr.symbols(coefs, comp)
    f = jr.frequencies(tabs, syms)
    dht = [p for m, p in markers(jr.pillow(img, q, ss, 1)) if m == 0xC4]
    assert len(dht) == 4
    for t in range(4):
        freq = np.ascontiguousarray(f[t, :256], np.int64)
        bits = np.zeros(16, np.uint8)
        vals = np.zeros(256, np.uint8)
        n = huff_host.jh_host_table(freq.ctypes.data, bits.ctypes.data, vals.ctypes.data)
        got = bytes([(t & 1) << 4 | t >> 1]) + bits.tobytes() + vals[:n].tobytes()
        assert got == dht[t], t
        assert (bits.astype(int).sum()) == n


def test_host_table_builder_limits_code_lengths(huff_host):
    """Fibonacci counts make a tree deeper than 16: the Annex K.3 adjustment, as jpeg_ref restates libjpeg"""
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    freq = np.zeros(256, np.int64)
    freq[:30] = fib
    bits = np.zeros(16, np.uint8)
    vals = np.zeros(256, np.uint8)
    n = huff_host.jh_host_table(freq.ctypes.data, bits.ctypes.data, vals.ctypes.data)
    rb, rv = jr.gen_optimal_table(np.concatenate([freq, [0]]))
    assert list(bits) == rb and list(vals[:n]) == rv
    assert sum(int(b) << (16 - i - 1) for i, b in enumerate(bits)) < 1 << 16  # a prefix code leaving all-ones free


def _bound(w, h, ss, icc=None):
    d = abi.JpegData(quality=100, subsampling=ss, optimize_coding=0, density_unit=0, x_density=1, y_density=1)
    if icc:
        buf = C.create_string_buffer(icc, len(icc))
        d.icc, d.icc_bytes = C.cast(buf, C.c_void_p), len(icc)
    return lib.load().dt_hip_jpeg_bound(w, h, C.byref(d))


@pytest.mark.parametrize("ss", [0, 1, 2])
def test_bound_holds_the_worst_file(ss):
    for w, h in ((1, 1), (17, 33), (640, 480)):
        img = jr.frame("noise", w, h, seed=w)
        for opt in (0, 1):
            assert _bound(w, h, ss) >= 8 + len(jr.pillow(img, 100, ss, opt))
    icc = bytes(200000)
    img = jr.frame("noise", 64, 64, seed=1)
    assert _bound(64, 64, ss, icc) >= 8 + len(jr.pillow(img, 100, ss, 0, icc=icc))


def test_bound_refuses_what_the_encoder_refuses():
    for w, h, q, ss in [(0, 4, 90, 0), (65536, 4, 90, 0), (4, 65536, 90, 0), (4, 4, 0, 0), (4, 4, 101, 0), (4, 4, 90, 3)]:
        d = abi.JpegData(quality=q, subsampling=ss)
        assert lib.load().dt_hip_jpeg_bound(w, h, C.byref(d)) == 0
        assert lib.load().dt_hip_last_error().decode()
    assert _bound(65535, 65535, 2) > 0


def test_struct_matches_the_library():
    assert lib.load().dt_hip_abi_sizeof(b"jpeg") == C.sizeof(abi.JpegData)
    assert (abi.DT_HIP_JPEG_444, abi.DT_HIP_JPEG_422, abi.DT_HIP_JPEG_420) == (0, 1, 2)


def test_params_mapping():
    for q in range(80, 96):
        d = params.jpeg(q)
        ss = 0 if q > 92 else 1 if q > 90 else 2
        assert (d.quality, d.subsampling, d.optimize_coding) == (q, ss, 1)
        assert (d.density_unit, d.x_density, d.y_density, d.icc_bytes) == (0, 1, 1, 0)
    for q in (1, 49, 50, 79, 96, 100):
        with pytest.raises(ValueError):
            params.jpeg(q)
    d = params.jpeg(95, icc=b"\1\2\3", dpi=300)
    assert (d.density_unit, d.x_density, d.y_density) == (1, 300, 300)
    assert d.icc_bytes == 3 and C.string_at(d.icc, 3) == b"\1\2\3"


def test_with_jpeg_swaps_the_export_node():
    lut = params.srgb_encode_lut()
    nodes = pipe.light_pipe_nodes(64, 48, lut.ctypes.data, float(lut[0]), params.unbounded_coeffs(lut))
    d = params.jpeg(90)
    out = pipe.with_jpeg(nodes, d)
    assert [n.op for n in out] == [n.op for n in nodes[:-1]] + ["export_u8", "export_jpeg"]
    assert out[-1].data is d and (out[-1].piece.roi_out.width, out[-1].piece.roi_out.height) == (64, 48)
    assert [n.op for n in nodes][-1] == "export_u16"
    with pytest.raises(ValueError):
        pipe.with_jpeg(out, d)
