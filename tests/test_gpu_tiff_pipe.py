"""-m gpu: the "export_tiff" node of the executor (pipe.cpp).

  * the light pipe on a small mosaic through pipe.with_tiff() at 8, 16 and 32 bits, without compression and deflated with
    the predictor: the file's decoded samples (tiff_ref.decode(), and libtiff where it is loaded) equal those of the same
    pipe ending in export_u8, in export_u16, and in its float output
  * the three wrong placements are refused in plan() with a message, and so is a pipe of the node alone
  * band mode and the tiler refuse the node"""
import ctypes as C

import numpy as np
import pytest

import hipcheck as hc
import tiff_ref as tr
from ansel_amd import abi, filmic, lib, params, pipe, synth

pytestmark = pytest.mark.gpu

W, H = 194, 130


def _base(w, h, lut_ptr, lut):
    return pipe.light_pipe_nodes(w, h, lut_ptr, float(lut[0]), params.unbounded_coeffs(lut), with_filmic=True,
                                 filmic=filmic.default_data())


def _run(nodes, d_in, out_bytes):
    l = hc.hip()
    d_out = lib.DeviceBuffer.from_numpy(0, np.zeros(out_bytes, np.uint8))
    p = pipe.DevicePipe(0, nodes, fusion=True)
    p.process(d_in.ptr, d_out.ptr)
    assert l.dt_hip_finish(0) == 1
    p.close()
    buf = d_out.to_numpy((out_bytes,), np.uint8)
    d_out.release()
    return buf


@pytest.fixture(scope="module")
def frames():
    """the pipe's own three outputs, computed once: RGBA u8, RGBA u16, RGBA f32 (as bits)"""
    hc.hip()
    lut = params.srgb_encode_lut()
    d_lut = lib.DeviceBuffer.from_numpy(0, lut)
    d_in = lib.DeviceBuffer.from_numpy(0, synth.bayer_mosaic(W, H, seed=11))
    nodes = _base(W, H, d_lut.ptr, lut)
    u8 = list(nodes[:-1]) + [pipe.Node("export_u8", None, nodes[-1].piece)]
    out = {8: _run(u8, d_in, W * H * 4).reshape(H, W, 4),
           16: _run(nodes, d_in, W * H * 8).view(np.uint16).reshape(H, W, 4),
           32: _run(nodes[:-1], d_in, W * H * 16).view(np.uint32).reshape(H, W, 4)}
    yield nodes, d_in, out
    d_in.release()
    d_lut.release()


@pytest.mark.parametrize("bpp", [8, 16, 32])
@pytest.mark.parametrize("compress", [0, 2])
def test_light_pipe_file_decodes_to_the_pipes_own_samples(frames, bpp, compress):
    nodes, d_in, out = frames
    td = params.tiff(bpp=bpp, compress=compress, icc=bytes(range(200)), dpi=300)
    td.capacity = pipe.tiff_bound(W, H, td)
    buf = _run(pipe.with_tiff(nodes, td), d_in, td.capacity)
    n = int(buf[:8].view(np.uint64)[0])
    assert n != 2 ** 64 - 1 and 8 + n <= td.capacity
    f = buf[8:8 + n].tobytes()
    tr.check_layout(f)
    want = tr.samples(out[bpp], 3)
    assert len(set(want)) > 16, "the pipe's frame is flat"
    assert tr.decode(f).tobytes() == want
    if tr.libtiff() is not None:
        assert tr.libtiff_read(f) == want
    td.capacity = 0
    assert f == tr.host_file(out[bpp], td)


def _small(bpp):
    lut = params.srgb_encode_lut()
    td = params.tiff(bpp=bpp, compress=1)
    td.capacity = pipe.tiff_bound(64, 48, td)
    return pipe.with_tiff(_base(64, 48, 0, lut), td), td


def test_misplaced_node_is_refused():
    l = hc.hip()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    for bpp in (8, 16, 32):
        nodes, td = _small(bpp)
        d_out = lib.DeviceBuffer(0, max(td.capacity, 64 * 48 * 16))
        node = nodes[-1]
        base = nodes[:-1] if bpp == 32 else nodes[:-2]  # ... colorout
        rgb = base[-1].piece
        wrong = {8: [base + [node], base + [pipe.Node("export_u16", None, rgb), node]],
                 16: [base + [node], base + [pipe.Node("export_u8", None, rgb), node]],
                 32: [base + [pipe.Node("export_u16", None, rgb), node], base + [pipe.Node("export_u8", None, rgb), node]]}[bpp]
        wrong.append(nodes + [pipe.Node("export_rows", abi.ExportRowsData(8, 3), rgb)])  # not the last node
        wrong.append([node])
        for bad in wrong:
            p = pipe.DevicePipe(0, bad)
            assert l.dt_hip_pipe_process(p.handle, d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
            assert "export_tiff" in l.dt_hip_last_error().decode()
            p.close()
        d_out.release()
    d_in.release()


def test_band_mode_and_tiler_refuse_the_node():
    l = hc.hip()
    nodes, td = _small(16)
    p = pipe.DevicePipe(0, nodes)
    band = abi.Band(0, 48, 0, 0, 0, 48)
    st = abi.BandState()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    assert l.dt_hip_pipe_band_begin(p.handle, C.byref(band), d_in.ptr, C.byref(st)) == abi.DT_HIP_INVALID_ARG
    assert "export_tiff" in l.dt_hip_last_error().decode()
    p.close()
    d_in.release()
    assert l.dt_hip_band_halo_rows(b"export_tiff", C.byref(nodes[-1].piece), C.cast(C.byref(td), C.c_void_p),
                                   C.sizeof(td)) == -1
