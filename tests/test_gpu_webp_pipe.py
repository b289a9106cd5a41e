"""-m gpu: the "export_webp" node of the executor (pipe.cpp).

  * the light pipe on a small mosaic through pipe.with_webp(): libwebp decodes the file to the RGB of the same pipe
    ending in export_u8 -- with fusion on and off, and with a flip (orientation 6) in front; the file equals the host
    build's file of that frame
  * the node is refused in plan() when it is not last, behind export_u16, or alone
  * band mode and the tiler refuse the node"""
import ctypes as C

import numpy as np
import pytest

import hipcheck as hc
import webp_ref as wr
from ansel_amd import abi, filmic, lib, params, pipe, synth

pytestmark = pytest.mark.gpu

W, H = 194, 130


def _base(w, h, lut_ptr, lut, orientation=None):
    return pipe.light_pipe_nodes(w, h, lut_ptr, float(lut[0]), params.unbounded_coeffs(lut), with_filmic=True,
                                 filmic=filmic.default_data(), orientation=orientation)


def _run(nodes, d_in, out_bytes, fusion=True):
    l = hc.hip()
    d_out = lib.DeviceBuffer.from_numpy(0, np.zeros(out_bytes, np.uint8))
    p = pipe.DevicePipe(0, nodes, fusion=fusion)
    p.process(d_in.ptr, d_out.ptr)
    assert l.dt_hip_finish(0) == 1
    p.close()
    buf = d_out.to_numpy((out_bytes,), np.uint8)
    d_out.release()
    return buf


@pytest.fixture(scope="module")
def setup():
    hc.hip()
    lut = params.srgb_encode_lut()
    d_lut = lib.DeviceBuffer.from_numpy(0, lut)
    d_in = lib.DeviceBuffer.from_numpy(0, synth.bayer_mosaic(W, H, seed=11))
    yield lut, d_lut, d_in
    d_in.release()
    d_lut.release()


@pytest.mark.parametrize("orientation", [None, 6])
@pytest.mark.parametrize("fusion", [True, False])
def test_light_pipe_file_decodes_to_the_pipes_own_frame(setup, orientation, fusion):
    lut, d_lut, d_in = setup
    nodes = _base(W, H, d_lut.ptr, lut, orientation)
    ow, oh = nodes[-1].piece.roi_out.width, nodes[-1].piece.roi_out.height
    assert (ow, oh) == ((W, H) if orientation is None else (H, W))
    u8 = list(nodes[:-1]) + [pipe.Node("export_u8", None, nodes[-1].piece)]
    want = _run(u8, d_in, ow * oh * 4, fusion).reshape(oh, ow, 4)
    assert len(np.unique(want[..., :3])) > 16, "the pipe's frame is flat"
    wd = params.webp(icc=bytes(range(200)))
    wd.capacity = pipe.webp_bound(ow, oh, wd)
    buf = _run(pipe.with_webp(nodes, wd), d_in, wd.capacity, fusion)
    n = int(buf[:8].view(np.uint64)[0])
    assert n != 2 ** 64 - 1 and 8 + n <= wd.capacity
    f = buf[8:8 + n].tobytes()
    wr.check_layout(f, ow, oh, bytes(range(200)))
    mode, px, info = wr.decode(f)
    assert mode == "RGB" and (px == want[..., :3]).all()
    assert info["icc_profile"] == bytes(range(200))
    assert f == wr.host_file(want, wr.data(6, icc=bytes(range(200))))


def _small():
    lut = params.srgb_encode_lut()
    wd = params.webp()
    wd.capacity = pipe.webp_bound(64, 48, wd)
    return pipe.with_webp(_base(64, 48, 0, lut), wd), wd


def test_misplaced_node_is_refused():
    l = hc.hip()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    nodes, wd = _small()
    d_out = lib.DeviceBuffer(0, max(wd.capacity, 64 * 48 * 16))
    node = nodes[-1]
    base = nodes[:-2]  # ... colorout
    rgb = base[-1].piece
    wrong = [base + [node],                                                   # behind a float node
             base + [pipe.Node("export_u16", None, rgb), node],               # behind export_u16
             nodes + [pipe.Node("export_rows", abi.ExportRowsData(8, 3), rgb)],  # not the last node
             [node]]
    for bad in wrong:
        p = pipe.DevicePipe(0, bad)
        assert l.dt_hip_pipe_process(p.handle, d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
        assert "export_webp" in l.dt_hip_last_error().decode()
        p.close()
    d_out.release()
    d_in.release()


def test_band_mode_and_tiler_refuse_the_node():
    l = hc.hip()
    nodes, wd = _small()
    p = pipe.DevicePipe(0, nodes)
    band = abi.Band(0, 48, 0, 0, 0, 48)
    st = abi.BandState()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    assert l.dt_hip_pipe_band_begin(p.handle, C.byref(band), d_in.ptr, C.byref(st)) == abi.DT_HIP_INVALID_ARG
    assert "export_webp" in l.dt_hip_last_error().decode()
    p.close()
    d_in.release()
    assert l.dt_hip_band_halo_rows(b"export_webp", C.byref(nodes[-1].piece), C.cast(C.byref(wd), C.c_void_p),
                                   C.sizeof(wd)) == -1
