"""-m gpu: the "export_png" node of the executor (pipe.cpp) and the batch (pipe_batch.cpp).

  * the light pipe + export_png (pipe.with_png): the file decodes to exactly the oracle chain's u8 / u16 frame, alpha
    dropped -- 24 MP at 8 and 16 bits, and the 100 MP frame with orientation 6 at 8 bits; at 24 MP it equals the host
    build byte for byte, and at level 5 it is at most 1.10 x libpng's file of the same frame
  * a batch of 3 frames whose writer reads the length word and writes L bytes gives the single-frame files
  * the node anywhere but last behind the matching export node is refused with a reason; band mode and the host tiler
    refuse it"""
import ctypes as C
import time

import numpy as np
import pytest

import checkers as ck
import hipcheck as hc
import png_ref as pr
from ansel_amd import abi, filmic, lib, params, pipe, synth
from test_gpu_flip import CFA_OPS, _need_host_memory, orient

pytestmark = pytest.mark.gpu

WRITER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_size_t)


def _nodes(w, h, lut_ptr, lut, pd, orientation=None):
    nodes = pipe.light_pipe_nodes(w, h, lut_ptr, float(lut[0]), params.unbounded_coeffs(lut), with_filmic=True,
                                  filmic=filmic.default_data(), orientation=orientation)
    return pipe.with_png(nodes, pd)


def _file(buf):
    n = int(np.frombuffer(buf[:8].tobytes(), np.uint64)[0])
    assert n != 2 ** 64 - 1 and n + 8 <= len(buf)
    return buf[8:8 + n].tobytes()


def _oracle_export(nodes, raw):
    """the oracle module by module up to the export node in front of export_png, then its conversion (RGBA)"""
    o = ck.oracle()
    assert o is not None, "oracle/liboracle.so missing: run build()"
    src = raw
    for n in nodes:
        w, h = n.piece.roi_out.width, n.piece.roi_out.height
        if n.op in ("export_u8", "export_u16"):
            out = ck.aligned_empty((h, w, 4), np.uint8 if n.op == "export_u8" else np.uint16)
            getattr(o, "oracle_" + n.op.replace("export_", "export_convert_"))(w, h, ck.ptr(src), ck.ptr(out))
            return out
        if n.op == "flip":
            src = orient(src, n.data.orientation)
            continue
        dst = ck.aligned_empty((h, w) if n.op in CFA_OPS else (h, w, 4), np.float32)
        assert ck.call(o, "oracle_" + n.op, n.piece, n.data, np.ascontiguousarray(src), dst) == 0, n.op
        src = dst
    raise AssertionError("no export node")


def _pipe_file(size, orientation, bpp, compare_host):
    import torch
    hc.hip()
    w, h = synth.SIZES[size]
    ow, oh = params.oriented_size(w, h, orientation or 0)
    lut = params.srgb_encode_lut()
    d_lut = torch.from_numpy(lut).to("cuda:0")
    raw = synth.bayer_mosaic_tiled(w, h, seed=2)
    pd = params.png(bpp=bpp)
    pd.capacity = pipe.png_bound(ow, oh, pd)
    p = pipe.DevicePipe(0, _nodes(w, h, d_lut.data_ptr(), lut, pd, orientation), fusion=True)
    d_in = torch.from_numpy(raw.view(np.int16)).to("cuda:0")
    d_out = torch.zeros(pd.capacity, dtype=torch.uint8, device="cuda:0")
    t0 = time.time()
    p.process(d_in.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    print("%s light pipe + png %d bits: %.1f ms incl. launch" % (size, bpp, (time.time() - t0) * 1e3))
    p.close()
    got = _file(d_out.cpu().numpy())
    del d_out, d_in
    torch.cuda.empty_cache()
    frame = _oracle_export(_nodes(w, h, lut.ctypes.data, lut, pd, orientation), raw)
    del raw
    assert frame.shape[:2] == (oh, ow)
    assert pr.inflate(got) == pr.host_filtered(frame)
    if pr.ref() is not None:
        rgb, _, _ = pr.libpng_read(got, ow, oh, bpp)
        assert np.array_equal(rgb, frame[..., :3])
        ref = pr.libpng_file(frame, 5)
        print("%s %d bits level 5: device %d bytes, libpng %d bytes, ratio %.4f"
              % (size, bpp, len(got), len(ref), len(got) / len(ref)))
        assert len(got) <= 1.10 * len(ref)
    if compare_host:
        assert got == pr.host_file(frame, 5)


def test_light_pipe_24MP_png_8_bits():
    _need_host_memory(24)
    _pipe_file("24MP", None, 8, True)


def test_light_pipe_24MP_png_16_bits():
    _need_host_memory(32)
    _pipe_file("24MP", None, 16, False)


def test_light_pipe_100MP_orientation_6_png_8_bits():
    _need_host_memory(64)
    _pipe_file("100MP", 6, 8, False)


def test_batch_writer_reads_the_length_word():
    l = hc.hip()
    w, h, nframes, depth = 1504, 1000, 3, 2
    lut = params.srgb_encode_lut()
    d_lut = lib.DeviceBuffer.from_numpy(0, lut)
    pd = params.png(bpp=16, icc=bytes(range(256)) * 20, dpi=300)
    pd.capacity = pipe.png_bound(w, h, pd)
    p = pipe.DevicePipe(0, _nodes(w, h, d_lut.ptr, lut, pd), fusion=True)
    frames = [synth.bayer_mosaic(w, h, seed=40 + k) for k in range(nframes)]
    want = []
    din, dout = lib.DeviceBuffer(0, w * h * 2), lib.DeviceBuffer(0, pd.capacity)
    for f in frames:
        din.upload(f)
        p.process(din.ptr, dout.ptr)
        assert l.dt_hip_finish(0) == 1
        want.append(_file(dout.to_numpy((pd.capacity,), np.uint8)))
    nb_in, nb_out = w * h * 2, pd.capacity
    pin_in = [l.dt_hip_alloc_host_pinned(nb_in) for _ in range(depth)]
    pin_out = [l.dt_hip_alloc_host_pinned(nb_out) for _ in range(depth)]
    assert all(pin_in) and all(pin_out)
    written = []

    def write_image(user, seq, host_out, nbytes):
        n = C.c_uint64.from_address(host_out).value
        written.append((seq, C.string_at(host_out + 8, n) if n + 8 <= nbytes else None))
        return 0

    cb = WRITER(write_image)
    b = l.dt_hip_batch_new(p.handle, depth, nb_in, nb_out)
    assert b and l.dt_hip_batch_set_writer(b, cb, None) == 0
    for k, f in enumerate(frames):
        if k >= depth:
            assert l.dt_hip_batch_wait(b, k % depth) == 0
        C.memmove(pin_in[k % depth], f.ctypes.data, nb_in)
        assert l.dt_hip_batch_submit(b, pin_in[k % depth], pin_out[k % depth]) == k % depth, l.dt_hip_last_error()
    assert l.dt_hip_batch_drain(b) == 0
    l.dt_hip_batch_free(b)
    for ptr in pin_in + pin_out:
        l.dt_hip_free_host_pinned(ptr)
    p.close()
    assert [s for s, _ in written] == list(range(nframes))
    for k, (_, got) in enumerate(written):
        assert got == want[k], "frame %d" % k
    assert want[0][:8] == b"\x89PNG\r\n\x1a\n" and pr.chunks(want[0])[-1][0] == "IEND"


def _small(bpp=8):
    w, h = 64, 48
    lut = params.srgb_encode_lut()
    pd = params.png(bpp=bpp)
    pd.capacity = pipe.png_bound(w, h, pd)
    return _nodes(w, h, 0, lut, pd), pd


def test_misplaced_node_is_refused():
    l = hc.hip()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    for bpp in (8, 16):
        nodes, pd = _small(bpp)
        d_out = lib.DeviceBuffer(0, max(pd.capacity, 64 * 48 * 16))
        png_node = nodes[-1]
        other = "export_u16" if bpp == 8 else "export_u8"
        for bad in (nodes[:-2] + [png_node],                                       # behind colorout
                    nodes[:-2] + [pipe.Node(other, None, nodes[-2].piece), png_node],  # behind the other depth's export
                    nodes[:-1] + [png_node, pipe.Node("export_rows", abi.ExportRowsData(8, 3), nodes[-2].piece)],
                    [png_node]):
            p = pipe.DevicePipe(0, bad)
            assert l.dt_hip_pipe_process(p.handle, d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
            assert "export_png" in l.dt_hip_last_error().decode()
            p.close()
        d_out.release()
    d_in.release()


def test_band_mode_and_tiler_refuse_the_node():
    l = hc.hip()
    nodes, pd = _small()
    p = pipe.DevicePipe(0, nodes)
    band = abi.Band(0, 48, 0, 0, 0, 48)
    st = abi.BandState()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    assert l.dt_hip_pipe_band_begin(p.handle, C.byref(band), d_in.ptr, C.byref(st)) == abi.DT_HIP_INVALID_ARG
    assert "export_png" in l.dt_hip_last_error().decode()
    p.close()
    d_in.release()
    assert l.dt_hip_band_halo_rows(b"export_png", C.byref(nodes[-1].piece), C.cast(C.byref(pd), C.c_void_p),
                                   C.sizeof(pd)) == -1
