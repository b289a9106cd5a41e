"""-m gpu: the "export_jpeg" node of the executor (pipe.cpp) and the batch (pipe_batch.cpp).

  * the light pipe with export_u8 + export_jpeg (pipe.with_jpeg): the file equals tests/jpeg_ref.py of the oracle
    chain's u8 frame -- 24 MP, and the 100 MP frame with orientation 6 (portrait, 8736 x 11648)
  * a batch of 3 frames whose writer reads the length word and writes L bytes gives the single-frame files
  * the node anywhere but last behind export_u8 is refused with a reason; band mode and the host tiler refuse it"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import checkers as ck
import hipcheck as hc
import jpeg_ref as jr
from ansel_amd import abi, filmic, lib, params, pipe, synth
from test_gpu_flip import CFA_OPS, _need_host_memory, orient

pytestmark = pytest.mark.gpu

WRITER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_size_t)


def _nodes(w, h, lut_ptr, lut, jd, orientation=None):
    nodes = pipe.light_pipe_nodes(w, h, lut_ptr, float(lut[0]), params.unbounded_coeffs(lut), with_filmic=True,
                                  filmic=filmic.default_data(), orientation=orientation)
    return pipe.with_jpeg(nodes, jd)


def _file(buf):
    n = int(np.frombuffer(buf[:8].tobytes(), np.uint64)[0])
    assert n != 2 ** 64 - 1 and n + 8 <= len(buf)
    return buf[8:8 + n].tobytes()


def _oracle_u8(nodes, raw):
    """the oracle module by module up to export_u8 (flip: the numpy permutation), then its u8 conversion"""
    o = ck.oracle()
    assert o is not None, "oracle/liboracle.so missing: run build()"
    src = raw
    for n in nodes:
        w, h = n.piece.roi_out.width, n.piece.roi_out.height
        if n.op == "export_u8":
            out = ck.aligned_empty((h, w, 4), np.uint8)
            o.oracle_export_convert_u8(w, h, ck.ptr(src), ck.ptr(out))
            return out
        if n.op == "flip":
            src = orient(src, n.data.orientation)
            continue
        dst = ck.aligned_empty((h, w) if n.op in CFA_OPS else (h, w, 4), np.float32)
        assert ck.call(o, "oracle_" + n.op, n.piece, n.data, np.ascontiguousarray(src), dst) == 0, n.op
        src = dst
    raise AssertionError("no export_u8 node")


def _pipe_file(size, orientation, quality):
    import torch
    hc.hip()
    w, h = synth.SIZES[size]
    ow, oh = params.oriented_size(w, h, orientation or 0)
    lut = params.srgb_encode_lut()
    d_lut = torch.from_numpy(lut).to("cuda:0")
    raw = synth.bayer_mosaic_tiled(w, h, seed=2)
    jd = params.jpeg(quality)
    jd.capacity = pipe.jpeg_bound(ow, oh, jd)
    p = pipe.DevicePipe(0, _nodes(w, h, d_lut.data_ptr(), lut, jd, orientation), fusion=True)
    d_in = torch.from_numpy(raw.view(np.int16)).to("cuda:0")
    d_out = torch.zeros(jd.capacity, dtype=torch.uint8, device="cuda:0")
    t0 = time.time()
    p.process(d_in.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    print("%s light pipe + jpeg q%d: %.1f ms incl. launch" % (size, quality, (time.time() - t0) * 1e3))
    p.close()
    got = _file(d_out.cpu().numpy())
    del d_out, d_in
    torch.cuda.empty_cache()
    u8 = _oracle_u8(_nodes(w, h, lut.ctypes.data, lut, jd, orientation), raw)
    assert u8.shape[:2] == (oh, ow)
    del raw
    exp = jr.encode(u8, quality, jd.subsampling, 1)
    assert got == exp, "%s: device file %d bytes, jpeg_ref of the oracle's u8 frame %d bytes" % (size, len(got), len(exp))


def test_light_pipe_24MP_jpeg_equals_reference_of_the_oracle():
    _need_host_memory(24)
    _pipe_file("24MP", None, 95)


def test_light_pipe_100MP_orientation_6_jpeg_equals_reference_of_the_oracle():
    _need_host_memory(64)
    _pipe_file("100MP", 6, 92)


def test_batch_writer_reads_the_length_word():
    l = hc.hip()
    w, h, nframes, depth = 1504, 1000, 3, 2
    lut = params.srgb_encode_lut()
    d_lut = lib.DeviceBuffer.from_numpy(0, lut)
    jd = params.jpeg(95, icc=bytes(range(256)) * 20, dpi=300)
    jd.capacity = pipe.jpeg_bound(w, h, jd)
    p = pipe.DevicePipe(0, _nodes(w, h, d_lut.ptr, lut, jd), fusion=True)
    frames = [synth.bayer_mosaic(w, h, seed=40 + k) for k in range(nframes)]
    want = []
    din, dout = lib.DeviceBuffer(0, w * h * 2), lib.DeviceBuffer(0, jd.capacity)
    for f in frames:
        din.upload(f)
        p.process(din.ptr, dout.ptr)
        assert l.dt_hip_finish(0) == 1
        want.append(_file(dout.to_numpy((jd.capacity,), np.uint8)))
    nb_in, nb_out = w * h * 2, jd.capacity
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
    # the single-frame path is the reference's encoding of the frame
    assert want[0][:2] == b"\xff\xd8" and want[0][-2:] == b"\xff\xd9"


def _small():
    w, h = 64, 48
    lut = params.srgb_encode_lut()
    jd = params.jpeg(90)
    jd.capacity = pipe.jpeg_bound(w, h, jd)
    nodes = _nodes(w, h, 0, lut, jd)
    return nodes, jd


def test_misplaced_node_is_refused():
    l = hc.hip()
    nodes, jd = _small()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    d_out = lib.DeviceBuffer(0, max(jd.capacity, 64 * 48 * 16))
    jpeg_node = nodes[-1]
    for bad in (nodes[:-2] + [jpeg_node],                                       # behind colorout, not export_u8
                nodes[:-1] + [jpeg_node, pipe.Node("export_rows", abi.ExportRowsData(8, 3), nodes[-2].piece)],  # not last
                [jpeg_node]):                                                    # alone
        p = pipe.DevicePipe(0, bad)
        assert l.dt_hip_pipe_process(p.handle, d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
        assert "export_jpeg" in l.dt_hip_last_error().decode()
        p.close()
    d_in.release()
    d_out.release()


def test_band_mode_and_tiler_refuse_the_node():
    l = hc.hip()
    nodes, jd = _small()
    p = pipe.DevicePipe(0, nodes)
    band = abi.Band(0, 48, 0, 0, 0, 48)
    st = abi.BandState()
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    assert l.dt_hip_pipe_band_begin(p.handle, C.byref(band), d_in.ptr, C.byref(st)) == abi.DT_HIP_INVALID_ARG
    assert "export_jpeg" in l.dt_hip_last_error().decode()
    p.close()
    d_in.release()
    assert l.dt_hip_band_halo_rows(b"export_jpeg", C.byref(nodes[-1].piece), C.cast(C.byref(jd), C.c_void_p),
                                   C.sizeof(jd)) == -1
