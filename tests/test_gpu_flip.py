"""-m gpu: the flip module (orientation) on the device.

  * the kernel: every orientation, float4 and 1-channel f32, odd / degenerate sizes -- every output word equals the
    numpy permutation of the input (uint32 views: NaN payloads and signed zeros included)
  * the named table of include/ansel_hip.h pinned against np.rot90 / .T
  * the host tiler (dt_hip_default_process_tiling_roi, op "flip") equals the untiled run
  * the executor: an orientation-0 node changes neither launches nor words; a rotated pipe equals the oracle's module
    chain up to flip, numpy-oriented, then the oracle chain after it (small frames for all 8 orientations, the 24 MP full
    pipe for the four swapping ones = EXIF 5-8, the light pipe at 100 MP with orientation 6)
  * band mode refuses a flip node with a reason"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import checkers as ck
import hipcheck as hc
from ansel_amd import abi, filmic, lib, params, pipe, synth, tiled

pytestmark = pytest.mark.gpu

CFA_OPS = ("rawprepare", "temperature", "highlights")


def orient(x, o):
    y = x
    if o & 1:
        y = y[::-1]
    if o & 2:
        y = y[:, ::-1]
    if o & 4:
        y = np.swapaxes(y, 0, 1)
    return np.ascontiguousarray(y)


def _words(w, h, ch, seed):
    """random 32-bit words: quiet and signalling NaN payloads, infinities, denormals and signed zeros all occur"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, size=(h, w, ch) if ch > 1 else (h, w), dtype=np.uint64).astype(np.uint32)
    flat = x.reshape(-1)
    special = np.array([0x7fc00001, 0x7f800001, 0xffbadbad, 0x7f800000, 0xff800000, 0x80000000, 0x00000001], np.uint32)
    flat[:min(flat.size, special.size)] = special[:min(flat.size, special.size)]
    return x


def _device_flip(x, o, ch):
    l = hc.hip()
    h, w = x.shape[:2]
    ow, oh = params.oriented_size(w, h, o)
    piece = abi.Piece.make(w, h, channels=ch, roi_out=abi.Roi.make(0, 0, ow, oh))
    d_in = lib.DeviceBuffer.from_numpy(0, x)
    d_out = lib.DeviceBuffer(0, x.nbytes)
    lib.check(l.dt_hip_iop_flip_process(0, C.byref(piece), C.byref(abi.FlipData(o)), d_in.ptr, d_out.ptr), "flip")
    assert l.dt_hip_finish(0) == 1
    out = d_out.to_numpy((oh, ow, ch) if ch > 1 else (oh, ow), np.uint32)
    d_in.release()
    d_out.release()
    return out


@pytest.mark.parametrize("ch", [4, 1])
@pytest.mark.parametrize("w,h", [(1, 1), (1, 257), (257, 1), (63, 65), (4097, 3), (3, 4097), (32, 32), (96, 33), (1000, 777)])
@pytest.mark.parametrize("o", range(8))
def test_kernel_equals_the_numpy_permutation(o, w, h, ch):
    x = _words(w, h, ch, seed=o * 7 + w + 3 * h + ch)
    got = _device_flip(x, o, ch)
    exp = orient(x, o)
    assert got.shape == exp.shape
    bad = int((got != exp).sum())
    assert bad == 0, "orientation %d, %d x %d x %d: %d words differ" % (o, w, h, ch, bad)


def test_the_named_table():
    """include/ansel_hip.h: 3 rotate 180, 4 transpose, 5 rotate 90 clockwise (EXIF 6), 6 rotate 90 counter-clockwise
    (EXIF 8), 7 transverse"""
    x = _words(37, 21, 4, seed=5)
    want = {0: x, 1: x[::-1], 2: x[:, ::-1], 3: np.rot90(x, 2), 4: np.swapaxes(x, 0, 1), 5: np.rot90(x, -1),
            6: np.rot90(x, 1), 7: np.swapaxes(np.rot90(x, 2), 0, 1)}
    for o, y in want.items():
        assert np.array_equal(_device_flip(x, o, 4), y), o
    for tag, o in params.EXIF_ORIENTATION.items():
        assert np.array_equal(orient(x, o), want[o]), tag


def test_process_refuses_bad_arguments():
    l = hc.hip()
    buf = lib.DeviceBuffer(0, 16 * 64)
    buf2 = lib.DeviceBuffer(0, 16 * 64)
    p = abi.Piece.make(8, 8)
    assert l.dt_hip_iop_flip_process(0, C.byref(p), C.byref(abi.FlipData(-1)), buf.ptr, buf2.ptr) == abi.DT_HIP_INVALID_ARG
    p = abi.Piece.make(16, 4)  # orientation 5 wants roi_out 4 x 16
    assert l.dt_hip_iop_flip_process(0, C.byref(p), C.byref(abi.FlipData(5)), buf.ptr, buf2.ptr) == abi.DT_HIP_INVALID_ARG
    assert "roi_out" in l.dt_hip_last_error().decode()
    p = abi.Piece.make(8, 8)
    assert l.dt_hip_iop_flip_process(0, C.byref(p), C.byref(abi.FlipData(2)), buf.ptr, buf.ptr) == abi.DT_HIP_INVALID_ARG


@pytest.mark.parametrize("o", range(8))
def test_host_tiled_run_equals_the_untiled_one(o):
    l = hc.hip()
    w, h = 301, 203
    x = _words(w, h, 4, seed=40 + o)
    whole = _device_flip(x, o, 4)
    ow, oh = params.oriented_size(w, h, o)
    piece = abi.Piece.make(w, h, channels=4, roi_out=abi.Roi.make(0, 0, ow, oh))
    t = abi.Tiling()
    l.dt_hip_default_tiling(C.byref(piece), 0, C.byref(t))
    out = np.zeros((oh, ow, 4), np.uint32)
    d = abi.FlipData(o)
    # ~ 90 x 90 pixels per tile: a grid of several tiles each way
    rc = l.dt_hip_default_process_tiling_roi(0, b"flip", C.byref(piece), C.cast(C.byref(d), C.c_void_p), C.sizeof(d),
                                             C.byref(t), x.ctypes.data, out.ctypes.data, 16, 16, 2 * 16 * 90 * 90)
    lib.check(rc, "dt_hip_default_process_tiling_roi(flip)")
    assert np.array_equal(out, whole)
    # the point-to-point tiler refuses flip (a mirrored tile lands elsewhere)
    assert l.dt_hip_default_process_tiling_ptp(0, b"flip", C.byref(piece), C.cast(C.byref(d), C.c_void_p), C.sizeof(d),
                                               C.byref(t), x.ctypes.data, out.ctypes.data, 16, 16, 0) == abi.DT_HIP_INVALID_ARG


# ---- the executor -------------------------------------------------------------------------------------------------
def _lut():
    lut = params.srgb_encode_lut()
    return lut, params.unbounded_coeffs(lut)


def _run_pipe(nodes, raw, ow, oh, profile=False):
    l = hc.hip()
    p = pipe.DevicePipe(0, nodes, fusion=True)
    d_in = lib.DeviceBuffer.from_numpy(0, raw)
    d_out = lib.DeviceBuffer(0, ow * oh * 8)
    if profile:
        l.dt_hip_events_reset(0)
        l.dt_hip_events_enable(0, 1)
    p.process(d_in.ptr, d_out.ptr)
    assert l.dt_hip_finish(0) == 1
    launches = None
    if profile:
        l.dt_hip_events_wait_for(0)
        tags, ms, cnt = (C.c_char_p * 64)(), (C.c_float * 64)(), (C.c_int * 64)()
        n = l.dt_hip_events_profiling(0, tags, ms, cnt, 64)
        launches = sorted((tags[i].decode(), cnt[i]) for i in range(n))
        l.dt_hip_events_enable(0, 0)
        l.dt_hip_events_reset(0)
    out = d_out.to_numpy((oh, ow, 4), np.uint16)
    groups = p.num_groups
    p.close()
    d_in.release()
    d_out.release()
    return out, groups, launches


def oracle_chain(nodes, raw, start=None):
    """the oracle module by module; a flip node is the numpy permutation of the formula.  start: (index, buffer) to
    resume from"""
    o = ck.oracle()
    assert o is not None, "oracle/liboracle.so missing: run build()"
    k0, src = start if start is not None else (0, raw)
    for k in range(k0, len(nodes)):
        n = nodes[k]
        w, h = n.piece.roi_out.width, n.piece.roi_out.height
        if n.op == "export_u16":
            out = ck.aligned_empty((h, w, 4), np.uint16)
            o.oracle_export_convert_u16(w, h, ck.ptr(src), ck.ptr(out))
            return out
        if n.op == "flip":
            src = orient(src, n.data.orientation)
            assert src.shape[:2] == (h, w)
            continue
        dst = ck.aligned_empty((h, w) if n.op in CFA_OPS else (h, w, 4), np.float32)
        assert ck.call(o, "oracle_" + n.op, n.piece, n.data, np.ascontiguousarray(src), dst) == 0, n.op
        src = dst
    raise AssertionError("no export_u16 node")


def _compare(dev, exp, what):
    assert dev.shape == exp.shape, (dev.shape, exp.shape)
    bad = 0
    for r0 in range(0, dev.shape[0], 512):
        bad += int((dev[r0:r0 + 512] != exp[r0:r0 + 512]).sum())
    assert bad == 0, "%s: %d of %d exported words differ from the oracle" % (what, bad, dev.size)


def test_orientation_zero_changes_neither_launches_nor_words():
    hc.hip()
    w, h = 400, 300
    lut, co = _lut()
    d_lut = lib.DeviceBuffer.from_numpy(0, lut)
    raw = synth.bayer_mosaic(w, h, seed=3)
    for build in (lambda **k: pipe.light_pipe_nodes(w, h, d_lut.ptr, float(lut[0]), co, filmic=filmic.default_data(), **k),
                  lambda **k: pipe.denoise_pipe_nodes(w, h, d_lut.ptr, float(lut[0]), co, filmic=filmic.default_data(),
                                                      with_nlmeans=True, with_bilat=True, **k)):
        base, g0, l0 = _run_pipe(build(), raw, w, h, profile=True)
        zero, g1, l1 = _run_pipe(build(orientation=0), raw, w, h, profile=True)
        assert g0 == g1
        assert l0 == l1 and l0
        assert np.array_equal(base, zero)


@pytest.mark.parametrize("o", range(8))
def test_small_light_pipe_with_every_orientation_equals_the_oracle(o):
    hc.hip()
    w, h = 400, 300
    lut, co = _lut()
    d_lut = lib.DeviceBuffer.from_numpy(0, lut)
    raw = synth.bayer_mosaic(w, h, seed=4)
    ow, oh = params.oriented_size(w, h, o)
    nodes = pipe.light_pipe_nodes(w, h, d_lut.ptr, float(lut[0]), co, filmic=filmic.default_data(), orientation=o)
    dev, groups, _ = _run_pipe(nodes, raw, ow, oh)
    base = pipe.light_pipe_nodes(w, h, d_lut.ptr, float(lut[0]), co, filmic=filmic.default_data())
    _, g0, _ = _run_pipe(base, raw, w, h)
    assert groups == (g0 if o == 0 else g0 + 1)  # one launch group more: the fused runs on either side stay fused
    exp = oracle_chain(pipe.light_pipe_nodes(w, h, lut.ctypes.data, float(lut[0]), co, filmic=filmic.default_data(),
                                             orientation=o), raw)
    _compare(dev, exp, "light pipe %d x %d, orientation %d" % (w, h, o))


def test_small_full_pipe_rotated_equals_the_oracle():
    hc.hip()
    w, h = 640, 400
    lut, co = _lut()
    d_lut = lib.DeviceBuffer.from_numpy(0, lut)
    raw = synth.bayer_mosaic(w, h, seed=6)
    for o in (5, 6):
        ow, oh = params.oriented_size(w, h, o)
        mk = lambda ptr: pipe.denoise_pipe_nodes(w, h, ptr, float(lut[0]), co, filmic=filmic.default_data(),
                                                 with_nlmeans=True, with_bilat=True, orientation=o)
        dev, _, _ = _run_pipe(mk(d_lut.ptr), raw, ow, oh)
        _compare(dev, oracle_chain(mk(lut.ctypes.data), raw), "full pipe %d x %d, orientation %d" % (w, h, o))


def test_band_mode_refuses_a_flip_node():
    import torch
    l = hc.hip()
    w, h = 400, 320
    lut, co = _lut()
    d_lut = torch.from_numpy(lut).to("cuda:0")
    for o in (2, 6):
        nodes = pipe.light_pipe_nodes(w, h, d_lut.data_ptr(), float(lut[0]), co, filmic=filmic.default_data(), orientation=o)
        p = pipe.DevicePipe(0, nodes)
        bands = tiled.plan_bands(w, h, 2)
        d_in = torch.zeros((bands[0].rows, w), dtype=torch.int16, device="cuda:0")
        st = abi.BandState()
        rc = l.dt_hip_pipe_band_begin(p.handle, C.byref(bands[0]), d_in.data_ptr(), C.byref(st))
        assert rc == abi.DT_HIP_INVALID_ARG
        assert "flip" in l.dt_hip_last_error().decode() and "row-band" in l.dt_hip_last_error().decode()
        p.close()
    # orientation 0 is no node: band mode runs
    nodes = pipe.light_pipe_nodes(w, h, d_lut.data_ptr(), float(lut[0]), co, filmic=filmic.default_data(), orientation=0)
    p = pipe.DevicePipe(0, nodes)
    assert l.dt_hip_band_halo_rows(b"flip", C.byref(nodes[3].piece), C.cast(C.byref(abi.FlipData(6)), C.c_void_p), 4) == -1
    p.close()


def test_a_blend_behind_flip_is_refused():
    hc.hip()
    lut, co = _lut()
    nodes = pipe.light_pipe_nodes(64, 48, 0, float(lut[0]), co, filmic=filmic.default_data(), orientation=6)
    k = [n.op for n in nodes].index("flip")
    blend = pipe.Node("blend", abi.BlendData(), nodes[k].piece)
    with pytest.raises(lib.AnselHipError, match="blend"):
        pipe.DevicePipe(0, nodes[:k + 1] + [blend] + nodes[k + 1:])


def test_a_flip_node_whose_consumer_reads_another_format_is_refused():
    """nothing is launched: the consumer would read past the flip's output"""
    l = hc.hip()
    lut, co = _lut()
    nodes = pipe.light_pipe_nodes(64, 48, 0, float(lut[0]), co, filmic=filmic.default_data(), orientation=6)
    k = [n.op for n in nodes].index("flip")
    nodes[k].piece.channels = 1
    p = pipe.DevicePipe(0, nodes)
    d_in = lib.DeviceBuffer(0, 64 * 48 * 2)
    d_out = lib.DeviceBuffer(0, 64 * 48 * 8)
    assert l.dt_hip_pipe_process(p.handle, d_in.ptr, d_out.ptr) == abi.DT_HIP_INVALID_ARG
    assert "channels" in l.dt_hip_last_error().decode()
    p.close()


# ---- at frame size ----------------------------------------------------------------------------------------------------
def _need_host_memory(gib):
    import psutil
    have = psutil.virtual_memory().available / 2.0 ** 30
    if have < gib:
        pytest.skip("the oracle chain of this frame needs ~%d GiB of host memory, %.0f GiB available" % (gib, have))


def _all_cores(n):
    try:
        C.CDLL("libgomp.so.1").omp_set_num_threads(n)
    except OSError:
        pass


def _at_size(which, size, orientations, host_gib):
    import torch
    hc.hip()
    _need_host_memory(host_gib)
    w, h = synth.SIZES[size]
    lut, co = _lut()
    d_lut = torch.from_numpy(lut).to("cuda:0")
    raw = synth.bayer_mosaic_tiled(w, h, seed=2)

    def mk(ptr, o):
        if which == "light":
            return pipe.light_pipe_nodes(w, h, ptr, float(lut[0]), co, filmic=filmic.default_data(), orientation=o)
        return pipe.denoise_pipe_nodes(w, h, ptr, float(lut[0]), co, filmic=filmic.default_data(), diffuse_iterations=2,
                                       with_nlmeans=True, with_bilat=True, orientation=o)

    devs = {}
    d_in = torch.from_numpy(raw.view(np.int16)).to("cuda:0")
    for o in orientations:
        ow, oh = params.oriented_size(w, h, o)
        p = pipe.DevicePipe(0, mk(d_lut.data_ptr(), o), fusion=True)
        d_out = torch.zeros((oh, ow, 4), dtype=torch.int16, device="cuda:0")
        p.process(d_in.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        p.close()
        devs[o] = d_out.cpu().numpy().view(np.uint16)
        del d_out
        assert devs[o].std() > 100
    del d_in
    torch.cuda.empty_cache()
    _all_cores(os.cpu_count() or 1)
    try:
        # the chain up to flip is the same for every orientation: run it once
        nodes = mk(lut.ctypes.data, orientations[0])
        k = [n.op for n in nodes].index("flip")
        t0 = time.time()
        src = raw
        o_lib = ck.oracle()
        for n in nodes[:k]:
            dst = ck.aligned_empty((h, w) if n.op in CFA_OPS else (h, w, 4), np.float32)
            assert ck.call(o_lib, "oracle_" + n.op, n.piece, n.data, np.ascontiguousarray(src), dst) == 0, n.op
            src = dst
        pre = src
        for o in orientations:
            exp = oracle_chain(mk(lut.ctypes.data, o), raw, start=(k, pre))
            _compare(devs.pop(o), exp, "%s pipe %s, orientation %d" % (which, size, o))
            del exp
        print("oracle chains %s %s: %.1f s" % (which, size, time.time() - t0))
    finally:
        if (os.cpu_count() or 1) > 32 and "OMP_NUM_THREADS" not in os.environ:
            _all_cores(32)


def test_full_pipe_24MP_swapping_orientations_equal_the_oracle():
    """orientations 4 - 7: the four that transpose the frame (EXIF 5 - 8, every portrait frame)"""
    _at_size("full", "24MP", [4, 5, 6, 7], host_gib=24)


def test_light_pipe_100MP_orientation_6_equals_the_oracle():
    _at_size("light", "100MP", [6], host_gib=20)
