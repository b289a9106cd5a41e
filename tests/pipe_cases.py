"""TEST INFRASTRUCTURE (not a test): node lists for the executor beyond the two canonical pipes, and their CPU reference.

  * oracle_chain(nodes, src, which)   the CPU reference of an arbitrary node list: per-node geometry, CFA or RGBA input,
                                      blend, flip (numpy), detailmask, the export conversions, the scanline packing, the
                                      encoders (tests/jpeg_ref.py, tests/png_ref.py), or a pipe that ends in float
  * device_modulewise(nodes, src)     the same list through the per-module C-ABI, every buffer sized from its node
  * device_pipe / device_bands / device_bands_c / device_batch   the executor's walks over the list
  * the parameter pools of the module tests (filmic per fused mode, the five adaptations, the conversion flavours, ...)
  * generate(seed)                    a valid node list from a small grammar, its input frame and its tags
  * generate_scaled(seed)             the same for lists whose RGBA part runs at a region scale != 1: a reduced-size export
                                      (mosaic, demosaic, initialscale, modules at its scale) or an RGBA frame at a scale
  * plan_groups / fused_pairs / band_eligible   plain restatements of dt_hip_pipe_t::plan(), of the frame walk's fused
                                      pairs and of the band walk's refusals, over the node list alone

A node list carries pointers (tone curves, the raw detail mask's plane): a list is built twice from the same seed or
case, once over host memory for the oracle and once over device memory -- class Tables."""
import ctypes as C

import numpy as np

import checkers as ck
from ansel_amd import abi, filmic, lib, params, pipe, synth

CFA_OPS = ("rawprepare", "temperature", "highlights")
RUN_OPS = ("exposure", "colorin", "channelmixerrgb", "filmicrgb", "colorout")  # the reference's pipe order
ENCODERS = ("export_jpeg", "export_png")
# modules a "blend" node may follow in a generated list: every RGBA module with blending.  (The three CFA modules are
# left out: the band walk ends its CFA stage at the first node that is none of them.)
BLENDABLE = RUN_OPS + ("denoiseprofile", "diffuse", "nlmeans", "bilat")


def orient(x, o):
    """the flip module as the numpy permutation of its formula (tests/test_gpu_flip.py)"""
    y = x
    if o & 1:
        y = y[::-1]
    if o & 2:
        y = y[:, ::-1]
    if o & 4:
        y = np.swapaxes(y, 0, 1)
    return np.ascontiguousarray(y)


# ---- pointers -------------------------------------------------------------------------------------------------------
class Tables:
    """what the data of a node list points to: the sRGB tone curves and the raw detail mask's plane, in host memory
    (device=False: the oracle's list) or on device 0.  Keep it alive as long as the list."""

    def __init__(self, device=False):
        self.device = device
        self.host = {"enc": params.srgb_encode_lut(), "dec": params.srgb_decode_lut()}
        self.coeffs = {k: params.unbounded_coeffs(v) for k, v in self.host.items()}
        self.dev = {}
        self.planes = {}

    def lut(self, name):
        """(pointer, first sample, fitted power law) of one tone curve, as params.conversion() and LabData.make() take it"""
        t = self.host[name]
        if self.device:
            if name not in self.dev:
                self.dev[name] = lib.DeviceBuffer.from_numpy(0, t)
            return (self.dev[name].ptr, float(t[0]), self.coeffs[name])
        return (t.ctypes.data, float(t[0]), self.coeffs[name])

    def plane(self, key, w, h):
        if key not in self.planes:
            self.planes[key] = lib.DeviceBuffer(0, w * h * 4) if self.device else ck.aligned_empty((h, w), np.float32)
        p = self.planes[key]
        return p.ptr if self.device else p.ctypes.data

    def release(self):
        for b in list(self.dev.values()) + (list(self.planes.values()) if self.device else []):
            b.release()
        self.dev, self.planes = {}, {}


# ---- parameter pools: what the module tests already use ---------------------------------------------------------------
FILMIC = {
    "agx_medium": dict(),
    "agx_extra": dict(version=filmic.AGX_EXTRA, saturation=25.0),
    "v7": dict(version=filmic.V7_2023, saturation=10.0),
    "v6_split": dict(version=filmic.V6_2022, preserve_color=filmic.METHOD_NONE, saturation=10.0),
    "v6_chroma": dict(version=filmic.V6_2022, preserve_color=filmic.METHOD_POWER_NORM, saturation=-15.0),
    "v4": dict(version=filmic.V4_2020, preserve_color=filmic.METHOD_MAX_RGB, saturation=10.0),  # not fused: its own launch
}
# the filmic mode (px_filmicrgb.h) each fused entry of the pool selects
FILMIC_MODE = {"agx_medium": "agx", "agx_extra": "agx", "v7": "v5", "v6_split": "split_v4", "v6_chroma": "chroma_v4"}
ADAPTATIONS = (abi.DT_HIP_ADAPTATION_LINEAR_BRADFORD, abi.DT_HIP_ADAPTATION_CAT16, abi.DT_HIP_ADAPTATION_FULL_BRADFORD,
               abi.DT_HIP_ADAPTATION_XYZ, abi.DT_HIP_ADAPTATION_RGB)
FLAVOURS = ("matrix", "lut_source", "lut_target", "clip_matrix", "blue_mapping")
DIFFUSE = {"lens_deblur_soft": dict(iterations=1), "inpaint_highlights": dict(iterations=2, threshold=0.05)}
BILAT = {"bilateral": lambda: abi.BilatData.bilateral(sigma_s=12.0, sigma_r=25.0, detail=0.33),
         "bilateral_fine": lambda: abi.BilatData.bilateral(sigma_s=7.0, sigma_r=9.0, detail=-0.6),
         "laplacian": lambda: abi.BilatData.local_laplacian()}
EXPOSURE = abi.ExposureData(-0.000244140625, float(np.float32(2.0) ** np.float32(0.7)))


def filmic_data(name, use_output_profile=True):
    return filmic.commit(filmic.UserParams.defaults(**FILMIC[name]), use_output_profile=use_output_profile)


def channelmixer_data(adaptation, clip=True, version=2):
    return params.channelmixerrgb(adaptation=adaptation, version=version, clip=clip, saturation=(0.1, -0.2, 0.05),
                                  lightness=(0.05, 0.0, -0.1))


def conversion_data(op, flavour, tb):
    """colorin (camera -> work) or colorout (work -> sRGB) in one flavour of px_conversion_rt: the plain matrix, tone curves
    on the way in, tone curves on the way out, a clip matrix (with both curves, as test_gpu_color.py builds it), blue mapping"""
    m = params.WORK_OUT @ params.CAMERA_TO_XYZ if op == "colorin" else params.SRGB_OUT @ params.WORK_IN
    if flavour == "matrix":
        return params.conversion(m)
    if flavour == "lut_source":
        return params.conversion(m, lut_source=[tb.lut("dec")] * 3)
    if flavour == "lut_target":
        return params.conversion(m, lut_target=[tb.lut("enc")] * 3)
    if flavour == "clip_matrix":
        return params.conversion(m, clip_matrix=params.SRGB_OUT @ params.WORK_IN, lut_source=[tb.lut("dec")] * 3,
                                 lut_target=[tb.lut("enc")] * 3)
    assert flavour == "blue_mapping", flavour
    return params.conversion(m, blue_mapping=True)


def lab_data(op, tb, nonlinear=False):
    m = params.WORK_IN if op == "rgb_to_lab" else params.WORK_OUT
    if not nonlinear:
        return abi.LabData.make(m)
    return abi.LabData.make(m, [tb.lut("dec" if op == "rgb_to_lab" else "enc")] * 3)


def blend_data(flavour, tb=None, plane=None):
    """uniform and parametric as tests/test_gpu_tiled.py _full_nodes("blended") builds them; "blur" and "details" are the
    parametric mask with a mask blur / a details threshold (neither runs on row bands); the Lab ones for Lab modules"""
    if flavour == "uniform":
        return abi.BlendData.uniform(params.WORK_IN, 60.0, abi.BLEND_MULTIPLY, 0.5)
    if flavour == "lab_uniform":
        return abi.BlendData.uniform(params.WORK_IN, 57.0, abi.BLEND_NORMAL, blend_cst=abi.BLEND_CS_LAB)
    if flavour == "lab_parametric":
        return abi.BlendData.uniform(params.WORK_IN, 85.0, blend_cst=abi.BLEND_CS_LAB).channel(abi.BLENDIF_L_in, 0.1, 0.3, 0.7, 0.9)
    d = abi.BlendData.uniform(params.WORK_IN, 80.0)
    d.channel(abi.BLENDIF_GRAY_in, 0.02, 0.15, 0.6, 0.9, boost=1.0)
    if flavour == "parametric":
        d.channel(abi.BLENDIF_Jz_in, 0.05, 0.2, 1.0, 1.0, boost=-4.0)
        d.channel(abi.BLENDIF_hz_out, 0.1, 0.3, 0.8, 0.95)
        d.contrast, d.brightness = 0.3, -0.2
    elif flavour == "blur":
        d.blur_radius = 3.0
    else:
        assert flavour == "details" and plane, flavour
        d.details = 0.3
        d.detail_mask = plane
    return d


# ---- the CPU reference ----------------------------------------------------------------------------------------------------
def _node_out(n):
    """(shape, dtype) of what one node writes; an encoder: (capacity,) bytes -- the length word, then the file"""
    w, h = n.piece.roi_out.width, n.piece.roi_out.height
    if n.op in ENCODERS:
        return (int(n.data.capacity),), np.uint8
    if n.op == "export_u16":
        return (h, w, 4), np.uint16
    if n.op == "export_u8":
        return (h, w, 4), np.uint8
    if n.op == "export_rows":
        return (h, w, int(n.data.layers)), np.uint8 if n.data.bpp == 8 else np.uint16
    return ((h, w) if n.op in CFA_OPS else (h, w, 4)), np.float32


def out_format(nodes):
    """(shape, dtype) of what the list's last node writes (a blend works in place in its module's output)"""
    k = len(nodes) - 1
    while nodes[k].op == "blend":
        k -= 1
    return _node_out(nodes[k])


def file_of(buf):
    """the file an encoder node left in its output: a little-endian uint64 length, then the bytes"""
    n = int(np.frombuffer(np.ascontiguousarray(buf[:8]).tobytes(), np.uint64)[0])
    assert n != 2 ** 64 - 1 and n + 8 <= len(buf), n
    return np.ascontiguousarray(buf[8:8 + n]).tobytes()


def oracle_chain(nodes, src, which="oracle", tap=None, fill=0.0):
    """The unsplit CPU chain of a node list: what band_engine.whole_frame() and test_gpu_pipe._run_cpu() do for the
    canonical pipes, for any list.  which="ref": the reference's own code wherever oracle/_ref has the function, the
    oracle's elsewhere (flip, the export nodes and the encoders have no _ref function).  Returns what the last node writes;
    behind an encoder that is the file's bytes.  tap(k, node, input, output, before) sees every node's buffers: a blend's
    input is the input of its module, and `before` is a copy of that module's output as the blend found it (None at every
    other node).  fill: what every module's output holds before the module runs -- the words a module leaves alone keep it."""
    o = ck.oracle()
    assert o is not None, "oracle/liboracle.so missing: run build()"
    r = ck.ref() if which == "ref" else None
    assert which == "oracle" or r is not None, "oracle/_ref/libansel_ref.so missing"

    def fn(name):
        if r is not None and hasattr(r, "ref_" + name):
            return r, "ref_" + name
        return o, "oracle_" + name

    cur = np.ascontiguousarray(src)
    prev = None
    for k, n in enumerate(nodes):
        w, h = n.piece.roi_out.width, n.piece.roi_out.height
        inp, before = cur, None
        if n.op == "blend":
            # dt_develop_blend_process(): blend(input of the module, output of the module), in place in the output
            assert prev is not None, "a blend node needs the module it blends in front of it"
            l, name = fn("develop_blend")
            inp = prev
            before = cur.copy() if tap is not None else None
            assert ck.call(l, name, n.piece, n.data, np.ascontiguousarray(prev), cur) == 0, "blend"
            prev = None
        elif n.op == "flip":
            prev, cur = None, orient(cur, n.data.orientation)
            assert cur.shape[:2] == (h, w), (cur.shape, w, h)
        elif n.op in ("export_u16", "export_u8"):
            shape, dtype = _node_out(n)
            out = ck.aligned_empty(shape, dtype)
            l, name = fn(n.op.replace("export_", "export_convert_"))
            getattr(l, name)(w, h, ck.ptr(cur), ck.ptr(out))
            prev, cur = None, out
        elif n.op == "export_rows":
            # the scanlines a format writer hands to its library: `layers` samples per pixel (tiff.c:322-339)
            prev, cur = None, np.ascontiguousarray(cur[..., :int(n.data.layers)])
        elif n.op == "export_jpeg":
            import jpeg_ref as jr
            cur = np.frombuffer(jr.encode(cur, int(n.data.quality), int(n.data.subsampling), 1), np.uint8)
        elif n.op == "export_png":
            import png_ref as pr
            cur = np.frombuffer(pr.host_file(cur, int(n.data.compression_level)), np.uint8)
        else:
            shape, dtype = _node_out(n)
            out = ck.aligned_empty(shape, dtype)
            out[...] = fill
            l, name = fn(n.op)
            assert ck.call(l, name, n.piece, n.data, cur, out) == 0, "%s (node %d) refused by the checker" % (n.op, k)
            prev, cur = cur, out
        if tap is not None:
            tap(k, n, inp, cur, before)
    return cur


# ---- the device walks ---------------------------------------------------------------------------------------------------
def allocated():
    """bytes the runtime's pool has handed out on device 0"""
    l = lib.load()
    assert l.dt_hip_finish(0) == 1, l.dt_hip_last_error()
    cur, peak = C.c_size_t(0), C.c_size_t(0)
    l.dt_hip_memory_statistics(0, C.byref(cur), C.byref(peak))
    return cur.value


def _result(buf, nodes):
    shape, dtype = out_format(nodes)
    out = buf.to_numpy(shape, dtype)
    return np.frombuffer(file_of(out), np.uint8) if nodes[-1].op in ENCODERS else out


def device_modulewise(nodes, src):
    """every node through its own C-ABI entry point (pipe.run_nodes() for the modules, the export entry points for the
    rest), each buffer sized from its node's region and output format; a blend works in place in its module's output"""
    l = lib.load()
    bufs = [lib.DeviceBuffer.from_numpy(0, src)]
    try:
        cur, prev = bufs[0], None
        for n in nodes:
            w, h = n.piece.roi_out.width, n.piece.roi_out.height
            if n.op == "blend":
                assert prev is not None
                lib.check(l.dt_hip_develop_blend_process(0, C.byref(n.piece), C.byref(n.data), prev.ptr, cur.ptr), "blend")
                prev = None
                continue
            shape, dtype = _node_out(n)
            if n.op == "demosaic" or (n.op == "bilat" and n.data.mode == abi.DT_HIP_BILAT_LOCAL_LAPLACIAN):
                # the fourth channel these two leave alone is the caller's: zeros, as oracle_chain(fill=0.0) has them
                out = lib.DeviceBuffer.from_numpy(0, np.zeros(shape, dtype))
            else:  # every word is the module's to write: whatever the pool holds (poison under hc.pool_fill())
                out = lib.DeviceBuffer(0, int(np.prod(shape)) * np.dtype(dtype).itemsize)
            bufs.append(out)
            if n.op == "export_u8":
                lib.check(l.dt_hip_export_convert_u8(0, w, h, cur.ptr, out.ptr), n.op)
            elif n.op == "export_rows":
                lib.check(l.dt_hip_export_pack_rows(0, w, h, n.data.bpp, n.data.layers, cur.ptr, out.ptr), n.op)
            elif n.op in ENCODERS:
                lib.check(getattr(l, "dt_hip_" + n.op)(0, w, h, C.byref(n.data), cur.ptr, out.ptr), n.op)
            else:
                pipe.run_nodes(0, [n], [cur.ptr, out.ptr])
            prev, cur = cur, out
        assert l.dt_hip_finish(0) == 1, l.dt_hip_last_error()
        return _result(cur, nodes)
    finally:
        for b in bufs:
            b.release()


def _out_bytes(nodes):
    shape, dtype = out_format(nodes)
    return int(np.prod(shape)) * np.dtype(dtype).itemsize


def device_pipe(nodes, src, fusion):
    """dt_hip_pipe_process(): (result, number of launch groups)"""
    l = lib.load()
    din, dout = lib.DeviceBuffer.from_numpy(0, src), lib.DeviceBuffer(0, _out_bytes(nodes))
    p = None
    try:
        p = pipe.DevicePipe(0, nodes, fusion=fusion)
        groups = p.num_groups
        p.process(din.ptr, dout.ptr)
        assert l.dt_hip_finish(0) == 1, l.dt_hip_last_error()
        return _result(dout, nodes), groups
    finally:
        if p is not None:
            p.close()
        din.release()
        dout.release()


def launch_tags(nodes, src):
    """{tag: launches} of one dt_hip_pipe_process() with fusion on, from the runtime's launch profile (as
    tests/test_gpu_flip.py counts launches): what the walk really launched, which the number of groups does not show"""
    l = lib.load()
    din, dout = lib.DeviceBuffer.from_numpy(0, src), lib.DeviceBuffer(0, _out_bytes(nodes))
    p = None
    try:
        p = pipe.DevicePipe(0, nodes, fusion=True)
        l.dt_hip_events_reset(0)
        l.dt_hip_events_enable(0, 1)
        try:
            p.process(din.ptr, dout.ptr)
            assert l.dt_hip_finish(0) == 1, l.dt_hip_last_error()
            l.dt_hip_events_wait_for(0)
            tags, ms, cnt = (C.c_char_p * 64)(), (C.c_float * 64)(), (C.c_int * 64)()
            n = l.dt_hip_events_profiling(0, tags, ms, cnt, 64)
            return {tags[i].decode(): int(cnt[i]) for i in range(n)}
        finally:
            l.dt_hip_events_enable(0, 0)
            l.dt_hip_events_reset(0)
    finally:
        if p is not None:
            p.close()
        din.release()
        dout.release()


def _band_buffers(nodes, src, bands):
    import torch
    shape, dtype = out_format(nodes)
    row_words = int(np.prod(shape[1:])) * np.dtype(dtype).itemsize
    ins = [torch.from_numpy(np.ascontiguousarray(src[b.row0:b.row0 + b.rows]).view(np.uint8).reshape(-1)).to("cuda:0") for b in bands]
    outs = [torch.zeros((b.rows * row_words,), dtype=torch.uint8, device="cuda:0") for b in bands]
    return torch, ins, outs, shape, dtype


def _bands_result(torch, outs, shape, dtype):
    torch.cuda.synchronize()
    return np.concatenate([t.cpu().numpy() for t in outs]).view(dtype).reshape(shape)


def device_bands(nodes, src, n):
    """the band walk driven from Python, all bands in lockstep on the one device (tiled.process_bands_locally)"""
    from ansel_amd import tiled
    w, h = nodes[0].piece.roi_out.width, nodes[0].piece.roi_out.height
    bands = tiled.plan_bands(w, h, n, tiled.pipe_demosaic_method(nodes))
    torch, ins, outs, shape, dtype = _band_buffers(nodes, src, bands)
    p = pipe.DevicePipe(0, nodes, fusion=True)
    try:
        engine = tiled.HipBandEngine(p, "cuda:0")
        tiled.process_bands_locally(engine, bands, [t.data_ptr() for t in ins], [t.data_ptr() for t in outs], w)
        return _bands_result(torch, outs, shape, dtype)
    finally:
        torch.cuda.synchronize()
        p.close()


def device_bands_c(nodes, src, n):
    """dt_hip_pipe_process_bands(): the band walk driven from inside the library, a host thread per band"""
    from ansel_amd import tiled
    l = lib.load()
    w, h = nodes[0].piece.roi_out.width, nodes[0].piece.roi_out.height
    bands = tiled.plan_bands(w, h, n, tiled.pipe_demosaic_method(nodes))
    torch, ins, outs, shape, dtype = _band_buffers(nodes, src, bands)
    pipes = [pipe.DevicePipe(0, nodes, fusion=True) for _ in range(n)]
    try:
        torch.cuda.synchronize()
        rc = l.dt_hip_pipe_process_bands((C.c_void_p * n)(*[p.handle for p in pipes]), n, (abi.Band * n)(*bands),
                                         (C.c_void_p * n)(*[t.data_ptr() for t in ins]),
                                         (C.c_void_p * n)(*[t.data_ptr() for t in outs]))
        lib.check(rc, "dt_hip_pipe_process_bands")
        return _bands_result(torch, outs, shape, dtype)
    finally:
        torch.cuda.synchronize()
        for p in pipes:
            p.close()


def device_batch(nodes, src, depth=2, frames=3):
    """dt_hip_batch_*: `frames` copies of the frame through a batch of `depth` slots; one result per frame"""
    l = lib.load()
    src = np.ascontiguousarray(src)
    nb_in, nb_out = src.nbytes, _out_bytes(nodes)
    shape, dtype = out_format(nodes)
    pins, p, b = [], None, None
    try:
        p = pipe.DevicePipe(0, nodes, fusion=True)
        for _ in range(2 * frames):
            q = l.dt_hip_alloc_host_pinned(nb_in if len(pins) < frames else nb_out)
            assert q, l.dt_hip_last_error()
            pins.append(q)
        pin_in, pin_out = pins[:frames], pins[frames:]
        for q in pin_in:
            C.memmove(q, src.ctypes.data, nb_in)
        b = l.dt_hip_batch_new(p.handle, depth, nb_in, nb_out)
        assert b, l.dt_hip_last_error()
        for k in range(frames):
            s = l.dt_hip_batch_submit(b, pin_in[k], pin_out[k])
            assert s == k % depth, (s, l.dt_hip_last_error())
        lib.check(l.dt_hip_batch_drain(b), "dt_hip_batch_drain")
        res = []
        for q in pin_out:
            a = np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_uint8)), shape=(nb_out,)).copy().view(dtype).reshape(shape)
            res.append(np.frombuffer(file_of(a), np.uint8) if nodes[-1].op in ENCODERS else a)
        return res
    finally:
        if b:
            l.dt_hip_batch_free(b)
        for q in pins:
            l.dt_hip_free_host_pinned(q)
        if p is not None:
            p.close()


def count_differing(a, b):
    """words that differ: floats by bit pattern (NaN payloads and the sign of zero included), as the module tests compare"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1
    if a.dtype == np.float32:
        return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())
    return int((a != b).sum())


# ---- restatements over the node list ------------------------------------------------------------------------------------------
def kept(nodes):
    """the list as the executor holds it: a flip of orientation 0 is the identity and no node (dt_hip_pipe_add_node())"""
    return [n for n in nodes if not (n.op == "flip" and n.data.orientation == 0)]


def _geometry(n):
    return (n.piece.roi_out.width, n.piece.roi_out.height)


def _roundf(v):
    """roundf(): halves away from zero (Python's round() takes them to the even neighbour)"""
    return int(np.copysign(np.floor(abs(v) + 0.5), v))


def _raw_group_supported(trio):
    p = trio[0].piece
    if not (p.filters and p.filters != 9 and p.channels == 1):
        return False
    w, d = p.roi_out.width, trio[0].data
    if w <= 0 or w % 4 or p.roi_in.width % 4 or _roundf(float(np.float32(d.x * p.roi_in.scale))) % 4:
        return False
    for n in trio[1:]:
        if not n.piece.filters or n.piece.filters == 9 or _geometry(n) != _geometry(trio[0]):
            return False
        if n.op == "highlights" and n.data.mode != abi.DT_HIP_HIGHLIGHTS_CLIP:
            return False
    return True


def plan_groups(nodes, fusion=True):
    """dt_hip_pipe_t::plan() restated: [(kind, first, count)] with kind "single", "raw" or "rgb" """
    nodes = kept(nodes)
    n = len(nodes)
    ops = [x.op for x in nodes]

    def blended(k):
        return k + 1 < n and ops[k + 1] == "blend"

    def linear_glue(k, op):
        return k < n and ops[k] == op and nodes[k].piece.channels == 4 and not nodes[k].data.nonlinearlut

    out, i = [], 0
    while i < n:
        kind, count = "single", 1
        if fusion and ops[i] == "rawprepare" and not blended(i) and not blended(i + 1) and not blended(i + 2):
            j = i + 1
            if j < n and ops[j] == "temperature":
                j += 1
            if j < n and ops[j] == "highlights":
                j += 1
            if j - i > 1 and _raw_group_supported(nodes[i:j]):
                kind, count = "raw", j - i
        elif fusion and nodes[i].piece.channels == 4 and not blended(i) and (
                ops[i] in RUN_OPS or (linear_glue(i, "lab_to_rgb") and i + 1 < n and ops[i + 1] in RUN_OPS)):
            geo = _geometry(nodes[i])
            j = i + 1 if ops[i] == "lab_to_rgb" else i
            last, stages = -1, 0
            while j < n:
                nd = nodes[j]
                if nd.op not in RUN_OPS or RUN_OPS.index(nd.op) <= last or blended(j):
                    break
                if _geometry(nd) != geo or nd.piece.channels != 4:
                    break
                if nd.op == "filmicrgb" and not 3 <= nd.data.version <= 9:
                    break
                if nd.op == "channelmixerrgb" and nd.data.adaptation > abi.DT_HIP_ADAPTATION_RGB:
                    break
                last = RUN_OPS.index(nd.op)
                stages += 1
                j += 1
            if j < n and ops[j] == "export_u16" and _geometry(nodes[j]) == geo:
                j += 1
                if (j < n and ops[j] == "export_rows" and nodes[j].data.bpp == 16 and nodes[j].data.layers == 3
                        and _geometry(nodes[j]) == geo):
                    j += 1
            elif stages > 0 and linear_glue(j, "rgb_to_lab") and not blended(j) and _geometry(nodes[j]) == geo:
                j += 1
            if j - i > 1 and stages > 0:
                kind, count = "rgb", j - i
        out.append((kind, i, count))
        i += count
    return out


def fused_pairs(nodes):
    """the four pairs the frame walk (dt_hip_pipe_process()) runs in one launch, by the rules its fallbacks state"""
    nodes = kept(nodes)
    groups = plan_groups(nodes)
    found = set()

    def is_blend(g):
        return g < len(groups) and nodes[groups[g][1]].op == "blend"

    for g, (kind, first, count) in enumerate(groups):
        if kind != "single" or g + 1 >= len(groups):
            continue
        nd = nodes[first]
        nkind, nfirst, ncount = groups[g + 1]
        run = nodes[nfirst:nfirst + ncount]
        tail = run[-1]
        if nd.op == "nlmeans" and nkind == "single" and tail.op == "bilat" and tail.data.mode == 0 and _geometry(tail) == _geometry(nd):
            found.add("nlmeans>bilat")
        if is_blend(g + 2):
            continue
        if nd.op == "denoiseprofile" and nkind == "rgb":
            # denoiseprofile.hip: the wavelets' last kernel takes a run without filmic that starts at RGB and ends in float
            ok = nd.data.mode in (abi.DT_HIP_DENOISEPROFILE_WAVELETS, abi.DT_HIP_DENOISEPROFILE_WAVELETS_AUTO)
            ok = ok and run[0].op != "lab_to_rgb" and tail.op not in ("export_u16", "export_rows")
            if ok and not any(x.op == "filmicrgb" for x in run) and _geometry(run[0]) == _geometry(nd):
                found.add("denoiseprofile+run")
        if nd.op == "bilat" and nkind == "rgb" and nd.data.mode == 0 and _geometry(run[0]) == _geometry(nd):
            found.add("bilat+run")
        if nd.op == "diffuse" and nkind == "single" and tail.op == "rgb_to_lab" and not tail.data.nonlinearlut:
            found.add("diffuse+rgb_to_lab")
    return found


RCD_TV, RCD_HALO = 94, 9      # rcd.c:70-76: tile pitch, border
AMZ_TV, AMZ_HALO, AMZ_TS = 128, 16, 160  # amaze.cc:181-350: rows a tile keeps, rows it reads beyond them, tile size


def _amaze_tile_on_chip(width, height, top, left):
    """amz::stream_tile_ok(): the tiles the on-chip AMaZE kernel takes -- the only one that walks a band"""
    bottom, right = min(top + AMZ_TS, height + 16), min(left + AMZ_TS, width + 16)
    rrmax = height - top if bottom > height else bottom - top
    ccmax = width - left if right > width else right - left
    if (rrmax < bottom - top and rrmax > AMZ_TS - 16) or (ccmax < right - left and ccmax > AMZ_TS - 16):
        return False
    return not (right - left < AMZ_TS and ((right - left) & 1))


def band_tile_rows(width, height, method):
    """rows of tiles dt_hip_plan_bands() can hand out for this frame and demosaic; 0: no band mode"""
    if method == abi.DT_HIP_DEMOSAIC_RCD:
        return 1 + (height - 2 * RCD_HALO - 1) // RCD_TV if min(width, height) >= 16 else 0
    if method == abi.DT_HIP_DEMOSAIC_AMAZE:
        if min(width, height) < 34:
            return 0
        rows = (height + AMZ_TV - 1) // AMZ_TV
        for ty in range(rows):
            for tx in range((width + AMZ_HALO + AMZ_TV - 1) // AMZ_TV):
                if not _amaze_tile_on_chip(width, height, -AMZ_HALO + ty * AMZ_TV, -AMZ_HALO + tx * AMZ_TV):
                    return 0
        return rows
    return height // 2 if method == -1 else 0  # no demosaic: even row pairs; PPG and the other methods: none


def band_rows(width, height, method, n_bands):
    """[(first row, rows)] of the bands dt_hip_plan_bands() cuts: whole tile rows of the demosaic, or even row pairs"""
    out = []
    tiles = band_tile_rows(width, height, method)
    for k in range(n_bands):
        t0, t1 = k * tiles // n_bands, (k + 1) * tiles // n_bands
        if method == abi.DT_HIP_DEMOSAIC_RCD:
            r0, r1 = (t0 * RCD_TV + RCD_HALO if t0 else 0), (t1 * RCD_TV + RCD_HALO if t1 < tiles else height)
        elif method == abi.DT_HIP_DEMOSAIC_AMAZE:
            r0, r1 = t0 * AMZ_TV, (t1 * AMZ_TV if t1 < tiles else height)
        else:
            r0, r1 = 2 * t0, (2 * t1 if k + 1 < n_bands else height)
        out.append((r0, r1 - r0))
    return out


def stencil_halo_bound(n):
    """rows of either neighbour a stencil module of the pools reads at most AT REGION SCALE 1, on the frames of this file
    (the exact count is dt_hip_band_halo_rows(); tests/test_pipe_cases.py holds it against this bound): the wavelets' and
    the non-local means' below 80, diffuse-or-sharpen below 93 an iteration.  At another scale the patch offsets, the
    search radius and the PDE's zoom move these figures (non-local means at scale 2 reads 96 rows and more): the scaled
    lists of generate_scaled() take the exact count, exact_halo().  The bound makes band_eligible() conservative, never
    wrong: a list it keeps off the bands (diffuse with two iterations on three bands of these frames, say) only loses that
    walk, and one it admits is checked against the exact halo on the CPU."""
    if n.op == "diffuse":
        return 93 * max(int(n.data.iterations), 1)
    if n.op == "nlmeans" or (n.op == "denoiseprofile" and n.data.mode in (abi.DT_HIP_DENOISEPROFILE_NLMEANS, abi.DT_HIP_DENOISEPROFILE_NLMEANS_AUTO)):
        return 80
    return 4 if n.op == "denoiseprofile" else 0


def exact_halo(n):
    """dt_hip_band_halo_rows() itself (a host function of the library: no GPU): the rows a node takes from either neighbour
    at its own region scale; a module that only copies its frame through (the wavelets on a frame too small) takes none"""
    if n.data is None or n.op == "blend":
        return 0
    return max(int(lib.load().dt_hip_band_halo_rows(n.op.encode(), C.byref(n.piece), C.cast(C.byref(n.data), C.c_void_p), C.sizeof(n.data))), 0)


def band_eligible(nodes, n_bands, halo_of=None):
    """the rules check_band_mode() and dt_hip_plan_bands() state (pipe_bands.cpp), over the node list alone -- and the one
    both band drivers state when they meet it ("a band owns fewer rows than the halo its neighbour needs: use fewer
    bands"): the halo rows of a stencil module come out of the neighbour's own rows.  halo_of: stencil_halo_bound (the
    lists at scale 1) or exact_halo (the scaled ones)"""
    halo_of = halo_of if halo_of is not None else stencil_halo_bound
    nodes = kept(nodes)
    w, h = _geometry(nodes[0])
    method = -1
    for n in nodes:
        if n.op == "demosaic":
            method = int(n.data.demosaicing_method)
    if band_tile_rows(w, h, method) < n_bands:
        return False
    rows = band_rows(w, h, method, n_bands)
    for n in nodes:
        halo = halo_of(n)
        for k, (r0, nr) in enumerate(rows):
            if (k and min(halo, r0) > rows[k - 1][1]) or (k + 1 < n_bands and min(halo, h - r0 - nr) > rows[k + 1][1]):
                return False
    for n in nodes:
        if _geometry(n) != (w, h):
            return False
        if n.op in ENCODERS + ("flip", "finalscale", "initialscale", "detailmask"):
            return False
        if n.op == "bilat" and n.data.mode != 0:
            return False
        if n.op == "blend":
            d = n.data
            parametric = bool(d.mask_mode & abi.MASK_PARAMETRIC)
            if (d.mask_mode & abi.MASK_ENABLED) and d.details != 0.0 and d.detail_mask and (parametric or d.form_mask):
                return False
            if d.feathering_radius > 0.1 or d.blur_radius > 0.0:
                return False
    return True


# ---- the figures of a non-local-means launch at a region scale, restated ------------------------------------------------------
def _scatter(scale, scattering, i1, i2):
    """scatter(), nlmeans_core.c:95-105: the scale a float, the rest binary64"""
    a1, a2 = abs(i1), abs(i2)
    return int(float(np.float32(scale)) * ((a1 * a1 * a1 + 7.0 * a1 * np.sqrt(a2)) * ((i1 > 0) - (i1 < 0)) * scattering / 6.0 + i1))


def nlmeans_figures(radius, scale):
    """denoise (non-local means), process_cpu() nlmeans.c:416-457: (patch radius P, offsets, reach = P + 1 + the largest shift)"""
    s = np.float32(min(scale, 2.0))
    P, K = int(np.ceil(np.float32(radius) * s)), int(np.ceil(np.float32(7.0) * s))
    return P, (2 * K + 1) ** 2, P + 1 + _scatter(s, 0.0, K, 0)


def dn_nlmeans_figures(d, scale):
    """denoise (profiled), non-local-means mode, denoiseprofile.c:1599-1648 and :1476-1500: (P, K, reach, the scattering derived
    from the scale -- it keeps the reach the user's values had at scale 1)"""
    s = np.float32(min(min(scale, 2.0), 1.0))
    K = int(d.nbhood)
    P = int(np.ceil(np.float32(d.radius) * s))
    maxk = int((K * K * K + 7.0 * K * np.sqrt(K)) * float(d.scattering) / 6.0 + K)
    K = int(max(np.float32(min(K, 4)), np.float32(K) * s))
    scattering = float(np.float32((maxk - K) * 6.0 / (K * K * K + 7.0 * K * np.sqrt(K))))
    shift = max(abs(_scatter(s, scattering, i, j)) for i in range(-K, K + 1) for j in range(-K, K + 1))
    return P, K, P + 1 + shift, scattering


# ---- the generator ------------------------------------------------------------------------------------------------------
# small, awkward frames: no pixel count is a multiple of 256, some widths are not a multiple of 4; the tall ones give three
# bands a tile row each (RCD: 94 rows a tile, AMaZE: 128); stencil pipes stay below 120 kpixels
RAW_FRAMES = ((244, 478), (248, 470), (252, 323), (202, 430), (130, 390), (318, 150), (203, 431))
TALL_RAW_FRAMES = 5  # the first five give RCD and AMaZE three tile rows
RGBA_FRAMES = ((243, 401), (200, 333), (322, 215), (127, 93))
DEMOSAICS = (abi.DT_HIP_DEMOSAIC_RCD, abi.DT_HIP_DEMOSAIC_RCD, abi.DT_HIP_DEMOSAIC_RCD, abi.DT_HIP_DEMOSAIC_AMAZE,
             abi.DT_HIP_DEMOSAIC_PPG)
ENDINGS = ("float", "u16", "u16_rows", "u8", "jpeg", "png8", "png16")
FRAME_ENDINGS = 4  # the first four end in a frame, the others in a file


class _Builder:
    def __init__(self, rng, tb, w, h):
        self.rng, self.tb, self.w, self.h = rng, tb, w, h
        self.nodes = []
        self.pm = (1.0, 1.0, 1.0, 1.0)
        self.plane = None  # the raw detail mask's plane, while the frame keeps the geometry it was written in
        self.stencils = 0
        self.plain = False  # leave out what has no row-band implementation
        self.scale = 1.0  # the scale of both regions of every piece made from here on (generate_scaled())

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def chance(self, p):
        return bool(self.rng.random() < p)

    def rgb(self):
        if self.scale == 1.0:
            return abi.Piece.make(self.w, self.h, channels=4, processed_maximum=self.pm)
        return abi.Piece.make(self.w, self.h, channels=4, processed_maximum=self.pm, roi_in=abi.Roi.make(0, 0, self.w, self.h, self.scale),
                              roi_out=abi.Roi.make(0, 0, self.w, self.h, self.scale))

    def add(self, op, data, piece=None):
        self.nodes.append(pipe.Node(op, data, piece if piece is not None else self.rgb()))

    def module(self, op, lab=False):
        """one RGBA module with parameters from the pools, and sometimes its blend"""
        tb = self.tb
        if op == "exposure":
            data = abi.ExposureData(self.pick((-0.000244140625, 0.01)), self.pick((1.6245047, 0.8)))
        elif op in ("colorin", "colorout"):
            data = conversion_data(op, self.pick(FLAVOURS), tb)
        elif op == "channelmixerrgb":
            data = channelmixer_data(self.pick(ADAPTATIONS), clip=self.chance(0.5), version=self.pick((0, 1, 2)))
        elif op == "filmicrgb":
            data = filmic_data(self.pick(tuple(FILMIC)), use_output_profile=self.chance(0.5))
        elif op == "denoiseprofile":
            mode = self.pick((abi.DT_HIP_DENOISEPROFILE_WAVELETS, abi.DT_HIP_DENOISEPROFILE_WAVELETS, abi.DT_HIP_DENOISEPROFILE_NLMEANS))
            data = params.denoiseprofile(mode=mode)
        elif op == "diffuse":
            name = self.pick(tuple(DIFFUSE))
            data = params.diffuse(name, **DIFFUSE[name])
        elif op == "nlmeans":
            data = abi.NlmeansData(float(self.pick((1, 2))), 50.0, 0.5, 1.0)
        else:
            assert op == "bilat", op
            data = BILAT[self.pick(("bilateral", "bilateral_fine") + (() if self.plain else ("laplacian",)))]()
        if op in ("denoiseprofile", "diffuse", "nlmeans", "bilat"):
            self.stencils += 1
        self.add(op, data)
        if self.chance(0.12):
            if lab:
                flavour = self.pick(("lab_uniform", "lab_parametric"))
            else:
                flavour = self.pick(("uniform", "parametric") + (() if self.plain else ("blur",))
                                    + (("details", "details") if self.plane else ()))
            self.add("blend", blend_data(flavour, tb, self.plane))

    def flip(self):
        o = int(self.rng.integers(0, 8))
        ow, oh = params.oriented_size(self.w, self.h, o)
        self.add("flip", params.flip(o), abi.Piece.make(self.w, self.h, channels=4, processed_maximum=self.pm,
                                                         roi_out=abi.Roi.make(0, 0, ow, oh)))
        self.w, self.h = ow, oh
        self.plane = None


def generate(seed, tables=None):
    """(nodes, src, tags) of one generated pipe.  The grammar:

        pipe  := [raw] rgba end
        raw   := any subset of rawprepare temperature highlights, in that order, then demosaic   (u16 or f32 mosaic in)
        rgba  := [detailmask] item { [flip] item } [finalscale]
        item  := a pointwise module | pointwise modules in pipe order | pointwise modules in any order
                 | denoiseprofile | diffuse | rgb_to_lab (nlmeans | bilat)+ lab_to_rgb
        end   := float | export_u16 [export_rows | export_png] | export_u8 [export_jpeg | export_png]

    with a blend behind any of the modules of BLENDABLE, and the placement rules of dt_hip_pipe_t::plan() and
    dt_hip_pipe_add_node(): an encoder last behind its export node, flip between nodes of the same channel count, no
    blend behind flip, no blend without its module.  The same seed gives the same list over any Tables.
    tags: "bands" / "batch" (the walks the list is eligible for, by band_eligible()), "start", "end", "tables"."""
    tb = tables if tables is not None else Tables(False)
    rng = np.random.default_rng(1000 + seed)
    start = ("raw_u16", "raw_f32", "rgba_scene", "rgba_adversarial", "raw_u16", "rgba_scene")[int(rng.integers(0, 6))]
    # six lists in ten are drawn without the nodes and frames that have no row-band implementation (which walks a list
    # is eligible for is decided from the finished list, by band_eligible())
    plain = bool(rng.random() < 0.6)
    if start.startswith("raw"):
        w, h = RAW_FRAMES[int(rng.integers(0, TALL_RAW_FRAMES if plain else len(RAW_FRAMES)))]
    else:
        w, h = RGBA_FRAMES[int(rng.integers(0, len(RGBA_FRAMES)))]
    assert (w * h) % 256, (w, h)
    b = _Builder(rng, tb, w, h)
    b.plain = plain

    # ---- the mosaic part
    if start.startswith("raw"):
        mosaic = synth.bayer_mosaic(w, h, seed=seed)
        trio = int(rng.integers(0, 8)) if start == "raw_f32" else 1 | (int(rng.integers(0, 4)) << 1)
        u16 = start == "raw_u16"
        rng_f = float(synth.WHITE - synth.BLACK)
        if trio & 1:
            src = mosaic if u16 else mosaic.astype(np.float32)
            b.add("rawprepare", abi.RawprepareData(0, 0, 0, 0, abi.f4(*[synth.BLACK] * 4), abi.f4(*[rng_f] * 4)),
                  abi.Piece.make(w, h, filters=synth.FILTERS_RGGB, channels=1,
                                 datatype=abi.DT_HIP_TYPE_UINT16 if u16 else abi.DT_HIP_TYPE_FLOAT))
        else:
            src = ((mosaic.astype(np.float32) - np.float32(synth.BLACK)) / np.float32(rng_f)).astype(np.float32)
        if trio & 2:
            b.add("temperature", abi.TemperatureData(abi.f4(*synth.WB_COEFFS)),
                  abi.Piece.make(w, h, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=b.pm))
            b.pm = synth.WB_COEFFS
        cfa = abi.Piece.make(w, h, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=b.pm)
        if trio & 4:
            b.add("highlights", abi.HighlightsData(abi.DT_HIP_HIGHLIGHTS_CLIP, 1.0), cfa)
        b.add("demosaic", abi.DemosaicData(0, 0, DEMOSAICS[int(rng.integers(0, len(DEMOSAICS) - (1 if plain else 0)))], 0.0), cfa)
    elif start == "rgba_scene":
        src = synth.rgba_image(w, h, seed=seed, lo=-0.05, hi=1.6)
    else:
        src = synth.adversarial_rgba(w, h, seed=seed)

    # ---- the RGBA part
    if not plain and b.chance(0.3):
        b.plane = tb.plane("detail", w, h)
        b.add("detailmask", abi.DetailmaskData.make((2.0, 1.0, 1.5), b.plane))
    # NaN and Inf through a stencil module poison the frame (the wavelets' thresholds are frame-wide sums): the adversarial
    # frame goes through pointwise pipes, as in the module tests
    stencils_allowed = 0 if start == "rgba_adversarial" else 3
    force = None
    for k in range(int(rng.integers(1, 5))):
        if k and not plain and b.chance(0.25):
            b.flip()
        kinds = ["point", "ordered", "ordered", "shuffled", "denoiseprofile", "diffuse", "lab"]
        kind = force if force else kinds[int(rng.integers(0, len(kinds)))]
        force = None
        if kind in ("denoiseprofile", "diffuse", "lab") and b.stencils >= stencils_allowed:
            kind = "ordered"
        if kind == "point":
            b.module(b.pick(RUN_OPS))
        elif kind in ("ordered", "ordered_without_filmic", "shuffled"):
            ops = [op for op in RUN_OPS if b.chance(0.6) and not (op == "filmicrgb" and kind == "ordered_without_filmic")] or ["exposure"]
            if kind == "shuffled":
                ops = [ops[i] for i in rng.permutation(len(ops))] + ([b.pick(RUN_OPS)] if b.chance(0.4) else [])
            for op in ops:
                b.module(op)
        elif kind == "lab":
            nonlinear = b.chance(0.2)
            b.add("rgb_to_lab", lab_data("rgb_to_lab", tb, nonlinear))
            for op in b.pick((("nlmeans",), ("bilat",), ("nlmeans", "bilat"), ("nlmeans", "bilat"), ("bilat", "nlmeans"))):
                b.module(op, lab=True)
            b.add("lab_to_rgb", lab_data("lab_to_rgb", tb, nonlinear))
            if b.chance(0.6):
                force = "ordered"
        else:
            b.module(kind)
            if b.chance(0.55):
                force = "ordered_without_filmic" if kind == "denoiseprofile" else "lab"
    if not plain and b.chance(0.25):
        scale = b.pick((0.5, 0.37, 0.81))
        ow, oh = max(int(round(b.w * scale)), 1), max(int(round(b.h * scale)), 1)
        b.add("finalscale", abi.FinalscaleData(int(rng.integers(0, 3))),
              abi.Piece.make(ow, oh, roi_in=abi.Roi.make(0, 0, b.w, b.h, 1.0), roi_out=abi.Roi.make(0, 0, ow, oh, scale)))
        b.w, b.h = ow, oh

    # ---- the end
    end = ENDINGS[int(rng.integers(0, FRAME_ENDINGS if plain else len(ENDINGS)))]
    if end in ("u16", "u16_rows", "png16"):
        b.add("export_u16", None)
    elif end != "float":
        b.add("export_u8", None)
    if end == "u16_rows":
        b.add("export_rows", abi.ExportRowsData(16, 3))
    elif end == "jpeg":
        jd = params.jpeg(b.pick((85, 92, 95)))
        jd.capacity = pipe.jpeg_bound(b.w, b.h, jd)
        b.add("export_jpeg", jd, abi.Piece.make(b.w, b.h, channels=4))
    elif end in ("png8", "png16"):
        pd = params.png(bpp=8 if end == "png8" else 16, compression=b.pick((1, 5, 9)))
        pd.capacity = pipe.png_bound(b.w, b.h, pd)
        b.add("export_png", pd, abi.Piece.make(b.w, b.h, channels=4))
    tags = {"bands": band_eligible(b.nodes, 2) and band_eligible(b.nodes, 3), "batch": True, "start": start, "end": end, "tables": tb}
    return b.nodes, np.ascontiguousarray(src), tags


# ---- lists at a region scale != 1 ----------------------------------------------------------------------------------------
EXPORT_SCALES = (0.37, 0.5, 0.81)  # a reduced-size export: initialscale behind the demosaic, the RGBA modules at its scale
RGBA_SCALES = (0.5, 2.0)           # an RGBA frame whose regions carry the scale: no resampler, the list stays band-eligible
SCALED_STENCILS = ("nlmeans", "diffuse", "denoiseprofile", "bilat")
SCALED_SEEDS = tuple(range(1, 25))
# The demosaic leaves the fourth channel to its caller, as the reference does: RCD on its border ring, AMaZE on the whole frame
# (rcd.c:96-127, amaze.cc); the local laplacian leaves it alone too.  The resampler, the Lab conversions, exposure,
# channelmixerrgb, filmic v4, diffuse and the bilateral grid carry or filter what they find there, and non-local means gives NaN
# for NaN.  These write a value of their own whatever they find (the executor holds the same rule for the buffers it owns,
# dt_hip_pipe_t::leaves_unwritten_alpha() in csrc/pipe_internal.h: change the two together):
SETS_ALPHA = ("colorin", "colorout", "denoiseprofile")


def alpha_is_written(nodes):
    """the last words of the list are a function of its input: behind the last module that leaves the fourth channel of its
    output unwritten comes one that writes it, or an ending that drops it.  Otherwise they are whatever the buffers held, on
    the host and on the device (tests/test_pipe_cases.py holds the scaled lists to this with the oracle's buffers full of NaN)"""
    written = True
    for n in nodes:
        if n.op == "demosaic" or (n.op == "bilat" and n.data.mode == abi.DT_HIP_BILAT_LOCAL_LAPLACIAN):
            written = False
        elif n.op in SETS_ALPHA or (n.op == "export_rows" and n.data.layers == 3):
            written = True
    return written


def generate_scaled(seed, tables=None):
    """(nodes, src, tags) of one pipe whose RGBA part runs at a region scale != 1, in one of two shapes:

        export := [rawprepare] [temperature] [highlights] demosaic initialscale(s) item+ end       s of EXPORT_SCALES
        rgba   := item+ end        on an RGBA frame, every piece at scale s                         s of RGBA_SCALES
        item   := pointwise modules in pipe order | denoiseprofile | diffuse | rgb_to_lab (nlmeans | bilat)+ lab_to_rgb
        end    := float | export_u16 [export_rows] | export_u8

    (a list whose draw leaves the fourth channel unwritten gets a colorout behind its items: alpha_is_written()).
    The shape, the scale and the first stencil module go round with the seed, so that a short seed list holds every scale,
    both shapes and every stencil module at a scale; the rest is drawn.  generate() is not touched by any of this.
    tags: "bands" (by band_eligible() over the exact halos, exact_halo()), "batch", "shape", "scale", "start", "end", "tables"."""
    tb = tables if tables is not None else Tables(False)
    rng = np.random.default_rng(7000 + seed)
    shape = ("export", "rgba")[seed % 2]
    first = SCALED_STENCILS[(seed // 2) % len(SCALED_STENCILS)]
    if shape == "export":
        scale = EXPORT_SCALES[(seed // 2) % len(EXPORT_SCALES)]
        w, h = RAW_FRAMES[int(rng.integers(0, len(RAW_FRAMES)))]
    else:
        scale = RGBA_SCALES[(seed // 8) % len(RGBA_SCALES)]
        w, h = RGBA_FRAMES[int(rng.integers(0, 3))]  # (the fourth is lower than three bands' halos)
    b = _Builder(rng, tb, w, h)
    b.plain = shape == "rgba"
    if shape == "export":
        mosaic = synth.bayer_mosaic(w, h, seed=100 + seed)
        u16 = b.chance(0.5)
        rng_f = float(synth.WHITE - synth.BLACK)
        src = mosaic if u16 else mosaic.astype(np.float32)
        b.add("rawprepare", abi.RawprepareData(0, 0, 0, 0, abi.f4(*[synth.BLACK] * 4), abi.f4(*[rng_f] * 4)),
              abi.Piece.make(w, h, filters=synth.FILTERS_RGGB, channels=1, datatype=abi.DT_HIP_TYPE_UINT16 if u16 else abi.DT_HIP_TYPE_FLOAT))
        if b.chance(0.7):
            b.add("temperature", abi.TemperatureData(abi.f4(*synth.WB_COEFFS)),
                  abi.Piece.make(w, h, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=b.pm))
            b.pm = synth.WB_COEFFS
        cfa = abi.Piece.make(w, h, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=b.pm)
        if b.chance(0.5):
            b.add("highlights", abi.HighlightsData(abi.DT_HIP_HIGHLIGHTS_CLIP, 1.0), cfa)
        b.add("demosaic", abi.DemosaicData(0, 0, DEMOSAICS[int(rng.integers(0, len(DEMOSAICS)))], 0.0), cfa)
        ow, oh = max(int(round(w * scale)), 1), max(int(round(h * scale)), 1)
        b.add("initialscale", abi.FinalscaleData(int(rng.integers(0, 3))),
              abi.Piece.make(ow, oh, processed_maximum=b.pm, roi_in=abi.Roi.make(0, 0, w, h, 1.0), roi_out=abi.Roi.make(0, 0, ow, oh, scale)))
        b.w, b.h = ow, oh
        start = "raw_u16" if u16 else "raw_f32"
    else:
        src = synth.rgba_image(w, h, seed=100 + seed, lo=-0.05, hi=1.6)
        start = "rgba_scene"
    b.scale = scale

    def item(kind):
        if kind in ("nlmeans", "bilat", "lab"):
            b.add("rgb_to_lab", lab_data("rgb_to_lab", tb))
            ops = (kind,) if kind != "lab" else b.pick((("nlmeans", "bilat"), ("bilat", "nlmeans"), ("bilat",), ("nlmeans",)))
            if kind == "nlmeans" and b.chance(0.5):
                ops = ("nlmeans", "bilat")
            for op in ops:
                b.module(op, lab=True)
            b.add("lab_to_rgb", lab_data("lab_to_rgb", tb))
        elif kind in ("denoiseprofile", "diffuse"):
            b.module(kind)
        else:
            for op in [op for op in RUN_OPS if b.chance(0.6)] or ["exposure"]:
                b.module(op)

    if b.chance(0.5):
        item("ordered")
    item(first)
    for _ in range(int(rng.integers(0, 3))):
        kind = b.pick(("ordered", "ordered", "denoiseprofile", "diffuse", "lab"))
        item(kind if kind == "ordered" or b.stencils < 3 else "ordered")
    if not alpha_is_written(b.nodes):
        # the draw left the fourth channel to the demosaic (or the local laplacian), which does not write it: the output profile
        # closes the list, as in the product's pipe
        b.module("colorout")
    end = ENDINGS[int(rng.integers(0, FRAME_ENDINGS))]
    if end in ("u16", "u16_rows"):
        b.add("export_u16", None)
    elif end != "float":
        b.add("export_u8", None)
    if end == "u16_rows":
        b.add("export_rows", abi.ExportRowsData(16, 3))
    bands = band_eligible(b.nodes, 2, exact_halo) and band_eligible(b.nodes, 3, exact_halo)
    tags = {"bands": bands, "batch": True, "shape": shape, "scale": scale, "start": start, "end": end, "tables": tb}
    return b.nodes, np.ascontiguousarray(src), tags


def describe(nodes):
    return " ".join(n.op for n in nodes)


# ---- the fixed cases of tests/test_gpu_fused_variants.py (built here so that the CPU suite can check their reference) ----
CM_KINDS = (None,) + ADAPTATIONS
FM_KINDS = (None, "agx_medium", "v7", "v6_split", "v6_chroma")
VARIANT_FRAME = (127, 93)


def variant_frames():
    w, h = VARIANT_FRAME
    return {"scene": synth.rgba_image(w, h, seed=2, lo=-0.05, hi=1.6), "adversarial": synth.adversarial_rgba(w, h)}


def variant_lab_frame():
    """the scene frame in Lab: the input of a run that starts at "lab_to_rgb" """
    w, h = VARIANT_FRAME
    img = synth.rgba_image(w, h, seed=2, lo=0.0, hi=1.0)
    lab = ck.aligned_empty(img.shape, np.float32)
    assert ck.call(ck.oracle(), "oracle_rgb_to_lab", abi.Piece.make(w, h, channels=4), abi.LabData.make(params.WORK_IN), img, lab) == 0
    return np.ascontiguousarray(lab)


def run_nodes_of(tb, cm=None, fm=None, present=("exposure", "colorin", "colorout"), end="u16", pre_lab=False,
                 post_lab=False, cm_clip=True, filmic_export=True, flavour="matrix", size=VARIANT_FRAME, scale=1.0):
    """one fusable run: [lab_to_rgb] exposure colorin [channelmixerrgb] [filmicrgb] colorout [rgb_to_lab | export_u16
    [export_rows]], each of exposure / colorin / colorout only if named in `present`"""
    w, h = size
    rgb = abi.Piece.make(w, h, channels=4, processed_maximum=synth.WB_COEFFS)
    if scale != 1.0:
        rgb.roi_in.scale = rgb.roi_out.scale = float(scale)
    nodes = []
    if pre_lab:
        nodes.append(pipe.Node("lab_to_rgb", lab_data("lab_to_rgb", tb), rgb))
    if "exposure" in present:
        nodes.append(pipe.Node("exposure", EXPOSURE, rgb))
    if "colorin" in present:
        nodes.append(pipe.Node("colorin", conversion_data("colorin", flavour, tb), rgb))
    if cm is not None:
        nodes.append(pipe.Node("channelmixerrgb", channelmixer_data(cm, clip=cm_clip), rgb))
    if fm is not None:
        nodes.append(pipe.Node("filmicrgb", filmic_data(fm, use_output_profile=filmic_export), rgb))
    if "colorout" in present:
        nodes.append(pipe.Node("colorout", conversion_data("colorout", flavour, tb), rgb))
    if post_lab:
        assert end == "float"
        nodes.append(pipe.Node("rgb_to_lab", lab_data("rgb_to_lab", tb), rgb))
    if end in ("u16", "rows"):
        nodes.append(pipe.Node("export_u16", None, rgb))
    if end == "rows":
        nodes.append(pipe.Node("export_rows", abi.ExportRowsData(16, 3), rgb))
    return nodes


SUBSETS = tuple(tuple(op for k, op in enumerate(("exposure", "colorin", "colorout")) if m >> k & 1) for m in range(8))
SWITCHES = (("present", SUBSETS), ("end", ("float", "u16", "rows")), ("pre_lab", (False, True)), ("post_lab", (False, True)),
            ("cm_clip", (False, True)), ("filmic_export", (False, True)), ("flavour", FLAVOURS),
            ("base", ((abi.DT_HIP_ADAPTATION_CAT16, "agx_medium"), (abi.DT_HIP_ADAPTATION_XYZ, "v7"),
                      (abi.DT_HIP_ADAPTATION_RGB, "v6_chroma"))))


def _valid(combo):
    return not (combo[3] and combo[1] != 0)  # "rgb_to_lab" closes a run that ends in float only


def _pairs_of(combo):
    return {(i, combo[i], j, combo[j]) for i in range(len(combo)) for j in range(i + 1, len(combo))}


def pairwise_cases():
    """a covering set over the run-time switches of rgb_chain: every pair of values of two switches that can occur
    together does, in at least one case.  Greedy over the valid combinations, in a fixed order: the same set every time.
    Returns (cases, the pairs to cover); a case is a tuple of value indices in the order of SWITCHES."""
    import itertools
    combos = [c for c in itertools.product(*[range(len(v)) for _, v in SWITCHES]) if _valid(c)]
    want = set()
    for c in combos:
        want |= _pairs_of(c)
    left, cases = set(want), []
    while left:
        best = max(combos, key=lambda c: len(_pairs_of(c) & left))
        cases.append(best)
        left -= _pairs_of(best)
    return cases, want


def pairwise_kwargs(case):
    kw = {name: values[k] for (name, values), k in zip(SWITCHES, case)}
    kw["cm"], kw["fm"] = kw.pop("base")
    return kw


SCALED_PAIRS = ("wavelets+run-cm_none", "bilateral+run", "diffuse+rgb_to_lab", "nlmeans>bilat>run")  # one case per fused pair


def fused_pair_cases(tb, scale=1.0):
    """(name, nodes, input kind, the pairs that fuse by rule, launch groups) for the four fused pairs of the frame walk and their
    fallbacks.  Frames of 200 x 333: the stencil modules' oracles stay cheap.  scale: the scale of every piece's regions."""
    w, h = 200, 333
    rgb = abi.Piece.make(w, h, channels=4, processed_maximum=synth.WB_COEFFS)
    if scale != 1.0:
        rgb.roi_in.scale = rgb.roi_out.scale = float(scale)

    def run(fm=None, end="float", **kw):
        return run_nodes_of(tb, cm=abi.DT_HIP_ADAPTATION_CAT16, fm=fm, end=end, size=(w, h), scale=scale, **kw)

    def N(op, data):
        return pipe.Node(op, data, rgb)

    wav = params.denoiseprofile()
    nlm = params.denoiseprofile(mode=abi.DT_HIP_DENOISEPROFILE_NLMEANS)
    to_lab, to_rgb = lab_data("rgb_to_lab", tb), lab_data("lab_to_rgb", tb)
    blend = N("blend", blend_data("lab_uniform"))
    soft = params.diffuse("lens_deblur_soft", iterations=2)
    nl = abi.NlmeansData(2.0, 50.0, 0.5, 1.0)
    # dn_finish_chain<CM> (denoiseprofile.hip) is six more compiled copies of px_channelmixerrgb: one case per kind
    out = [("wavelets+run-" + ("cm_none" if cm is None else "cm_%d" % cm),
            [N("denoiseprofile", wav)] + run_nodes_of(tb, cm=cm, end="float", size=(w, h), scale=scale), "rgb", {"denoiseprofile+run"})
           for cm in CM_KINDS]
    out += [
        ("wavelets+run_with_filmic", [N("denoiseprofile", wav)] + run(fm="agx_medium", end="u16"), "rgb", set()),
        ("dn_nlmeans+run", [N("denoiseprofile", nlm)] + run(), "rgb", set()),
        ("dn_nlmeans+run_with_filmic", [N("denoiseprofile", nlm)] + run(fm="v7", end="u16"), "rgb", set()),
        ("bilateral+run", [N("bilat", BILAT["bilateral"]()), N("lab_to_rgb", to_rgb)] + run(fm="agx_medium", end="u16"),
         "lab", {"bilat+run"}),
        ("laplacian+run", [N("bilat", BILAT["laplacian"]()), N("lab_to_rgb", to_rgb)] + run(fm="agx_medium", end="u16"), "lab", set()),
        ("diffuse+rgb_to_lab", [N("diffuse", soft), N("rgb_to_lab", to_lab)], "rgb", {"diffuse+rgb_to_lab"}),
        ("diffuse+rgb_to_lab_nonlinear", [N("diffuse", soft), N("rgb_to_lab", lab_data("rgb_to_lab", tb, True))], "rgb", set()),
        ("nlmeans>bilat>run", [N("nlmeans", nl), N("bilat", BILAT["bilateral"]()), N("lab_to_rgb", to_rgb)] + run(end="u16"),
         "lab", {"nlmeans>bilat", "bilat+run"}),
        ("nlmeans>bilat>blend", [N("nlmeans", nl), N("bilat", BILAT["bilateral_fine"]()), blend, N("lab_to_rgb", to_rgb)] + run(end="u16"),
         "lab", {"nlmeans>bilat"}),
        ("nlmeans>laplacian>run", [N("nlmeans", nl), N("bilat", BILAT["laplacian"]()), N("lab_to_rgb", to_rgb)] + run(end="u16"),
         "lab", set()),
    ]
    # the launch groups of each list: the module or modules on their own, the blend, and ONE fused run behind them
    groups = {"nlmeans>bilat>run": 3, "nlmeans>bilat>blend": 4, "nlmeans>laplacian>run": 3}
    return [c + (groups.get(c[0], 2),) for c in out]


def pair_frame(kind):
    w, h = 200, 333
    img = synth.rgba_image(w, h, seed=9, lo=0.0, hi=1.0)
    if kind == "rgb":
        return img
    lab = ck.aligned_empty(img.shape, np.float32)
    rgb = abi.Piece.make(w, h, channels=4)
    assert ck.call(ck.oracle(), "oracle_rgb_to_lab", rgb, abi.LabData.make(params.WORK_IN), img, lab) == 0
    return np.ascontiguousarray(lab)


# ---- lists the library must refuse ---------------------------------------------------------------------------------------
def invalid_cases(tb):
    """(name, nodes, words of the refusal): each must come back DT_HIP_INVALID_ARG with the pool at its baseline"""
    w, h = 64, 48
    rgb = abi.Piece.make(w, h, channels=4)
    exposure = pipe.Node("exposure", EXPOSURE, rgb)
    blend = pipe.Node("blend", blend_data("uniform"), rgb)
    flip6 = pipe.Node("flip", params.flip(6), abi.Piece.make(w, h, channels=4, roi_out=abi.Roi.make(0, 0, h, w)))
    jd = params.jpeg(90)
    jd.capacity = pipe.jpeg_bound(w, h, jd)
    pd = params.png(bpp=16)
    pd.capacity = pipe.png_bound(w, h, pd)
    one = abi.Piece.make(h, w, channels=1)
    return [
        ("jpeg_not_last", [exposure, pipe.Node("export_u8", None, rgb), pipe.Node("export_jpeg", jd, rgb),
                           pipe.Node("export_rows", abi.ExportRowsData(8, 3), rgb)], "must be the last node"),
        ("jpeg_behind_u16", [exposure, pipe.Node("export_u16", None, rgb), pipe.Node("export_jpeg", jd, rgb)], "behind 'export_u8'"),
        ("png16_behind_u8", [exposure, pipe.Node("export_u8", None, rgb), pipe.Node("export_png", pd, rgb)], "behind 'export_u16'"),
        ("flip_then_one_channel", [exposure, flip6, pipe.Node("temperature", abi.TemperatureData(abi.f4(1, 1, 1, 1)), one)], "channels"),
        ("blend_first", [blend, exposure], "needs the module"),
        ("blend_behind_flip", [exposure, flip6, blend], "flip has no blending"),
        ("blend_behind_dropped_flip", [exposure, pipe.Node("flip", params.flip(0), rgb), blend], "flip has no blending"),
    ]


SEEDS = tuple(range(1, 73))
