"""Host-side mirror of the export pixelpipe for the hot path: an ordered list of nodes, each a
module with its committed `data` and its piece view, executed on one device through the C-ABI --
what dt_dev_pixelpipe_process_rec() + pixelpipe_process_on_GPU() do in the reference
(src/develop/pixelpipe_hb.c:881-1282, src/develop/pixelpipe_gpu.c:191-744), reduced to the
device-resident chain: every module output stays in HBM and is the next module's input.

Buffers are caller-provided device pointers (torch tensors in bench.py, DeviceBuffer in tests).
"""
import ctypes as C

import numpy as np

from . import abi, lib, params, synth

# bytes per pixel of each module's input / output (algorithmic traffic)
MODULE_BPP = {
    "rawprepare": (2, 4), "temperature": (4, 4), "highlights": (4, 4), "demosaic": (4, 16),
    "exposure": (16, 16), "colorin": (16, 16), "channelmixerrgb": (16, 16), "filmicrgb": (16, 16),
    "colorout": (16, 16), "export_u16": (16, 8), "rgb_to_lab": (16, 16), "lab_to_rgb": (16, 16), "nlmeans": (16, 16),
    "bilat": (16 + 16, 16),  # splat reads L, slice reads + writes the plane (48 B/px)
    "flip": (16, 16),
    "export_u8": (16, 4), "export_jpeg": (4, 0),
    "export_png": (4, 0),  # 8 bits: node_bytes_per_px() reads 8 B/px at 16 bits
    "export_tiff": (4, 0),  # 8 bits: node_bytes_per_px() reads 8 / 16 B/px at 16 / 32 bits
    "export_webp": (4, 0),
}


class Node:
    def __init__(self, op, data, piece):
        self.op = op
        self.data = data
        self.piece = piece


def insert_flip(nodes, after_op, orientation, image_orientation=0):
    """the flip module right behind the node `after_op`: orientation 0..7, or -1 for image_orientation (params.flip()).
    The nodes behind it get the oriented geometry (their pieces are copied, not changed in place)."""
    data = params.flip(orientation, image_orientation)
    k = [n.op for n in nodes].index(after_op)
    # flip's input format is what the next module reads (a piece describes its module's INPUT: behind demosaic, whose own
    # piece is the mosaic's, that is float4)
    src = nodes[k + 1].piece
    w, h = nodes[k].piece.roi_out.width, nodes[k].piece.roi_out.height
    ow, oh = params.oriented_size(w, h, data.orientation)
    fp = abi.Piece.make(w, h, channels=src.channels, processed_maximum=tuple(src.processed_maximum),
                        roi_out=abi.Roi.make(0, 0, ow, oh))
    out = list(nodes[:k + 1]) + [Node("flip", data, fp)]
    for n in nodes[k + 1:]:
        p = n.piece
        q = abi.Piece.make(ow, oh, filters=p.filters, channels=p.channels, datatype=p.datatype,
                           processed_maximum=tuple(p.processed_maximum))
        out.append(Node(n.op, n.data, q))
    return out


def with_jpeg(nodes, jpeg_data):
    """the node list with its trailing export_u16 swapped for export_u8 + export_jpeg (jpeg_data: params.jpeg() or an
    abi.JpegData, its capacity set -- jpeg_bound()).  The node's output is the little-endian uint64 file length, then the
    file.  The other nodes are shared with `nodes`."""
    if not nodes or nodes[-1].op != "export_u16":
        raise ValueError("with_jpeg: the node list does not end in export_u16")
    last = nodes[-1]
    w, h = last.piece.roi_out.width, last.piece.roi_out.height
    return list(nodes[:-1]) + [Node("export_u8", None, last.piece),
                               Node("export_jpeg", jpeg_data, abi.Piece.make(w, h, channels=4))]


def jpeg_bound(width, height, jpeg_data):
    """dt_hip_jpeg_bound(): a capacity the encoder's output always fits"""
    return int(lib.load().dt_hip_jpeg_bound(width, height, C.byref(jpeg_data)))


def with_png(nodes, png_data):
    """the node list with export_png appended behind its trailing export_u16 (png_data: params.png() or an abi.PngData,
    its capacity set -- png_bound()); at 8 bits the export_u16 is swapped for export_u8 first.  The node's output is the
    little-endian uint64 file length, then the file.  The other nodes are shared with `nodes`."""
    if not nodes or nodes[-1].op != "export_u16":
        raise ValueError("with_png: the node list does not end in export_u16")
    last = nodes[-1]
    w, h = last.piece.roi_out.width, last.piece.roi_out.height
    head = list(nodes) if png_data.bit_depth == 16 else list(nodes[:-1]) + [Node("export_u8", None, last.piece)]
    return head + [Node("export_png", png_data, abi.Piece.make(w, h, channels=4))]


def png_bound(width, height, png_data):
    """dt_hip_png_bound(): a capacity the encoder's output always fits"""
    return int(lib.load().dt_hip_png_bound(width, height, C.byref(png_data)))


def with_tiff(nodes, tiff_data):
    """the node list with export_tiff appended (tiff_data: params.tiff() or an abi.TiffData, its capacity set --
    tiff_bound()): at 16 bits behind the trailing export_u16, at 8 bits that node is swapped for export_u8 first, at 32
    bits it is dropped and the encoder reads the float frame of the node in front of it.  The node's output is the
    little-endian uint64 file length, then the file.  The other nodes are shared with `nodes`."""
    if not nodes or nodes[-1].op != "export_u16":
        raise ValueError("with_tiff: the node list does not end in export_u16")
    last = nodes[-1]
    w, h = last.piece.roi_out.width, last.piece.roi_out.height
    head = {16: list(nodes), 8: list(nodes[:-1]) + [Node("export_u8", None, last.piece)], 32: list(nodes[:-1])}[int(tiff_data.bpp)]
    return head + [Node("export_tiff", tiff_data, abi.Piece.make(w, h, channels=4))]


def tiff_bound(width, height, tiff_data):
    """dt_hip_tiff_bound(): a capacity the encoder's output always fits"""
    return int(lib.load().dt_hip_tiff_bound(width, height, C.byref(tiff_data)))


def with_webp(nodes, webp_data):
    """the node list with its trailing export_u16 swapped for export_u8 + export_webp (webp_data: params.webp() or an
    abi.WebpData, its capacity set -- webp_bound()).  The node's output is the little-endian uint64 file length, then the
    file.  The other nodes are shared with `nodes`."""
    if not nodes or nodes[-1].op != "export_u16":
        raise ValueError("with_webp: the node list does not end in export_u16")
    last = nodes[-1]
    w, h = last.piece.roi_out.width, last.piece.roi_out.height
    return list(nodes[:-1]) + [Node("export_u8", None, last.piece),
                               Node("export_webp", webp_data, abi.Piece.make(w, h, channels=4))]


def webp_bound(width, height, webp_data):
    """dt_hip_webp_bound(): a capacity the encoder's output always fits"""
    return int(lib.load().dt_hip_webp_bound(width, height, C.byref(webp_data)))


def light_pipe_nodes(width, height, lut_target_ptr, lut_first, lut_coeffs, with_filmic=True, filmic=None,
                     demosaic_method=abi.DT_HIP_DEMOSAIC_RCD, orientation=None, image_orientation=0):
    """config 2 of BASELINE.json: rawprepare -> temperature -> highlights(clip) -> demosaic ->
    exposure -> colorin -> color calibration -> filmic -> colorout -> u16, module defaults.
    orientation (None: no node): the flip module between demosaic and exposure (insert_flip())."""
    raw = abi.Piece.make(width, height, filters=synth.FILTERS_RGGB, channels=1, datatype=abi.DT_HIP_TYPE_UINT16)
    cfa1 = abi.Piece.make(width, height, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=(1, 1, 1, 1))
    cfa2 = abi.Piece.make(width, height, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=synth.WB_COEFFS)
    rgb = abi.Piece.make(width, height, channels=4, processed_maximum=synth.WB_COEFFS)
    rng = float(synth.WHITE - synth.BLACK)
    nodes = [
        Node("rawprepare", abi.RawprepareData(0, 0, 0, 0, abi.f4(*[synth.BLACK] * 4), abi.f4(*[rng] * 4)), raw),
        Node("temperature", abi.TemperatureData(abi.f4(*synth.WB_COEFFS)), cfa1),
        Node("highlights", abi.HighlightsData(abi.DT_HIP_HIGHLIGHTS_CLIP, 1.0), cfa2),
        Node("demosaic", abi.DemosaicData(0, 0, demosaic_method, 0.0), cfa2),
        # exposure +0.7 EV, black -0.000244 (module defaults for scene-referred workflow)
        Node("exposure", abi.ExposureData(-0.000244140625, float(np.float32(2.0) ** np.float32(0.7))), rgb),
        Node("colorin", params.conversion(params.WORK_OUT @ params.CAMERA_TO_XYZ), rgb),
        Node("channelmixerrgb", params.channelmixerrgb(), rgb),
    ]
    if with_filmic:
        nodes.append(Node("filmicrgb", filmic, rgb))
    lt = [(lut_target_ptr, lut_first, lut_coeffs)] * 3
    nodes.append(Node("colorout", params.conversion(params.SRGB_OUT @ params.WORK_IN, lut_target=lt), rgb))
    nodes.append(Node("export_u16", None, rgb))
    if orientation is not None:
        nodes = insert_flip(nodes, "demosaic", orientation, image_orientation)
    return nodes


def denoise_pipe_nodes(width, height, lut_target_ptr, lut_first, lut_coeffs, filmic=None,
                       diffuse_preset="lens_deblur_soft", diffuse_iterations=2, with_nlmeans=False, with_bilat=None,
                       orientation=None, image_orientation=0):
    """config 3 of BASELINE.json, as far as it runs on device: the light pipe + denoise (profiled)
    wavelets after demosaic and diffuse-or-sharpen after color calibration, in the reference's module
    order (src/develop/iop_order.c:196-232).  orientation (None: no node): the flip module between
    denoise (profiled) and exposure (insert_flip())."""
    nodes = light_pipe_nodes(width, height, lut_target_ptr, lut_first, lut_coeffs, with_filmic=filmic is not None,
                             filmic=filmic)
    rgb = abi.Piece.make(width, height, channels=4, processed_maximum=synth.WB_COEFFS)
    out = []
    for n in nodes:
        out.append(n)
        if n.op == "demosaic":
            out.append(Node("denoiseprofile", params.denoiseprofile(), rgb))
        if n.op == "channelmixerrgb":
            out.append(Node("diffuse", params.diffuse(diffuse_preset, iterations=diffuse_iterations), rgb))
            if with_nlmeans:
                # a Lab module: the pipe converts work RGB -> Lab before and back after it (pixelpipe_cpu.c:59-75)
                out.append(Node("rgb_to_lab", abi.LabData.make(params.WORK_IN), rgb))
                out.append(Node("nlmeans", abi.NlmeansData(2.0, 50.0, 0.5, 1.0), rgb))
                if with_bilat is None or with_bilat:
                    out.append(Node("bilat", abi.BilatData.bilateral(), rgb))
                out.append(Node("lab_to_rgb", abi.LabData.make(params.WORK_OUT), rgb))
    if orientation is not None:
        out = insert_flip(out, "denoiseprofile", orientation, image_orientation)
    return out


def node_bytes_per_px(n):
    """algorithmic bytes per pixel of one node"""
    if n.op == "denoiseprofile":
        from . import modinfo
        return 112 + 96 * modinfo.denoiseprofile_bands(n.piece)
    if n.op == "diffuse":
        from . import modinfo
        return 96 * max(int(n.data.iterations), 1) * modinfo.diffuse_scales(n.piece, n.data)
    if n.op == "export_png":
        return int(n.data.bit_depth) // 2  # RGBA u8 or u16 in, the file (a fraction of it) out
    if n.op == "export_tiff":
        return int(n.data.bpp) // 2  # RGBA u8, u16 or f32 in, the file out
    return sum(MODULE_BPP[n.op])


def algorithmic_bytes_per_pixel(nodes):
    return sum(node_bytes_per_px(n) for n in nodes)


class DevicePipe:
    """dt_hip_pipe_t: the C++ executor of libansel_hip (csrc/pipe.cpp; batches, row bands and tiling in pipe_batch.cpp, pipe_bands.cpp, pipe_tiling.cpp) loaded with a node list"""

    def __init__(self, devid, nodes, fusion=True):
        self.lib = lib.load()
        self.devid = devid
        self.nodes = nodes  # keeps the ctypes structs alive
        self.handle = self.lib.dt_hip_pipe_new(devid)
        if not self.handle:
            raise lib.AnselHipError("dt_hip_pipe_new failed: %s" % self.lib.dt_hip_last_error().decode())
        for n in nodes:
            if n.data is None:
                rc = self.lib.dt_hip_pipe_add_node(self.handle, n.op.encode(), C.byref(n.piece), None, 0)
            else:
                rc = self.lib.dt_hip_pipe_add_node(self.handle, n.op.encode(), C.byref(n.piece),
                                                   C.cast(C.byref(n.data), C.c_void_p), C.sizeof(n.data))
            lib.check(rc, "dt_hip_pipe_add_node(%s)" % n.op)
        self.lib.dt_hip_pipe_set_fusion(self.handle, 1 if fusion else 0)

    @property
    def num_groups(self):
        return self.lib.dt_hip_pipe_num_groups(self.handle)

    def process(self, dev_in, dev_out):
        lib.check(self.lib.dt_hip_pipe_process(self.handle, dev_in, dev_out), "dt_hip_pipe_process")

    READ_FILE_STAGING = 64 << 20

    def read_file(self, dev_out_ptr, capacity, staging_bytes=None):
        """the file a pipe that ends in export_jpeg / _png / _tiff / _webp left in dev_out_ptr (`capacity` bytes: the length
        word, then the file) -> bytes.  dt_hip_read_file_to_host() moves the file and not the capacity, through a pinned
        staging buffer of min(capacity, 64 MiB) (staging_bytes: another size); a longer file is read once more into a buffer
        of the 8 + L the first call reported."""
        devid = self.devid
        nbytes = max(8, min(int(capacity), int(staging_bytes or self.READ_FILE_STAGING)))
        for attempt in (0, 1):
            # (a multiple of 16 so that nothing else shares the last 16-byte word; host_bytes itself stays within the capacity)
            host = self.lib.dt_hip_alloc_host_pinned((nbytes + 15) & ~15)
            if not host:
                raise lib.AnselHipError("read_file: no pinned staging buffer of %d bytes" % nbytes)
            try:
                lib.check(self.lib.dt_hip_read_file_to_host(devid, dev_out_ptr, capacity, host, nbytes), "dt_hip_read_file_to_host")
                if self.lib.dt_hip_finish(devid) != 1:
                    raise lib.AnselHipError("read_file: dt_hip_finish failed: %s" % self.lib.dt_hip_last_error().decode())
                n = C.c_uint64.from_address(host).value
                if n == 2 ** 64 - 1:
                    raise lib.AnselHipError("read_file: no file in the buffer (length word UINT64_MAX: the encoder refused the "
                                            "frame, or its file does not fit the %d bytes of capacity)" % capacity)
                if 8 + n <= nbytes:
                    return C.string_at(host + 8, n)
            finally:
                self.lib.dt_hip_free_host_pinned(host)
            if attempt:
                break
            nbytes = 8 + n
        raise lib.AnselHipError("read_file: the file of %d bytes did not fit a staging buffer of %d" % (n, nbytes))

    def close(self):
        if self.handle:
            self.lib.dt_hip_pipe_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_nodes(devid, nodes, buffers):
    """buffers: list of len(nodes)+1 device pointers; node i reads buffers[i], writes buffers[i+1]"""
    l = lib.load()
    for i, n in enumerate(nodes):
        src, dst = buffers[i], buffers[i + 1]
        if n.op == "export_u16":
            rc = l.dt_hip_export_convert_u16(devid, n.piece.roi_out.width, n.piece.roi_out.height, src, dst)
        elif n.op in ("rgb_to_lab", "lab_to_rgb"):
            rc = getattr(l, "dt_hip_transform_" + n.op)(devid, C.byref(n.piece), C.byref(n.data), src, dst)
        else:
            fn = getattr(l, "dt_hip_iop_%s_process" % n.op)
            rc = fn(devid, C.byref(n.piece), C.byref(n.data), src, dst)
        lib.check(rc, n.op)
