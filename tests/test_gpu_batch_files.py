"""-m gpu: a batch in file mode (dt_hip_batch_set_file_output(), pipe_batch.cpp) and DevicePipe.read_file().

The light pipe at 304 x 200 through pipe.with_jpeg / with_png (8 bits) / with_tiff (8 bits, deflate, predictor 2) / with_webp;
three frames at depth 2 -- a noise mosaic, a flat one and synth.bayer_mosaic(), so that the lengths of two frames that share
a slot differ strongly.  The reference is the existing single-frame path: p.process() and a download of the whole capacity.

  * the writer gets bytes == 8 + L and the single-frame file, and the host buffer keeps its fill from 8 + L on: the
    download was trimmed
  * host buffers of the middle file's size: the longest frame's wait is DT_HIP_FILE_TOO_LARGE, its writer call never
    happens, its buffer holds the true L and the fill; the frames behind it are written; a drain reports the error once
  * without a writer dt_hip_batch_wait() gives the same codes and dt_hip_batch_file_bytes() the 8 + L
  * what the mode refuses, and the mode switched off again
  * DevicePipe.read_file(), with a staging buffer smaller than the file too"""
import ctypes as C

import numpy as np
import pytest

import hipcheck as hc
from ansel_amd import abi, filmic, lib, params, pipe, synth

pytestmark = pytest.mark.gpu

W, H = 304, 200
FILL = 0xA5
U64_MAX = 2 ** 64 - 1
WRITER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_size_t)

FORMATS = {
    "jpeg": (lambda: params.jpeg(95), pipe.with_jpeg, pipe.jpeg_bound),
    "png": (lambda: params.png(8), pipe.with_png, pipe.png_bound),
    "tiff": (lambda: params.tiff(bpp=8, compress=2), pipe.with_tiff, pipe.tiff_bound),
    "webp": (lambda: params.webp(), pipe.with_webp, pipe.webp_bound),
}


def _base(lut_ptr, lut):
    return pipe.light_pipe_nodes(W, H, lut_ptr, float(lut[0]), params.unbounded_coeffs(lut), with_filmic=True,
                                 filmic=filmic.default_data())


def _frames():
    rng = np.random.default_rng(5)
    noise = rng.integers(synth.BLACK, synth.WHITE + 1, (H, W)).astype(np.uint16)
    flat = np.full((H, W), 4000, np.uint16)
    return [noise, flat, np.ascontiguousarray(synth.bayer_mosaic(W, H, seed=41)).view(np.uint16).reshape(H, W)]


class _Setup:
    """a format's pipe, its three frames and their single-frame files (the reference), made once"""

    def __init__(self, fmt):
        self.l = l = hc.hip()
        make, with_fmt, bound = FORMATS[fmt]
        self.lut = params.srgb_encode_lut()
        self.d_lut = lib.DeviceBuffer.from_numpy(0, self.lut)
        self.data = make()
        self.data.capacity = bound(W, H, self.data)
        assert self.data.capacity > 0, "%s refuses %d x %d" % (fmt, W, H)
        self.nb_in, self.nb_out = W * H * 2, int(self.data.capacity)
        self.pipe = pipe.DevicePipe(0, with_fmt(_base(self.d_lut.ptr, self.lut), self.data), fusion=True)
        self.frames = _frames()
        self.d_in, self.d_out = lib.DeviceBuffer(0, self.nb_in), lib.DeviceBuffer(0, self.nb_out)
        self.want = []
        for f in self.frames:
            self.d_in.upload(f)
            self.pipe.process(self.d_in.ptr, self.d_out.ptr)
            assert l.dt_hip_finish(0) == 1, l.dt_hip_last_error()
            buf = self.d_out.to_numpy((self.nb_out,), np.uint8)
            n = int(buf[:8].view(np.uint64)[0])
            assert n != U64_MAX and 8 + n <= self.nb_out
            self.want.append(buf[8:8 + n].tobytes())
        self.pinned = []

    def pin(self, nbytes, fill=None):
        p = self.l.dt_hip_alloc_host_pinned(nbytes)
        assert p
        self.pinned.append(p)
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (nbytes,))
        if fill is not None:
            a[:] = fill
        return p, a

    def unpin(self):
        for p in self.pinned:
            self.l.dt_hip_free_host_pinned(p)
        self.pinned = []

    def close(self):
        self.unpin()
        self.pipe.close()
        for b in (self.d_in, self.d_out, self.d_lut):
            b.release()


@pytest.fixture(scope="module", params=sorted(FORMATS))
def fmt(request):
    s = _Setup(request.param)
    yield s
    s.close()


@pytest.fixture(scope="module")
def jpeg():
    s = _Setup("jpeg")
    yield s
    s.close()


class _Writer:
    def __init__(self):
        self.calls = []
        self.cb = WRITER(self._write)

    def _write(self, user, seq, host_out, nbytes):
        self.calls.append((seq, nbytes, C.string_at(host_out, nbytes)))
        return 0


def _stream(s, b, order, depth=2):
    """the frames `order` (indices into s.frames) through batch b, each with a pinned host_out of its own of s.nb_out bytes
    of FILL; the slot is waited for in front of the submit that needs it -> every frame's wait code, every host buffer"""
    l = s.l
    pin_in = [s.pin(s.nb_in) for _ in range(depth)]
    outs = [s.pin(s.nb_out, FILL) for _ in order]
    codes, slots = [], []
    for k, idx in enumerate(order):
        if k >= depth:
            codes.append(l.dt_hip_batch_wait(b, slots[k - depth]))
        pin_in[k % depth][1][:] = s.frames[idx].view(np.uint8).reshape(-1)
        slots.append(l.dt_hip_batch_submit(b, pin_in[k % depth][0], outs[k][0]))
        assert slots[-1] >= 0, l.dt_hip_last_error()
    for k in range(max(0, len(order) - depth), len(order)):
        codes.append(l.dt_hip_batch_wait(b, slots[k]))
    return codes, [a for _, a in outs]


def _word(a):
    return int(a[:8].view(np.uint64)[0])


def test_files_equal_the_single_frame_files(fmt):
    s, l = fmt, fmt.l
    lengths = [len(f) for f in s.want]
    assert max(lengths) > 1.5 * min(lengths), lengths  # frames that share a slot differ strongly in L
    wr = _Writer()
    b = l.dt_hip_batch_new(s.pipe.handle, 2, s.nb_in, s.nb_out)
    assert b
    assert l.dt_hip_batch_set_writer(b, wr.cb, None) == 0
    assert l.dt_hip_batch_set_file_output(b, s.nb_out) == 0, l.dt_hip_last_error()
    codes, outs = _stream(s, b, [0, 1, 2])
    assert l.dt_hip_batch_drain(b) == 0
    l.dt_hip_batch_free(b)
    assert codes == [0, 0, 0]
    assert [c[0] for c in wr.calls] == [0, 1, 2]
    for k, (seq, nbytes, got) in enumerate(wr.calls):
        n = len(s.want[k])
        assert nbytes == 8 + n, "frame %d" % k
        assert got[:8] == np.uint64(n).tobytes() and got[8:] == s.want[k], "frame %d" % k
        assert outs[k][:8 + n].tobytes() == got
        assert (outs[k][8 + n:] == FILL).all(), "frame %d: the download wrote beyond 8 + L" % k
    s.unpin()


def test_small_host_buffers(fmt):
    s, l = fmt, fmt.l
    by_len = sorted(range(3), key=lambda k: len(s.want[k]))
    short, mid, longest = by_len
    # the middle file with its length word, rounded up to 16: what the middle and the short frame fit and the longest does not
    host_bytes = (8 + len(s.want[mid]) + 15) & ~15
    assert 8 + len(s.want[longest]) > host_bytes
    wr = _Writer()
    b = l.dt_hip_batch_new(s.pipe.handle, 2, s.nb_in, s.nb_out)
    assert b and l.dt_hip_batch_set_writer(b, wr.cb, None) == 0
    assert l.dt_hip_batch_set_file_output(b, host_bytes) == 0, l.dt_hip_last_error()
    # the longest first: the frames behind it are still written
    order = [longest, mid, short]
    codes, outs = _stream(s, b, order)
    assert codes == [abi.DT_HIP_FILE_TOO_LARGE, 0, 0]
    assert [c[0] for c in wr.calls] == [1, 2]
    assert _word(outs[0]) == len(s.want[longest]) and (outs[0][8:] == FILL).all()
    for k in (1, 2):
        n = len(s.want[order[k]])
        assert wr.calls[k - 1][1] == 8 + n and wr.calls[k - 1][2][8:] == s.want[order[k]]
        assert (outs[k][8 + n:] == FILL).all()
    assert l.dt_hip_batch_drain(b) == 0
    # a drain reports the frame once, with a message that names it and both sizes; the batch goes on afterwards
    codes, outs = _stream(s, b, [longest])
    assert codes == [abi.DT_HIP_FILE_TOO_LARGE]
    msg = l.dt_hip_last_error().decode()
    assert "frame 3" in msg and str(8 + len(s.want[longest])) in msg and str(host_bytes) in msg, msg
    assert l.dt_hip_batch_drain(b) == 0
    pin_in, out = s.pin(s.nb_in), s.pin(s.nb_out, FILL)
    pin_in[1][:] = s.frames[longest].view(np.uint8).reshape(-1)
    assert l.dt_hip_batch_submit(b, pin_in[0], out[0]) >= 0
    assert l.dt_hip_batch_drain(b) == abi.DT_HIP_FILE_TOO_LARGE
    assert "frame 4" in l.dt_hip_last_error().decode()
    assert l.dt_hip_batch_drain(b) == 0
    pin_in[1][:] = s.frames[short].view(np.uint8).reshape(-1)
    out[1][:] = FILL
    assert l.dt_hip_batch_submit(b, pin_in[0], out[0]) >= 0
    assert l.dt_hip_batch_drain(b) == 0
    l.dt_hip_batch_free(b)
    assert wr.calls[-1][0] == 5 and wr.calls[-1][2][8:] == s.want[short]
    assert len(wr.calls) == 3
    s.unpin()


def test_without_a_writer(fmt):
    s, l = fmt, fmt.l
    by_len = sorted(range(3), key=lambda k: len(s.want[k]))
    host_bytes = (8 + len(s.want[by_len[1]]) + 15) & ~15
    b = l.dt_hip_batch_new(s.pipe.handle, 2, s.nb_in, s.nb_out)
    assert b
    n = C.c_size_t(0)
    assert l.dt_hip_batch_file_bytes(b, 0, C.byref(n)) == abi.DT_HIP_INVALID_ARG  # the mode is off
    assert l.dt_hip_batch_set_file_output(b, host_bytes) == 0
    assert l.dt_hip_batch_file_bytes(b, 0, C.byref(n)) == abi.DT_HIP_INVALID_ARG  # no frame yet
    assert l.dt_hip_last_error()
    assert l.dt_hip_batch_file_bytes(b, 2, C.byref(n)) == abi.DT_HIP_INVALID_ARG  # no such slot
    codes, outs = _stream(s, b, by_len)
    assert codes == [0, 0, abi.DT_HIP_FILE_TOO_LARGE]
    # slot 0 held frames 0 and 2, slot 1 frame 1: the last frame waited for
    assert l.dt_hip_batch_file_bytes(b, 0, C.byref(n)) == 0 and n.value == 8 + len(s.want[by_len[2]])
    assert l.dt_hip_batch_file_bytes(b, 1, C.byref(n)) == 0 and n.value == 8 + len(s.want[by_len[1]])
    for k in (0, 1):
        f = s.want[by_len[k]]
        assert _word(outs[k]) == len(f) and outs[k][8:8 + len(f)].tobytes() == f and (outs[k][8 + len(f):] == FILL).all()
    assert _word(outs[2]) == len(s.want[by_len[2]]) and (outs[2][8:] == FILL).all()
    assert l.dt_hip_batch_drain(b) == 0
    l.dt_hip_batch_free(b)
    s.unpin()


def test_refused_settings(jpeg):
    s, l = jpeg, jpeg.l
    # a pipe that ends in export_u16 has no length word
    p16 = pipe.DevicePipe(0, _base(s.d_lut.ptr, s.lut), fusion=True)
    b16 = l.dt_hip_batch_new(p16.handle, 2, s.nb_in, W * H * 8)
    assert b16
    assert l.dt_hip_batch_set_file_output(b16, 4096) == abi.DT_HIP_INVALID_ARG
    assert "export_u16" in l.dt_hip_last_error().decode()
    assert l.dt_hip_batch_set_file_output(b16, 0) == 0  # off is what it is
    l.dt_hip_batch_free(b16)
    p16.close()
    b = l.dt_hip_batch_new(s.pipe.handle, 2, s.nb_in, s.nb_out)
    assert b
    for bad in (4, 7, s.nb_out + 1):
        assert l.dt_hip_batch_set_file_output(b, bad) == abi.DT_HIP_INVALID_ARG, bad
        assert str(bad) in l.dt_hip_last_error().decode()
    assert l.dt_hip_batch_set_file_output(b, s.nb_out) == 0
    # an unpinned and a misaligned host_out: refused with nothing in flight, and the next valid submit works
    pin_in, out = s.pin(s.nb_in), s.pin(s.nb_out + 16, FILL)
    pin_in[1][:] = s.frames[2].view(np.uint8).reshape(-1)
    plain = np.full(s.nb_out + 64, FILL, np.uint8)
    plain_ptr = plain.ctypes.data + (-plain.ctypes.data) % 16
    for what, ptr in (("unpinned", plain_ptr), ("misaligned", out[0] + 8)):
        assert l.dt_hip_batch_submit(b, pin_in[0], ptr) == abi.DT_HIP_INVALID_ARG, what
        assert l.dt_hip_last_error().decode().startswith("dt_hip_batch_submit: "), what
        assert l.dt_hip_batch_drain(b) == 0 and l.dt_hip_finish(0) == 1
        assert (plain == FILL).all() and (out[1] == FILL).all(), what
    assert l.dt_hip_batch_submit(b, pin_in[0], out[0]) == 0, l.dt_hip_last_error()
    assert l.dt_hip_batch_wait(b, 0) == 0
    n = len(s.want[2])
    assert _word(out[1]) == n and out[1][8:8 + n].tobytes() == s.want[2] and (out[1][8 + n:] == FILL).all()
    l.dt_hip_batch_free(b)
    s.unpin()


def test_mode_off_again_downloads_the_capacity(jpeg):
    """as tests/test_gpu_jpeg_pipe.py::test_batch_writer_reads_the_length_word: the writer sees out_bytes"""
    s, l = jpeg, jpeg.l
    wr = _Writer()
    b = l.dt_hip_batch_new(s.pipe.handle, 2, s.nb_in, s.nb_out)
    assert b and l.dt_hip_batch_set_writer(b, wr.cb, None) == 0
    assert l.dt_hip_batch_set_file_output(b, 4096) == 0
    assert l.dt_hip_batch_set_file_output(b, 0) == 0
    codes, outs = _stream(s, b, [0, 1, 2])
    assert codes == [0, 0, 0] and l.dt_hip_batch_drain(b) == 0
    n = C.c_size_t(0)
    assert l.dt_hip_batch_file_bytes(b, 0, C.byref(n)) == abi.DT_HIP_INVALID_ARG
    l.dt_hip_batch_free(b)
    assert [(c[0], c[1]) for c in wr.calls] == [(k, s.nb_out) for k in range(3)]
    for k, (_, _, got) in enumerate(wr.calls):
        assert got[:8] == np.uint64(len(s.want[k])).tobytes() and got[8:8 + len(s.want[k])] == s.want[k]
    s.unpin()


def test_read_file(jpeg):
    s, l = jpeg, jpeg.l
    s.d_in.upload(s.frames[2])
    s.pipe.process(s.d_in.ptr, s.d_out.ptr)
    assert s.pipe.read_file(s.d_out.ptr, s.nb_out) == s.want[2]
    # a staging buffer smaller than the file: the first call reports 8 + L, the second takes it
    assert len(s.want[2]) > 1024
    assert s.pipe.read_file(s.d_out.ptr, s.nb_out, staging_bytes=1024) == s.want[2]
    assert s.pipe.read_file(s.d_out.ptr, s.nb_out, staging_bytes=8) == s.want[2]
    # no file in the buffer: the encoder's refusal word
    d_none = lib.DeviceBuffer.from_numpy(0, np.full(64, 0xFF, np.uint8))
    with pytest.raises(lib.AnselHipError):
        s.pipe.read_file(d_none.ptr, 64)
    d_none.release()
