#!/usr/bin/env python3
"""Time the JPEG encoder (dt_hip_export_jpeg, ansel_amd/csrc/jpeg.hip) on one MI355X and print one JSON line.

    python tools/bench_jpeg.py [--steps 10] [--sizes 24MP,100MP] [--no-pillow] [--no-batch]

  encoder  on the light pipe's u8 frame (synthetic mosaic) resident in HBM, at each size, for 4:4:4 q95 and 4:2:0 q90,
           optimize_coding on and off: ms per call (median of --steps, HIP events), ms per stage (tagged launches:
           jpeg_fdct, jpeg_stats, jpeg_tables, jpeg_lengths = lengths + scan, jpeg_emit = zero + emit, jpeg_stuff =
           count + scan + compact + headers), the file's bytes
  pillow   the same frame through Pillow's libjpeg(-turbo) on one host thread, same settings (one encode)
  download the capacity (dt_hip_jpeg_bound) copied device -> pinned host: what the batch moves per frame
  batch    the 100 MP light pipe + export_jpeg (4:4:4 q95, optimized) in a batch of 8 frames, depth 2, whose writer reads
           the length word and writes the file: ms per frame

The line carries lib_sha16, the first 16 hex digits of the sha256 of the library that ran."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("jpeg_fdct", "jpeg_stats", "jpeg_tables", "jpeg_lengths", "jpeg_emit", "jpeg_stuff")
MODES = (("444_q95", 95, 0), ("420_q90", 90, 2))


def _median_ms(torch, fn, steps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2]


def _stages(l, torch, fn, steps):
    fn()
    torch.cuda.synchronize()
    l.dt_hip_events_reset(0)
    l.dt_hip_events_enable(0, 1)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    l.dt_hip_events_enable(0, 0)
    tags, tms, cnt = (C.c_char_p * 64)(), (C.c_float * 64)(), (C.c_int * 64)()
    nk = l.dt_hip_events_profiling(0, tags, tms, cnt, 64)
    got = {tags[i].decode(): tms[i] / steps for i in range(min(nk, 64))}
    return {k: round(got[k], 4) for k in STAGES if k in got}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="24MP,100MP")
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--no-batch", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from ansel_amd import abi, filmic, lib, params, pipe, synth
    l = lib.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lib.check(l.dt_hip_set_stream(0, C.c_void_p(stream.cuda_stream)), "dt_hip_set_stream")
    res = {"tool": "bench_jpeg", "device": l.dt_hip_get_device_name(0).decode(),
           "lib_sha16": bench._sha16(os.path.join(ROOT, "ansel_amd", "libansel_hip.so")), "steps": args.steps}
    lut_host = params.srgb_encode_lut()
    lut = torch.from_numpy(lut_host).to(dev)
    co = params.unbounded_coeffs(lut_host)

    enc = {}
    for size in args.sizes.split(","):
        w, h = synth.SIZES[size]
        raw = torch.from_numpy(synth.bayer_mosaic_tiled(w, h, seed=1).view(np.int16)).to(dev)
        nodes = pipe.light_pipe_nodes(w, h, lut.data_ptr(), float(lut_host[0]), co, filmic=filmic.default_data())
        nodes = nodes[:-1] + [pipe.Node("export_u8", None, nodes[-1].piece)]
        u8 = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        p = pipe.DevicePipe(0, nodes, fusion=True)
        p.process(raw.data_ptr(), u8.data_ptr())
        torch.cuda.synchronize()
        p.close()
        del raw
        host_u8 = u8.cpu().numpy() if not args.no_pillow else None
        row = {}
        for name, q, ss in MODES:
            for opt in (0, 1):
                d = abi.JpegData(quality=q, subsampling=ss, optimize_coding=opt, density_unit=0, x_density=1, y_density=1)
                d.capacity = pipe.jpeg_bound(w, h, d)
                out = torch.empty(d.capacity, dtype=torch.uint8, device=dev)
                fn = lambda: lib.check(l.dt_hip_export_jpeg(0, w, h, C.byref(d), u8.data_ptr(), out.data_ptr()), "jpeg")
                ms = _median_ms(torch, fn, args.steps)
                st = _stages(l, torch, fn, args.steps)
                n = int(out[:8].cpu().numpy().view(np.uint64)[0])
                r = {"ms": round(ms, 3), "stages_ms": st, "bytes": n, "capacity": d.capacity}
                if opt == 1:
                    pin = torch.empty(d.capacity, dtype=torch.uint8, pin_memory=True)
                    r["download_capacity_ms"] = round(_median_ms(torch, lambda: pin.copy_(out, non_blocking=True), 3), 3)
                    del pin
                if host_u8 is not None:
                    from PIL import Image
                    im = Image.fromarray(host_u8[..., :3])
                    b = io.BytesIO()
                    t0 = time.perf_counter()
                    im.save(b, "JPEG", quality=q, subsampling=ss, optimize=bool(opt))
                    r["pillow_1thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    r["pillow_bytes_equal"] = b.getvalue() == bytes(out[8:8 + n].cpu().numpy())
                row["%s_opt%d" % (name, opt)] = r
                del out
        enc[size] = row
        del u8
        torch.cuda.empty_cache()
    res["encoder"] = enc

    if not args.no_batch:
        w, h = synth.SIZES["100MP"]
        jd = params.jpeg(95)
        jd.capacity = pipe.jpeg_bound(w, h, jd)
        nodes = pipe.with_jpeg(pipe.light_pipe_nodes(w, h, lut.data_ptr(), float(lut_host[0]), co,
                                                     filmic=filmic.default_data()), jd)
        p = pipe.DevicePipe(0, nodes, fusion=True)
        raw = synth.bayer_mosaic_tiled(w, h, seed=1)
        nb_in, nb_out, depth, nframes = w * h * 2, jd.capacity, 2, 8
        pin_in = [l.dt_hip_alloc_host_pinned(nb_in) for _ in range(depth)]
        pin_out = [l.dt_hip_alloc_host_pinned(nb_out) for _ in range(depth)]
        for ptr in pin_in:
            C.memmove(ptr, raw.ctypes.data, nb_in)
        tmp = tempfile.mkdtemp()
        sizes = []

        def write_image(user, seq, host_out, nbytes):
            n = C.c_uint64.from_address(host_out).value
            if n + 8 > nbytes:
                return 1
            with open(os.path.join(tmp, "f%d.jpg" % (seq % 2)), "wb") as f:
                f.write(C.string_at(host_out + 8, n))
            sizes.append(n)
            return 0

        cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_size_t)(write_image)
        b = l.dt_hip_batch_new(p.handle, depth, nb_in, nb_out)
        assert b and l.dt_hip_batch_set_writer(b, cb, None) == 0
        t0 = None
        for k in range(nframes + 1):   # frame 0 warms up
            if k == 1:
                assert l.dt_hip_batch_drain(b) == 0
                t0 = time.perf_counter()
            if k >= depth:
                assert l.dt_hip_batch_wait(b, k % depth) == 0
            assert l.dt_hip_batch_submit(b, pin_in[k % depth], pin_out[k % depth]) >= 0, l.dt_hip_last_error()
        assert l.dt_hip_batch_drain(b) == 0
        res["batch_100MP_light_jpeg"] = {"ms_per_frame": round((time.perf_counter() - t0) / nframes * 1e3, 2),
                                         "frames": nframes, "depth": depth, "file_bytes": sizes[-1],
                                         "capacity": nb_out}
        l.dt_hip_batch_free(b)
        for ptr in pin_in + pin_out:
            l.dt_hip_free_host_pinned(ptr)
        p.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
