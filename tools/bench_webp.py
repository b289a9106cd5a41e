#!/usr/bin/env python3
"""Time the lossless WebP encoder (dt_hip_export_webp, ansel_amd/csrc/webp.hip) on one MI355X and print one JSON line.

    python tools/bench_webp.py [--steps 10] [--sizes 24MP,100MP] [--levels 1,6] [--no-libwebp] [--no-flat]

  encoder  on the light pipe's u8 frame (synthetic mosaic) resident in HBM, at each size and level: ms per call (median
           of --steps, HIP events), ms per stage (tagged launches: webp_predict, webp_lz, webp_tables, webp_scan = count
           + scan, webp_emit = zero + head + groups + tokens, webp_copy), the file's bytes; and the bytes of our own
           8-bit PNG at level 5 of the same frame
  flat     the matcher's worst case, a frame of one colour at each size and level 6: every position matches up to the
           longest reference (4096 pixels), so every thread compares that many pixels; ms per call, stages, bytes
  libwebp  the same frame through Pillow's libwebp, lossless, at its default (quality 75, method 4) and its fastest
           setting (quality 0, method 0), one encode after the other on one host thread: ms and bytes

The line carries lib_sha16, the first 16 hex digits of the sha256 of the library that ran."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ("webp_predict", "webp_lz", "webp_tables", "webp_scan", "webp_emit", "webp_copy")
LIBWEBP = {"default": dict(quality=75, method=4), "fastest": dict(quality=0, method=0)}


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


def _libwebp(frame, setting):
    """one lossless libwebp encode of the frame's RGB on the calling thread: (ms, bytes)"""
    import io
    from PIL import Image
    im = Image.fromarray(frame[..., :3])
    b = io.BytesIO()
    t0 = time.perf_counter()
    im.save(b, "WEBP", lossless=True, **LIBWEBP[setting])
    return (time.perf_counter() - t0) * 1e3, len(b.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="24MP,100MP")
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--no-libwebp", action="store_true")
    ap.add_argument("--no-flat", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from ansel_amd import filmic, lib, params, pipe, synth
    l = lib.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lib.check(l.dt_hip_set_stream(0, C.c_void_p(stream.cuda_stream)), "dt_hip_set_stream")
    res = {"tool": "bench_webp", "device": l.dt_hip_get_device_name(0).decode(),
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
        frame = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        p = pipe.DevicePipe(0, nodes, fusion=True)
        p.process(raw.data_ptr(), frame.data_ptr())
        torch.cuda.synchronize()
        p.close()
        del raw
        pd = params.png(bpp=8, compression=5)
        pd.capacity = pipe.png_bound(w, h, pd)
        out = torch.empty(pd.capacity, dtype=torch.uint8, device=dev)
        lib.check(l.dt_hip_export_png(0, w, h, C.byref(pd), frame.data_ptr(), out.data_ptr()), "png")
        torch.cuda.synchronize()
        png_bytes = int(out[:8].cpu().numpy().view(np.uint64)[0])
        del out
        torch.cuda.empty_cache()
        for level in [int(v) for v in args.levels.split(",")]:
            d = params.webp(level=level)
            d.capacity = pipe.webp_bound(w, h, d)
            out = torch.empty(d.capacity, dtype=torch.uint8, device=dev)
            fn = lambda: lib.check(l.dt_hip_export_webp(0, w, h, C.byref(d), frame.data_ptr(), out.data_ptr()), "webp")
            ms = _median_ms(torch, fn, args.steps)
            st = _stages(l, torch, fn, args.steps)
            n = int(out[:8].cpu().numpy().view(np.uint64)[0])
            enc["%s_level%d" % (size, level)] = {"ms": round(ms, 3), "stages_ms": st, "bytes": n, "capacity": d.capacity,
                                                 "png_level5_bytes": png_bytes, "bytes_over_png": round(n / png_bytes, 4)}
            del out
            torch.cuda.empty_cache()
        if not args.no_flat:
            flat = torch.full((h, w, 4), 181, dtype=torch.uint8, device=dev)
            d = params.webp(level=6)
            d.capacity = pipe.webp_bound(w, h, d)
            out = torch.empty(d.capacity, dtype=torch.uint8, device=dev)
            fn = lambda: lib.check(l.dt_hip_export_webp(0, w, h, C.byref(d), flat.data_ptr(), out.data_ptr()), "webp")
            ms = _median_ms(torch, fn, min(args.steps, 3))
            st = _stages(l, torch, fn, min(args.steps, 3))
            enc["%s_flat_level6" % size] = {"ms": round(ms, 3), "stages_ms": st,
                                            "bytes": int(out[:8].cpu().numpy().view(np.uint64)[0])}
            del out, flat
            torch.cuda.empty_cache()
        if not args.no_libwebp:
            host = frame.cpu().numpy()
            for setting in LIBWEBP:
                ms, n = _libwebp(host, setting)
                for level in [int(v) for v in args.levels.split(",")]:
                    r = enc["%s_level%d" % (size, level)]
                    r["libwebp_%s_1thread_ms" % setting] = round(ms, 1)
                    r["libwebp_%s_bytes" % setting] = n
                    r["bytes_over_libwebp_%s" % setting] = round(r["bytes"] / n, 4)
        del frame
        torch.cuda.empty_cache()
    res["encoder"] = enc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
