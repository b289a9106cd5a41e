#!/usr/bin/env python3
"""Time the PNG encoder (dt_hip_export_png, ansel_amd/csrc/png.hip) on one MI355X and print one JSON line.

    python tools/bench_png.py [--steps 10] [--sizes 24MP,100MP] [--depths 8,16] [--levels 1,5,9] [--no-libpng]

  encoder  on the light pipe's u8 / u16 frame (synthetic mosaic) resident in HBM, at each size, depth and level: ms per
           call (median of --steps, HIP events), ms per stage (tagged launches: png_filter, png_lz, png_tables,
           png_scan, png_emit = zero + emit + tail, png_idat = IDAT chunks + head), the file's bytes
  libpng   the same frame through libpng 1.6 with Ansel's settings (tests/native/png_ref.c) on one host thread per
           encode, the encodes side by side on threads of their own (at most 12; ctypes releases the GIL): ms and bytes

The line carries lib_sha16, the first 16 hex digits of the sha256 of the library that ran."""
import argparse
import ctypes as C
import json
from concurrent.futures import ThreadPoolExecutor
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ("png_filter", "png_lz", "png_tables", "png_scan", "png_emit", "png_idat")
FRAMES = {}  # (size, depth) -> RGBA numpy frame


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


def _libpng(key):
    """one libpng encode on the calling thread: (key, ms, bytes)"""
    import png_ref as pr
    size, depth, level = key
    t0 = time.perf_counter()
    n = len(pr.libpng_file(FRAMES[(size, depth)], level))
    return key, (time.perf_counter() - t0) * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="24MP,100MP")
    ap.add_argument("--depths", default="8,16")
    ap.add_argument("--levels", default="1,5,9")
    ap.add_argument("--no-libpng", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from ansel_amd import filmic, lib, params, pipe, synth
    l = lib.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lib.check(l.dt_hip_set_stream(0, C.c_void_p(stream.cuda_stream)), "dt_hip_set_stream")
    res = {"tool": "bench_png", "device": l.dt_hip_get_device_name(0).decode(),
           "lib_sha16": bench._sha16(os.path.join(ROOT, "ansel_amd", "libansel_hip.so")), "steps": args.steps}
    lut_host = params.srgb_encode_lut()
    lut = torch.from_numpy(lut_host).to(dev)
    co = params.unbounded_coeffs(lut_host)
    levels = [int(v) for v in args.levels.split(",")]
    enc = {}
    for size in args.sizes.split(","):
        w, h = synth.SIZES[size]
        raw = torch.from_numpy(synth.bayer_mosaic_tiled(w, h, seed=1).view(np.int16)).to(dev)
        for depth in [int(v) for v in args.depths.split(",")]:
            nodes = pipe.light_pipe_nodes(w, h, lut.data_ptr(), float(lut_host[0]), co, filmic=filmic.default_data())
            if depth == 8:
                nodes = nodes[:-1] + [pipe.Node("export_u8", None, nodes[-1].piece)]
            frame = torch.empty((h, w, 4), dtype=torch.uint8 if depth == 8 else torch.int16, device=dev)
            p = pipe.DevicePipe(0, nodes, fusion=True)
            p.process(raw.data_ptr(), frame.data_ptr())
            torch.cuda.synchronize()
            p.close()
            if not args.no_libpng:
                host = frame.cpu().numpy()
                FRAMES[(size, depth)] = host if depth == 8 else host.view(np.uint16)
            for level in levels:
                d = params.png(bpp=depth, compression=level)
                d.capacity = pipe.png_bound(w, h, d)
                out = torch.empty(d.capacity, dtype=torch.uint8, device=dev)
                fn = lambda: lib.check(l.dt_hip_export_png(0, w, h, C.byref(d), frame.data_ptr(), out.data_ptr()), "png")
                ms = _median_ms(torch, fn, args.steps)
                st = _stages(l, torch, fn, args.steps)
                n = int(out[:8].cpu().numpy().view(np.uint64)[0])
                enc["%s_%dbit_level%d" % (size, depth, level)] = {"ms": round(ms, 3), "stages_ms": st, "bytes": n,
                                                                   "capacity": d.capacity}
                del out
                torch.cuda.empty_cache()
            del frame
            torch.cuda.empty_cache()
        del raw
        torch.cuda.empty_cache()
    if not args.no_libpng:
        import png_ref as pr
        if pr.ref() is None:
            res["libpng"] = "not installed"
        else:
            keys = [(s, dp, lv) for (s, dp) in FRAMES for lv in levels]
            with ThreadPoolExecutor(min(12, len(keys))) as pool:
                for (s, dp, lv), ms, n in pool.map(_libpng, keys):
                    r = enc["%s_%dbit_level%d" % (s, dp, lv)]
                    r["libpng_1thread_ms"] = round(ms, 1)
                    r["libpng_bytes"] = n
                    r["bytes_over_libpng"] = round(r["bytes"] / n, 4)
    res["encoder"] = enc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
