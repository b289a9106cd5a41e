#!/usr/bin/env python3
"""Time the TIFF encoder (dt_hip_export_tiff, ansel_amd/csrc/tiff.hip) on one MI355X and print one JSON line.

    python tools/bench_tiff.py [--steps 10] [--sizes 24MP,100MP] [--bpps 8,16,32] [--no-libtiff]

  encoder  on the light pipe's u8 / u16 / float frame (synthetic mosaic) resident in HBM, at each size and depth, without
           compression and with deflate at level 6 and the depth's predictor (2, or 3 for floats), libtiff's default rows
           per strip: ms per call (median of --steps, HIP events), ms per stage (tagged launches: tiff_rows, tiff_lz,
           tiff_tables, tiff_scan, tiff_emit = zero + emit + tail, tiff_copy), the file's bytes and its strips
  png      the PNG encoder at level 6 on the same u8 / u16 frame, for comparison: ms and bytes
  libtiff  the same frame through libtiff (tests/tiff_ref.py, ctypes) with the same settings on one host thread per
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGES = ("tiff_rows", "tiff_lz", "tiff_tables", "tiff_scan", "tiff_emit", "tiff_copy")
FRAMES = {}  # (size, bpp) -> RGBA numpy frame (32 bits: the floats' bits)
COMPRESS = {"none": 0, "deflate6": 2}  # params.tiff(compress=...)


def _libtiff(key):
    """one libtiff encode on the calling thread: (key, ms, bytes)"""
    import tiff_ref as tr
    from ansel_amd import params
    size, bpp, mode = key
    d = params.tiff(bpp=bpp, compress=COMPRESS[mode], level=6)
    t0 = time.perf_counter()
    n = len(tr.libtiff_file(FRAMES[(size, bpp)], d))
    return key, (time.perf_counter() - t0) * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="24MP,100MP")
    ap.add_argument("--bpps", default="8,16,32")
    ap.add_argument("--no-libtiff", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from bench_png import _median_ms
    from ansel_amd import filmic, lib, params, pipe, synth
    l = lib.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lib.check(l.dt_hip_set_stream(0, C.c_void_p(stream.cuda_stream)), "dt_hip_set_stream")
    res = {"tool": "bench_tiff", "device": l.dt_hip_get_device_name(0).decode(),
           "lib_sha16": bench._sha16(os.path.join(ROOT, "ansel_amd", "libansel_hip.so")), "steps": args.steps}
    lut_host = params.srgb_encode_lut()
    lut = torch.from_numpy(lut_host).to(dev)
    co = params.unbounded_coeffs(lut_host)

    def stages(fn):
        fn()
        torch.cuda.synchronize()
        l.dt_hip_events_reset(0)
        l.dt_hip_events_enable(0, 1)
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        l.dt_hip_events_enable(0, 0)
        tags, tms, cnt = (C.c_char_p * 64)(), (C.c_float * 64)(), (C.c_int * 64)()
        nk = l.dt_hip_events_profiling(0, tags, tms, cnt, 64)
        got = {tags[i].decode(): tms[i] / args.steps for i in range(min(nk, 64))}
        return {k: round(got[k], 4) for k in STAGES if k in got}

    enc = {}
    for size in args.sizes.split(","):
        w, h = synth.SIZES[size]
        raw = torch.from_numpy(synth.bayer_mosaic_tiled(w, h, seed=1).view(np.int16)).to(dev)
        for bpp in [int(v) for v in args.bpps.split(",")]:
            nodes = pipe.light_pipe_nodes(w, h, lut.data_ptr(), float(lut_host[0]), co, filmic=filmic.default_data())
            nodes = {8: nodes[:-1] + [pipe.Node("export_u8", None, nodes[-1].piece)], 16: nodes, 32: nodes[:-1]}[bpp]
            frame = torch.empty((h, w, 4), dtype={8: torch.uint8, 16: torch.int16, 32: torch.float32}[bpp], device=dev)
            p = pipe.DevicePipe(0, nodes, fusion=True)
            p.process(raw.data_ptr(), frame.data_ptr())
            torch.cuda.synchronize()
            p.close()
            if not args.no_libtiff:
                FRAMES[(size, bpp)] = frame.cpu().numpy().view({8: np.uint8, 16: np.uint16, 32: np.uint32}[bpp])
            for mode, compress in COMPRESS.items():
                d = params.tiff(bpp=bpp, compress=compress, level=6)
                d.capacity = pipe.tiff_bound(w, h, d)
                out = torch.empty(d.capacity, dtype=torch.uint8, device=dev)
                fn = lambda: lib.check(l.dt_hip_export_tiff(0, w, h, C.byref(d), frame.data_ptr(), out.data_ptr()), "tiff")
                ms = _median_ms(torch, fn, args.steps)
                st = stages(fn)
                n = int(out[:8].cpu().numpy().view(np.uint64)[0])
                rb = w * 3 * bpp // 8
                rows = max(1, 8192 // rb)
                enc["%s_%dbit_%s" % (size, bpp, mode)] = {"ms": round(ms, 3), "stages_ms": st, "bytes": n, "capacity": d.capacity,
                                                          "strips": (h + rows - 1) // rows, "strip_bytes": rows * rb}
                del out
                torch.cuda.empty_cache()
            if bpp != 32:
                d = params.png(bpp=bpp, compression=6)
                d.capacity = pipe.png_bound(w, h, d)
                out = torch.empty(d.capacity, dtype=torch.uint8, device=dev)
                fn = lambda: lib.check(l.dt_hip_export_png(0, w, h, C.byref(d), frame.data_ptr(), out.data_ptr()), "png")
                ms = _median_ms(torch, fn, args.steps)
                enc["%s_%dbit_png6" % (size, bpp)] = {"ms": round(ms, 3), "bytes": int(out[:8].cpu().numpy().view(np.uint64)[0])}
                del out
            del frame
            torch.cuda.empty_cache()
        del raw
        torch.cuda.empty_cache()
    if not args.no_libtiff:
        import tiff_ref as tr
        if tr.libtiff() is None:
            res["libtiff"] = "not installed"
        else:
            res["libtiff"] = tr.libtiff_name()
            keys = [(s, b, m) for (s, b) in FRAMES for m in COMPRESS]
            with ThreadPoolExecutor(min(12, len(keys))) as pool:
                for (s, b, m), ms, n in pool.map(_libtiff, keys):
                    r = enc["%s_%dbit_%s" % (s, b, m)]
                    r["libtiff_1thread_ms"] = round(ms, 1)
                    r["libtiff_bytes"] = n
                    r["bytes_over_libtiff"] = round(r["bytes"] / n, 4)
    res["encoder"] = enc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
