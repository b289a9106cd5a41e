#!/usr/bin/env python3
"""Time the flip module (orientation) on one MI355X and print one JSON line.

    python tools/bench_flip.py [--steps 10] [--sizes 24MP,100MP] [--no-pipes]

  kernel   dt_hip_iop_flip_process() alone on a float4 plane resident in HBM, every orientation, at each size: ms (median
           of --steps launches, HIP events) and GB/s at the 32 B/px the permutation moves, against the device-to-device
           copy rate measured in the same run (bench.py's measured_ceiling())
  pipes    the full pipe (bench.py's timed workload: denoise (profiled), diffuse or sharpen, non-local means, local contrast)
           and the light pipe at 100 MP, each with no flip node and with orientation 6 behind its last module before
           exposure: ms per frame (median of --steps) and the difference

The line carries lib_sha16, the first 16 hex digits of the sha256 of the library that ran."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="24MP,100MP")
    ap.add_argument("--no-pipes", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from ansel_amd import abi, lib, params, pipe, synth
    l = lib.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lib.check(l.dt_hip_set_stream(0, C.c_void_p(stream.cuda_stream)), "dt_hip_set_stream")
    res = {"tool": "bench_flip", "device": l.dt_hip_get_device_name(0).decode(),
           "lib_sha16": bench._sha16(os.path.join(ROOT, "ansel_amd", "libansel_hip.so")), "steps": args.steps}
    res["copy_ceiling"] = bench.measured_ceiling(torch, dev)
    copy = res["copy_ceiling"]["copy_GBs"]

    kern = {}
    for size in args.sizes.split(","):
        w, h = synth.SIZES[size]
        src = torch.empty((h, w, 4), dtype=torch.float32, device=dev).uniform_()
        dst = torch.empty_like(src)
        row = {}
        for o in range(8):
            ow, oh = params.oriented_size(w, h, o)
            piece = abi.Piece.make(w, h, channels=4, roi_out=abi.Roi.make(0, 0, ow, oh))
            d = abi.FlipData(o)
            fn = lambda: lib.check(l.dt_hip_iop_flip_process(0, C.byref(piece), C.byref(d), src.data_ptr(), dst.data_ptr()), "flip")
            ms = _median_ms(torch, fn, args.steps)
            gbs = 32.0 * w * h / (ms * 1e-3) / 1e9
            row[str(o)] = {"ms": round(ms, 4), "GBps": round(gbs, 1), "frac_of_copy": round(gbs / copy, 3)}
        kern[size] = row
        del src, dst
        torch.cuda.empty_cache()
    res["kernel"] = kern

    if not args.no_pipes:
        w, h = synth.SIZES["100MP"]
        lut_host = params.srgb_encode_lut()
        lut = torch.from_numpy(lut_host).to(dev)
        raw = torch.from_numpy(synth.bayer_mosaic_tiled(w, h, seed=1).view(np.int16)).to(dev)
        out = torch.empty((max(w, h) * min(w, h) * 4,), dtype=torch.int16, device=dev)
        pipes = {}
        for which, after in (("full", "denoiseprofile"), ("light", "demosaic")):
            row = {}
            for o in (None, 6):
                nodes = bench.build_pipe(w, h, lut.data_ptr(), lut_host, True, which)
                if o is not None:
                    nodes = pipe.insert_flip(nodes, after, o)
                p = pipe.DevicePipe(0, nodes, fusion=True)
                ms = _median_ms(torch, lambda: p.process(raw.data_ptr(), out.data_ptr()), args.steps)
                row["no_flip" if o is None else "orientation_%d" % o] = {"ms": round(ms, 3), "groups": p.num_groups}
                p.close()
            row["delta_ms"] = round(row["orientation_6"]["ms"] - row["no_flip"]["ms"], 3)
            pipes[which + "_100MP"] = row
        res["pipes"] = pipes
    print(json.dumps(res))


if __name__ == "__main__":
    main()
