#!/usr/bin/env python3
"""A batch of exported files on one MI355X: the download of the whole capacity against the download of the file
(dt_hip_batch_set_file_output(), ansel_amd/csrc/file_copy.hip).  Prints one JSON line.

    python tools/bench_batch_files.py [--sizes 24MP,100MP] [--formats jpeg,png,tiff,webp] [--frames 20] [--warmup 5]
                                      [--repeats 3] [--groups 16,64,256]

For every size and format, the light pipe + the encoder (jpeg: q95 4:4:4; png: 8 bits, level 5; tiff: 8 bits, uncompressed
-- the largest file; webp: lossless, level 6):

  batch    (--repeats 0: left out) depth 2, a writer that only reads the length; --warmup frames, then --frames timed
           ones; the two modes take turns inside every repeat, so both see the same machine: ms a frame per repeat, the median and the spread (max - min)
           per mode.  In file mode the pinned host buffers hold 8 + L rounded up to 1 MiB, not the capacity.
  copy     file_to_host on the frame's file alone, by events (median of 5): ms and GB/s -- and, for comparison,
           hipMemcpyAsync of the same 8 + L bytes into the same pinned buffer (the host knows L here; in the batch it
           does not)
  legs     upload (hipMemcpyAsync of the mosaic) and kernels (pipe + encoder) alone, by events: what bounds a frame
  --groups with the measuring build (ANSEL_HIP_LIB=ansel_amd/libansel_hip_measuring.so): the copy at each number of
           workgroups (the product's number is a constant: FC_GROUPS of file_copy.hip)

The line carries lib_sha16, the first 16 hex digits of the sha256 of the library that ran."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _event_ms(torch, fn, steps=5):
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
    return _median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="24MP,100MP")
    ap.add_argument("--formats", default="jpeg,png,tiff,webp")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--groups", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from ansel_amd import filmic, lib, params, pipe, synth
    l = lib.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lib.check(l.dt_hip_set_stream(0, C.c_void_p(stream.cuda_stream)), "dt_hip_set_stream")
    measuring = "measuring" in os.path.basename(lib.LIB_PATH)
    groups = [int(g) for g in args.groups.split(",") if g]
    if groups and not measuring:
        raise SystemExit("--groups needs the measuring build: ANSEL_HIP_LIB=ansel_amd/libansel_hip_measuring.so")
    res = {"tool": "bench_batch_files", "device": l.dt_hip_get_device_name(0).decode(), "lib": os.path.basename(lib.LIB_PATH),
           "lib_sha16": bench._sha16(lib.LIB_PATH), "frames": args.frames, "warmup": args.warmup, "depth": 2, "rows": {}}
    lut_host = params.srgb_encode_lut()
    lut = torch.from_numpy(lut_host).to(dev)
    co = params.unbounded_coeffs(lut_host)
    formats = {"jpeg": (lambda: params.jpeg(95), pipe.with_jpeg, pipe.jpeg_bound),
               "png": (lambda: params.png(8), pipe.with_png, pipe.png_bound),
               "tiff": (lambda: params.tiff(bpp=8, compress=0), pipe.with_tiff, pipe.tiff_bound),
               "webp": (lambda: params.webp(), pipe.with_webp, pipe.webp_bound)}
    WRITER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_size_t)
    seen = []

    def write_image(user, seq, host_out, nbytes):
        n = C.c_uint64.from_address(host_out).value  # the writer only reads the length
        seen.append((n, nbytes))
        return 0 if n + 8 <= nbytes else 1

    cb = WRITER(write_image)
    depth = 2
    for size in args.sizes.split(","):
        w, h = synth.SIZES[size]
        raw = synth.bayer_mosaic_tiled(w, h, seed=1)
        nb_in = w * h * 2
        pin_in = l.dt_hip_alloc_host_pinned(nb_in)
        assert pin_in
        C.memmove(pin_in, raw.ctypes.data, nb_in)
        d_in = torch.from_numpy(raw.view(np.int16)).to(dev)
        del raw
        for fmt in args.formats.split(","):
            make, with_fmt, bound = formats[fmt]
            data = make()
            data.capacity = bound(w, h, data)
            cap = int(data.capacity)
            nodes = with_fmt(pipe.light_pipe_nodes(w, h, lut.data_ptr(), float(lut_host[0]), co, filmic=filmic.default_data()), data)
            p = pipe.DevicePipe(0, nodes, fusion=True)
            d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
            row = {"capacity": cap}
            # the legs alone
            row["kernels_ms"] = round(_event_ms(torch, lambda: p.process(d_in.data_ptr(), d_out.data_ptr())), 3)
            row["upload_ms"] = round(_event_ms(torch, lambda: lib.check(
                l.dt_hip_write_buffer_to_device(0, pin_in, d_in.data_ptr(), 0, nb_in, 0), "upload")), 3)
            L = len(p.read_file(d_out.data_ptr(), cap))
            row["L"] = L
            host_bytes = min(cap, (8 + L + (1 << 20) - 1) & ~((1 << 20) - 1))
            row["host_bytes"] = host_bytes
            pin_cap = [l.dt_hip_alloc_host_pinned(cap) for _ in range(depth if args.repeats > 0 else 0)]
            pin_file = [l.dt_hip_alloc_host_pinned(host_bytes) for _ in range(depth)]
            assert all(pin_cap) and all(pin_file), "no pinned memory for %s %s" % (size, fmt)
            # the copy alone
            fth = lambda: lib.check(l.dt_hip_read_file_to_host(0, d_out.data_ptr(), cap, pin_file[0], host_bytes), "file_to_host")
            ms = _event_ms(torch, fth)
            row["file_to_host_ms"] = round(ms, 4)
            row["file_to_host_GBps"] = round((8 + L) / ms / 1e6, 2)
            ms = _event_ms(torch, lambda: lib.check(
                l.dt_hip_read_buffer_from_device(0, pin_file[0], d_out.data_ptr(), 0, 8 + L, 0), "memcpy"))
            row["memcpy_same_bytes_ms"] = round(ms, 4)
            row["memcpy_same_bytes_GBps"] = round((8 + L) / ms / 1e6, 2)
            if groups:
                row["file_to_host_ms_by_groups"] = {}
                for g in groups:
                    os.environ["ANSEL_HIP_FILE_COPY_GROUPS"] = str(g)
                    row["file_to_host_ms_by_groups"][str(g)] = round(_event_ms(torch, fth), 4)
                del os.environ["ANSEL_HIP_FILE_COPY_GROUPS"]
            if args.repeats > 0:
                # the batch: the two modes take turns
                b = l.dt_hip_batch_new(p.handle, depth, nb_in, cap)
                assert b and l.dt_hip_batch_set_writer(b, cb, None) == 0
                per = {"capacity": [], "file": []}
                for _ in range(args.repeats):
                    for mode in ("capacity", "file"):
                        lib.check(l.dt_hip_batch_set_file_output(b, host_bytes if mode == "file" else 0), "set_file_output")
                        outs = pin_file if mode == "file" else pin_cap
                        t0 = None
                        for k in range(args.warmup + args.frames):
                            if k == args.warmup:
                                assert l.dt_hip_batch_drain(b) == 0
                                t0 = time.perf_counter()
                            if k >= depth:
                                assert l.dt_hip_batch_wait(b, k % depth) == 0, l.dt_hip_last_error()
                            assert l.dt_hip_batch_submit(b, pin_in, outs[k % depth]) >= 0, l.dt_hip_last_error()
                        assert l.dt_hip_batch_drain(b) == 0, l.dt_hip_last_error()
                        per[mode].append((time.perf_counter() - t0) / args.frames * 1e3)
                        assert seen[-1] == (L, 8 + L if mode == "file" else cap), seen[-1]
                l.dt_hip_batch_free(b)
                for mode, v in per.items():
                    row[mode + "_mode_ms_per_frame"] = {"repeats": [round(x, 2) for x in v], "median": round(_median(v), 2),
                                                        "spread": round(max(v) - min(v), 2)}
                row["file_mode_gain_ms"] = round(_median(per["capacity"]) - _median(per["file"]), 2)
                legs = {"upload": row["upload_ms"], "kernels": row["kernels_ms"], "download": row["file_to_host_ms"]}
                row["file_mode_longest_leg"] = max(legs, key=legs.get)
            for ptr in pin_cap + pin_file:
                l.dt_hip_free_host_pinned(ptr)
            p.close()
            del d_out
            torch.cuda.empty_cache()
            res["rows"]["%s_%s" % (size, fmt)] = row
            print("# %s %s: %s" % (size, fmt, json.dumps(row)), file=sys.stderr, flush=True)
        l.dt_hip_free_host_pinned(pin_in)
        del d_in
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
