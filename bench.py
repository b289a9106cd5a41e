#!/usr/bin/env python3
"""bench.py -- MPix/s of the full-resolution export pixelpipe on MI355X, with the HBM roofline of
the dominant kernel and (--full) the reference's CPU path timed beside it.

    python bench.py --gpus 1 --steps 10 --warmup 2
    python bench.py --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one pass of the export pipe over one synthetic raw frame: every module of the pipe,
input mosaic already resident in HBM, output RGBA u16 left in HBM.  Workload (config.workload):
BASELINE.json's metric is "MPix/s full export pixelpipe (100 MP raw)": the FULL pipe -- config 3's
module list (rawprepare, white balance, highlight clip, RCD demosaic, denoise (profiled) wavelets,
exposure, colorin, color calibration, diffuse or sharpen, non-local means and local contrast
(bilateral grid) in Lab, filmic RGB, colorout, float->u16), every heavy iop the north star names, all at
module defaults -- on the 100 MP frame (11648 x 8736 RGGB).  `--pipe light` times config 2's module list
(no denoise / diffuse / local contrast) instead; at N = 1 the default run also carries it as `config.light_pipe`.

N > 1: one process per GPU, one frame per GPU (BASELINE.json config 5: batch export shards
frames across GPUs, no data-path collective) -> "scaling": "weak"; value = N frames / max time.
--mode tiled is BASELINE.json config 4 instead: ONE frame cut into N row bands (ansel_amd/tiled.py),
an 8-byte all-reduce and one 9-row halo send/recv per frame -> "scaling": "strong".
Started WITHOUT a launcher (`python bench.py --gpus N`, WORLD_SIZE unset) it spawns its own N ranks under
torch.distributed.run on 127.0.0.1; a launcher whose WORLD_SIZE disagrees with --gpus is an error.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: `value`, `ms_per_step`, the
per-kernel times of the timed steps (HIP events) and the roofline figures derived from them and the committed counter tables.
Everything else runs only with --full, after the timed region.  Besides `value` the line then carries, at N = 1:
`config.light_pipe` -- config 2's module list on the SAME 100 MP frame, timed in the same run (and, as
`config.light_pipe.with_amaze`, once more with AMaZE in RCD's place); `config.default_diffuse`, `config.full_pipe_24MP`, the
host-to-host legs and `roofline.peak_measured` (a copy / triad / fill / sum measured on the device); `verified` -- the output
buffer the timed steps wrote, compared word for word with the oracle's chain after the timed region (the oracle is the checker
here, never the thing measured); `cpu_baseline` -- the reference's own code on the host cores, same module chain.  N > 1 and
--mode tiled / bands check their ranks' or bands' outputs with --full as well.

PyTorch is used for device memory, the stream and torch.distributed only; all pixel work goes
through the C-ABI of libansel_hip.so (include/ansel_hip.h).  There is no CPU fallback.

--dump-outputs DIR writes what the last timed step exported (the RGBA u16 words, as float32 .npy files; a fixed seeded
sample of the pixels above 4 MP) so that two builds run with the same arguments can be compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", default="100MP", help="24MP | 45MP | 60MP | 100MP | WxH")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run what the headline figure does not need: the comparison with the oracle, "
                         "the other pipes and frame sizes, the measured copy ceiling, the host-to-host legs and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-verify", action="store_true",
                    help="--full without the post-timing comparison of the timed output buffer with the oracle chain")
    ap.add_argument("--no-light-pipe", action="store_true",
                    help="--full without the config.light_pipe, config.default_diffuse and config.full_pipe_24MP legs")
    ap.add_argument("--light-steps", type=int, default=10, help="timed steps of the config.light_pipe leg")
    ap.add_argument("--no-host-legs", action="store_true",
                    help="--full without the PCIe-inclusive host-to-host measurements (never `value`)")
    ap.add_argument("--no-fusion", action="store_true", help="one launch per module (A/B against the fused executor)")
    ap.add_argument("--cpu-sample", default=None,
                    help="frame size of the bounded CPU sample (default: 24MP)")
    ap.add_argument("--pipe", default="full", choices=("full", "light", "denoise"),
                    help="full = the metric's workload: config 3's modules (denoise (profiled) wavelets, diffuse or sharpen, "
                         "non-local means) + local contrast (bilateral grid); light = BASELINE.json config 2; "
                         "denoise = full without local contrast (round 2's config.full_pipe)")
    ap.add_argument("--mode", default="batch", choices=("batch", "tiled", "bands"),
                    help="N > 1: batch = one frame per GPU (config 5, weak); tiled = ONE frame cut into row bands, "
                         "one band per GPU and rank, halo rows exchanged over RCCL (config 4, strong); bands = the same walk "
                         "from ONE process through dt_hip_pipe_process_bands(): one host thread per band, peer copies "
                         "between the devices ordered by events (no launcher; --gpus = devices, --bands = bands)")
    ap.add_argument("--bands", type=int, default=0, help="--mode bands: number of row bands (default: one per device); more "
                                                        "bands than devices puts several on a device (a one-GPU dry run)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the exported RGBA words of the last step to DIR/*.npy (float32; the whole "
                         "frame up to 4 MP, a fixed seeded sample of its pixels above that), so that two builds can be compared")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def frame_size(name):
    from ansel_amd import synth
    if name in synth.SIZES:
        return synth.SIZES[name]
    w, h = name.lower().split("x")
    return int(w), int(h)


# diffuse or sharpen in the full pipe: the reference's "lens deblur: soft" preset (src/iop/diffuse.c:304-325: four speeds, orders 1
# and 3 along the isophotes, radius 8 -> 5 scales) cut from its 8 iterations to 2 -- 10 B-spline analyses + 10 PDE passes, 960 of the
# pipe's 2 114 algorithmic B/px.  The module's $DEFAULT (diffuse.c:79-98) is 1 iteration with all four speeds 0: the line carries
# that pipe too, as config.default_diffuse.
DIFFUSE_TIMED = ("lens_deblur_soft", 2)
DIFFUSE_DEFAULT = ("default", 1)


def build_pipe(width, height, lut_ptr, lut, with_filmic, which="light", demosaic_method=None, diffuse=DIFFUSE_TIMED):
    from ansel_amd import abi, params, pipe
    filmic = None
    if with_filmic:
        from ansel_amd import filmic as fm
        filmic = fm.default_data()
    coeffs = params.unbounded_coeffs(lut)
    if which in ("full", "denoise"):
        # BASELINE.json config 3: + denoise (profiled wavelets) + non-local means + diffuse or sharpen; "full" also
        # runs local contrast (bilateral grid) behind non-local means, inside the same Lab section
        return pipe.denoise_pipe_nodes(width, height, lut_ptr, float(lut[0]), coeffs, filmic=filmic, with_nlmeans=True,
                                       with_bilat=(which == "full"), diffuse_preset=diffuse[0], diffuse_iterations=diffuse[1])
    return pipe.light_pipe_nodes(width, height, lut_ptr, float(lut[0]), coeffs, with_filmic=with_filmic,
                                 filmic=filmic, demosaic_method=abi.DT_HIP_DEMOSAIC_RCD if demosaic_method is None else demosaic_method)


def have_filmic():
    try:
        from ansel_amd import filmic  # noqa: F401
        return True
    except Exception:
        return False


def _chain_pass(l, prefix, nodes, w, h, raw, cfa, rgb, out16):
    """one pass of the module chain on host buffers, ping-ponging between two CFA and two RGBA planes"""
    import checkers as ck
    src = raw
    ci = ri = 0
    for n in nodes:
        if n.op == "export_u16":
            getattr(l, prefix + "export_convert_u16")(w, h, ck.ptr(src), ck.ptr(out16))
            continue
        if n.op in ("rawprepare", "temperature", "highlights"):
            dst = cfa[ci]
            ci ^= 1
        else:
            dst = rgb[ri]
            ri ^= 1
        rc = ck.call(l, prefix + n.op, n.piece, n.data, src, dst)
        assert rc == 0, n.op
        src = dst


def cpu_baseline(size_name, with_filmic, which="light", device_size=None):
    """The reference's own process() code (oracle/_ref/libansel_ref_fast.so: its sources compiled in place with
    its release flags, OpenMP) on a bounded sample of the same workload: threads bound to cores
    (OMP_PROC_BIND=spread, OMP_PLACES=cores -- set by cpu_baseline_in_child() for a fresh process), the thread count
    swept over {16, 32, 64, 128, all} on the sample frame and the best kept; when a pass at that count is short enough,
    one more pass on the DEVICE's frame size replaces the sample.  Buffers are first touched by the OpenMP team
    (the warm-up pass), so pages land on the NUMA node of the thread that streams them.  Falls back to the C
    restatement (kind "port") where _ref is absent."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import checkers as ck
    from ansel_amd import params, synth
    ref = ck.ref(fast=True)
    kind = "reference" if ref is not None else "port"
    l = ref if ref is not None else ck.oracle()
    if l is None:
        return None
    prefix = "ref_" if ref is not None else "oracle_"
    ncpu = os.cpu_count() or 1
    if ref is not None:
        ref.ref_get_num_threads.restype = C.c_int
        set_threads = ref.ref_set_num_threads
    else:
        set_threads = C.CDLL("libgomp.so.1").omp_set_num_threads
    lut = params.srgb_encode_lut()

    def buffers(w, h):
        raw = ck.aligned_empty((h, w), np.uint16)
        raw[...] = synth.bayer_mosaic_tiled(w, h, seed=1)
        return (raw, [ck.aligned_empty((h, w), np.float32) for _ in range(2)],
                [ck.aligned_empty((h, w, 4), np.float32) for _ in range(2)], ck.aligned_empty((h, w, 4), np.uint16))

    quota = cgroup_cpu_quota()
    first = int(round(quota)) if quota and quota >= 1 else 32  # a container with a CPU quota runs best on that many threads
    counts = sorted({c for c in (16, 32, 64, 128, ncpu, first) if c <= ncpu} | {ncpu})
    # the thread count: a sweep on a 6 MP frame of the same chain (a pass there takes 0.1 - 1.5 s) ...
    sw, sh = 3000, 2000
    snodes = build_pipe(sw, sh, lut.ctypes.data, lut, with_filmic, which)
    raw, cfa, rgb, out16 = buffers(sw, sh)
    sweep = {}
    t_budget = time.time() + 12.0
    for c in sorted(counts, key=lambda c: (abs(c - first), c)):
        set_threads(c)
        _chain_pass(l, prefix, snodes, sw, sh, raw, cfa, rgb, out16)  # warm-up: page in, spin up the team
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            _chain_pass(l, prefix, snodes, sw, sh, raw, cfa, rgb, out16)
            times.append(time.perf_counter() - t0)
        sweep[c] = min(times)
        if time.time() > t_budget and len(sweep) >= 2:
            break
    best_c = min(sweep, key=sweep.get)
    del raw, cfa, rgb, out16
    # ... the figure: the sample frame (24 MP unless --cpu-sample says otherwise) at that count, best of two passes after a warm-up
    w, h = frame_size(size_name)
    nodes = build_pipe(w, h, lut.ctypes.data, lut, with_filmic, which)
    raw, cfa, rgb, out16 = buffers(w, h)
    set_threads(best_c)
    _chain_pass(l, prefix, nodes, w, h, raw, cfa, rgb, out16)
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        _chain_pass(l, prefix, nodes, w, h, raw, cfa, rgb, out16)
        times.append(time.perf_counter() - t0)
    best = min(times)
    sample = "%d x %d RGGB frame (%s), same module chain, best of 2 passes after a warm-up, %.2f s per pass" % (w, h, size_name, best)
    value = w * h / 1e6 / best
    on_sample = {"value": round(value, 3), "unit": "MPix/s", "sample": sample}
    # the device's own frame size -- the frame the metric is quoted on -- when one pass of it is affordable: <= ~40 s predicted
    # (round 6; it was 8 s, which left the full pipe's figure on the 24 MP sample: the 100 MP full chain is ~22 s a pass at the
    # ~4.6 MPix/s of the boxes seen, warm-up + one timed pass ~45 s of the run)
    if device_size is not None and device_size != (w, h):
        dw, dh = device_size
        predicted = best * (dw * dh) / float(w * h)
        if predicted <= 40.0:
            del raw, cfa, rgb, out16
            dn = build_pipe(dw, dh, lut.ctypes.data, lut, with_filmic, which)
            raw, cfa, rgb, out16 = buffers(dw, dh)
            _chain_pass(l, prefix, dn, dw, dh, raw, cfa, rgb, out16)
            t0 = time.perf_counter()
            _chain_pass(l, prefix, dn, dw, dh, raw, cfa, rgb, out16)
            t = time.perf_counter() - t0
            value = dw * dh / 1e6 / t
            sample = ("%d x %d RGGB frame (the device's), same module chain, one pass after a warm-up, %.2f s; thread "
                      "count chosen on a %d x %d frame" % (dw, dh, t, sw, sh))
    # `cores`: what the container may use -- its cgroup quota where it has one (threads beyond it share those cores)
    cores = int(round(quota)) if quota and quota >= 1 else best_c
    return {"value": round(value, 3), "unit": "MPix/s", "cores": min(cores, best_c), "threads": best_c, "kind": kind, "sample": sample,
            "on_sample_frame": on_sample, "host_threads": ncpu, "cpu_quota": quota,
            "binding": "OMP_PROC_BIND=%s OMP_PLACES=%s" % (os.environ.get("OMP_PROC_BIND"), os.environ.get("OMP_PLACES")),
            "thread_sweep_mpix_s_on_6MP": {str(c): round(sw * sh / 1e6 / t, 3) for c, t in sorted(sweep.items())}}


def cpu_baseline_in_child(size_name, with_filmic, which, device_size):
    """cpu_baseline() in a process of its own: the OpenMP runtime reads its binding once, when it starts, and this
    process has started it long ago (torch, the oracle's verify pass) -- with threads bound here the same 24 MP chain
    ran at 5.8 MPix/s against 57 MPix/s in a fresh process (profiles/r02_cpu_baseline_binding_sweep.txt)"""
    env = dict(os.environ)
    env.setdefault("OMP_PROC_BIND", "spread")
    env.setdefault("OMP_PLACES", "cores")
    code = ("import sys, json; sys.path.insert(0, %r); import bench; "
            "print('CPU_BASELINE ' + json.dumps(bench.cpu_baseline(%r, %r, %r, device_size=%r)))"
            % (ROOT, size_name, bool(with_filmic), which, tuple(device_size)))
    try:
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=420)
    except subprocess.TimeoutExpired:
        return None
    for ln in out.stdout.splitlines():
        if ln.startswith("CPU_BASELINE "):
            return json.loads(ln[len("CPU_BASELINE "):])
    sys.stderr.write("bench.py: the CPU baseline child failed:\n" + out.stderr[-600:] + "\n")
    return None


def verify_output(out16, raw_host, width, height, with_filmic, which):
    """AFTER the timed region: the buffer the timed steps wrote against the oracle's module-by-module chain on the
    same mosaic (oracle/liboracle.so, the checker; every host core).  Returns the `verify` object of the line."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import checkers as ck
    from ansel_amd import params
    l = ck.oracle()
    if l is None:
        return {"verified": None, "why": "oracle/liboracle.so missing"}
    try:
        C.CDLL("libgomp.so.1").omp_set_num_threads(os.cpu_count() or 1)
    except OSError:
        pass
    lut = params.srgb_encode_lut()
    nodes = build_pipe(width, height, lut.ctypes.data, lut, with_filmic, which)
    t0 = time.perf_counter()
    src = raw_host
    for n in nodes:
        if n.op == "export_u16":
            exp = ck.aligned_empty((height, width, 4), np.uint16)
            l.oracle_export_convert_u16(width, height, ck.ptr(src), ck.ptr(exp))
            break
        dst = ck.aligned_empty((height, width) if n.op in ("rawprepare", "temperature", "highlights") else (height, width, 4),
                               np.float32)
        fn = getattr(l, "oracle_" + n.op)
        fn.restype = C.c_int
        rc = fn(C.byref(n.piece), C.byref(n.data) if n.data is not None else None, ck.ptr(src), ck.ptr(dst))
        assert rc == 0, n.op
        src = dst
    t_oracle = time.perf_counter() - t0
    got = out16.cpu().numpy().view(np.uint16)
    bad = 0
    for r0 in range(0, height, 512):
        bad += int((got[r0:r0 + 512] != exp[r0:r0 + 512]).sum())
    return {"verified": bad == 0, "words": int(got.size), "mismatches": bad,
            "against": "oracle/liboracle.so chain on the same mosaic, %.1f s on %d host threads" % (t_oracle, os.cpu_count() or 1)}


PMC_SUMMARIES = {  # committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE summaries of THIS configuration, newest first
    "full": ("r06_pmc_hbm_bytes_100MP_full.json", "r05_dma_pmc_hbm_bytes_100MP_full.json", "r05_pmc_hbm_bytes_100MP_full.json", "r04_pmc_hbm_bytes_100MP_full.json", "r03_pmc_hbm_bytes_100MP_full.json"),
    "light": ("r03_pmc_hbm_bytes_100MP_light_fused.json", "r02_pmc_hbm_bytes_100MP_light_fused.json"),
}


def _sha16(path):
    import hashlib
    try:
        return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def _table_sha16(src):
    """the `lib_sha16` a committed counter summary records (tools/profile_round.sh's run), None for the older ones"""
    if not src:
        return None
    try:
        return json.load(open(os.path.join(ROOT, "profiles", src.split("profiles/")[-1]))).get("lib_sha16")
    except (OSError, ValueError):
        return None


def pmc_table(args):
    """{kernel tag: HBM bytes per launch} from the COMMITTED PMC summary of this exact configuration (not collected
    in this run: counters need rocprofv3 around the process -- tools/profile_round.sh -> tools/pmc_hbm_json.py:
    separate FETCH_SIZE / WRITE_SIZE passes with the gfx950 corrections of MI355X_MICROARCH.md); ({}, None) when no
    summary matches the configuration."""
    if args.size != "100MP" or args.no_fusion or args.mode != "batch":
        return {}, None
    for name in PMC_SUMMARIES.get(args.pipe, ()):
        path = os.path.join(ROOT, "profiles", name)
        try:
            kernels = json.load(open(path))["kernels"]
        except (OSError, ValueError, KeyError):
            continue
        return {k: v["hbm_bytes"] for k, v in kernels.items() if "hbm_bytes" in v}, "committed PMC summary profiles/" + name
    return {}, None


def sclk_table(args):
    """{kernel name: effective shader clock in MHz during its launches} from the COMMITTED summary of a rocprofv3 --pmc
    GRBM_GUI_ACTIVE pass over this configuration (tools/profile_round.sh -> tools/pmc_sclk_json.py; MI355X_MICROARCH.md
    "DVFS give-back": the chip clocks to its power budget, effective clock = busy cycles / wall time).  Round 4's review,
    item 4: a kernel's VALU floor is instructions x architectural cycles / CLOCK, and the clock is not the 2.4 GHz of the
    data sheet under an FMA-dense stream (profiles/r05_valu_issue_cycles.json: 1.87 - 1.96 GHz for v_fma_f32, 2.2 - 2.3 for
    v_add_f32, 2.4 for the half- and quarter-rate classes, at 2.0 cycles per full-rate wave64 instruction throughout)"""
    if args.size != "100MP" or args.no_fusion or args.mode != "batch" or args.pipe != "full":
        return {}, None
    kernels = None
    for name in ("r06_sclk_per_kernel_100MP_full.json", "r05_dma_sclk_per_kernel_100MP_full.json", "r05_sclk_per_kernel_100MP_full.json"):  # newest first
        try:
            kernels = json.load(open(os.path.join(ROOT, "profiles", name)))["kernels"]
            break
        except (OSError, ValueError, KeyError):
            continue
    if kernels is None:
        return {}, None
    # (launches of a few microseconds -- the wavelets' four-channel launches that leave at once -- have no meaningful ratio)
    return ({k: v["sclk_mhz"] for k, v in kernels.items() if "sclk_mhz" in v and v.get("ms_avg", 0.0) >= 0.05},
            "committed profiles/" + name)


def sclk_of(table, tag):
    names = TAG_KERNELS.get(tag, (tag, tag.replace("_u16", "")))
    got = [v for k, v in table.items() for n in dict.fromkeys(names) if k == n or k.startswith(n + "<")]
    return round(sum(got) / len(got), 1) if got else None


# which kernels (function names as the PMC summary keeps them, template arguments stripped) a bench tag launches
TAG_KERNELS = {
    "nlm_chunks": ("nlm_chunks_v3", "nlm_chunks_v4", "nlm_chunks_v2", "nlm_chunks_pipelined", "nlm_chunks"),
    "diffuse_pde": ("diffuse_pde_strip", "diffuse_pde"), "diffuse_decompose": ("bspline_decompose_strip", "bspline_decompose"),
    "dn_decompose": ("dn_decompose_strip", "dn_decompose"), "rgb_chain_u16": ("rgb_chain",), "rgb_chain_rows16": ("rgb_chain",),
    "bilat_blur": ("bilat_blur_yz", "bilat_blur_x", "bilat_blur_line", "bilat_blur_line_z"), "bilat_splat": ("bilat_splat2", "bilat_zcells", "bilat_splat", "bilat_lightness"),
    "dn_band_threshold": ("dn_band_sums", "dn_band_threshold"),
}


def traffic_of(table, tag):
    """HBM bytes of ONE launch of `tag` (a tag whose launch runs several kernels: their sum)"""
    names = TAG_KERNELS.get(tag, (tag, tag.replace("_u16", "")))
    got = [table[n] for n in dict.fromkeys(names) if n in table]
    if not got:
        return None
    return sum(got) if tag in ("bilat_blur", "bilat_splat", "dn_band_threshold") else got[0]


# What binds each kernel, and the peak it is priced against.  HBM: 8 TB/s.  VALU: one wave64 instruction per
# SIMD every 2 cycles for full-rate binary32, 4 for binary64, 8 for the quarter-rate transcendental unit
# (MI355X_MICROARCH.md "Per-instruction cycle constants") -> the kernel's issue-cycle total from its instruction mix
# (profiles/r04_isa_mix.json, tools/valu_model.py arch) over 1024 SIMDs at 2.4 GHz is its floor.
KERNEL_BOUND = {"raw_chain": "hbm", "rgb_chain": "valu", "rgb_chain_u16": "valu", "rcd_tiles": "valu+lds",
                "nlm_chunks": "lds+valu", "nlm_tail": "latency (a 72-addition row chain per offset; four workgroups a CU)", "diffuse_pde": "valu", "dn_decompose": "valu", "diffuse_decompose": "hbm",
                "bilat_splat": "latency (one lane per grid node walks its pixels in order)", "bilat_slice": "hbm", "bilat_blur": "latency",
                "dn_synthesize": "hbm", "dn_precondition": "hbm", "dn_finish": "hbm", "dn_finish_chain": "hbm", "rgb_to_lab": "hbm",
                "lab_to_rgb": "hbm"}


def fp32_valu_figure(tag, dom, pixels, nodes=None):
    """the dominant launch against the binary32 vector peak, for the kernel SURVEY 8(d) says is not an HBM kernel: non-local means'
    algorithmic flops -- (2 K + 1)^2 offsets x ~25 flop per pixel and offset at K = 7, the module's default on a full-resolution
    export: 5.6 kflop per pixel -- over its average duration, against the 157.3 TFLOP/s of MI355X_MICROARCH.md (256 CUs x 4 SIMDs
    x 32 lanes x 2 flop per FMA x 2.4 GHz).  The kernel's instructions are additions, multiplications and integer operations, not
    FMAs (0.3 %): one flop per lane and issue slot, so 0.5 is the most this figure can reach; roofline.valu_frac is the same launch
    in issue slots."""
    if tag != "nlm_chunks" or not dom.get("ms_avg"):
        return None
    # nlmeans' search radius: K = ceil(7 x scale) (src/iop/nlmeans.c:425), the scale of the pipe's node
    import math
    k = 7
    for n in nodes or ():
        if n.op == "nlmeans":
            k = int(math.ceil(7.0 * min(float(n.piece.roi_in.scale), 2.0)))
    offsets = (2 * k + 1) ** 2
    flops = offsets * 25.0 * pixels
    ach = flops / (dom["ms_avg"] * 1e-3) / 1e12
    return {"achieved": round(ach, 2), "peak": 157.3, "unit": "TFLOP/s", "frac": round(ach / 157.3, 4), "offsets": offsets,
            "flops_per_px": int(offsets * 25), "ceiling_for_a_stream_without_fma": 0.5}


def valu_floor_ms(tag, mpix, table=None):
    if table is None:
        table = next((t for t in ("r06_isa_mix.json", "r05_dma_isa_mix.json", "r05_isa_mix.json") if os.path.exists(os.path.join(ROOT, "profiles", t))), "r04_isa_mix.json")
    return _valu_floor_ms(tag, mpix, table)


def valu_floor_step_ms(tag, mpix):
    """the issue floors of ALL instantiations the table lists for `tag`, summed: a frame launches each once (the wavelets' scales)"""
    table = next((t for t in ("r06_isa_mix.json", "r05_dma_isa_mix.json", "r05_isa_mix.json") if os.path.exists(os.path.join(ROOT, "profiles", t))), "r04_isa_mix.json")
    try:
        kernels = json.load(open(os.path.join(ROOT, "profiles", table))).get("kernels", {})
    except (OSError, ValueError):
        return None
    base = {"dn_decompose": "dn_decompose_strip"}.get(tag, tag)
    return sum(v["issue_floor_ms_per_mpix"] for k, v in kernels.items() if k.startswith(base + "<") and "issue_floor_ms_per_mpix" in v) * mpix


def _valu_floor_ms(tag, mpix, table):
    """VALU issue floor of `tag` on a frame of `mpix` megapixels from a COMMITTED instruction-mix table (tools/valu_model.py ... arch
    over the rocprofv3 SQ counters of this bench): the dynamic instruction mix priced per class at the ARCHITECTURAL issue rate of a
    SIMD-32 -- 2 cycles per full-rate wave64 instruction, 4 for binary64 and conversions, 8 for the transcendental unit -- at the 2.4 GHz
    peak clock.  profiles/r05_valu_issue_cycles.json (tools/valu_clock_microbench.hip: the shader clock read beside the cycle count)
    confirms those rates on this chip -- v_fma / v_mul / v_add 1.9 - 2.1 cycles, v_cmp / v_cvt / v_div_scale / v_div_fixup / v_max3 3.3 -
    4.0, v_rcp / v_sqrt 6.3 - 8.0 -- and shows what rounds 2 - 4 called "measured rates" (2.5 - 3.0 cycles: wall time x an assumed 2.4
    GHz) to be the CLOCK: 1.87 - 1.96 GHz under an FMA stream, 2.0 - 2.1 under multiplies, 2.2 - 2.3 under additions.  A tag that launches
    several instantiations of a kernel (the wavelets: one per dilation) takes their mean.  None when the table lacks the kernel"""
    try:
        mix = json.load(open(os.path.join(ROOT, "profiles", table)))
    except (OSError, ValueError):
        return None
    alias = {"dn_decompose": "dn_decompose_strip", "nlm_chunks": "nlm_chunks_v3", "diffuse_decompose": "bspline_decompose_strip",
             "diffuse_pde": "diffuse_pde_strip", "dn_finish_chain": "dn_finish_chain"}
    kernels = mix.get("kernels", {})
    base = alias.get(tag, tag.replace("_u16", ""))
    inst = [v for k, v in kernels.items() if k.startswith(base + "<") and "issue_floor_ms_per_mpix" in v]
    if inst:
        return sum(v["issue_floor_ms_per_mpix"] for v in inst) / len(inst) * mpix
    k = kernels.get(tag) or kernels.get(base)
    if not k or "issue_floor_ms_per_mpix" not in k:
        return None
    return k["issue_floor_ms_per_mpix"] * mpix


def measured_ceiling(torch, dev, gib=1.0, reps=8):
    """what a streaming kernel reaches on THIS device in THIS run (beside the 8 TB/s of the data sheet): a
    device-to-device copy (read + write), a triad a = b + s c (two reads + a write), a fill (write) and a sum (read) over
    `gib` GiB planes, HIP events on the current stream, best of `reps`"""
    n = int(gib * (1 << 30)) // 4
    a = torch.empty(n, dtype=torch.float32, device=dev)
    b = torch.ones(n, dtype=torch.float32, device=dev)
    c = torch.ones(n, dtype=torch.float32, device=dev)
    out = {}
    # fill (writes only) and sum (reads only) tell which direction a kernel is short of: the B-spline analysis and the wavelet
    # levels write as many bytes as they read
    for name, fn, streams in (("copy", lambda: a.copy_(b), 2), ("triad", lambda: torch.add(b, c, alpha=2.0, out=a), 3),
                              ("fill", lambda: a.fill_(1.5), 1), ("sum", lambda: b.sum(), 1)):
        fn()
        best = None
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None or ms < best else best
        out[name + "_GBs"] = round(streams * n * 4 / (best * 1e-3) / 1e9, 1)
    del a, b, c
    return out


def full_pipe_leg(torch, np, pipe, synth, l, devid, dev, size, lut, lut_host, with_filmic, fusion, verify=True, steps=3):
    """the metric's pipe on another frame size, after the timed region: ms per step, per-kernel ms, non-local means per megapixel,
    and the exported words against the oracle"""
    w, h = frame_size(size)
    raw_host = synth.bayer_mosaic_tiled(w, h, seed=1)
    raw = torch.from_numpy(raw_host.view(np.int16)).to(dev)
    nodes = build_pipe(w, h, lut.data_ptr(), lut_host, with_filmic, "full")
    ex = pipe.DevicePipe(devid, nodes, fusion=fusion)
    out = torch.empty((h, w, 4), dtype=torch.int16, device=dev)
    ex.process(raw.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(dev)
    l.dt_hip_events_reset(devid)
    l.dt_hip_events_enable(devid, 1)
    t1 = time.perf_counter()
    for _ in range(steps):
        ex.process(raw.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t1) / steps * 1e3
    l.dt_hip_events_enable(devid, 0)
    k = read_kernel_events(l, devid)
    bpp = pipe.algorithmic_bytes_per_pixel(nodes)
    mpix = w * h / 1e6
    kms = {n: round(v["ms_avg"] * v["launches"] / steps, 3) for n, v in sorted(k.items())}
    nlm_ms = kms.get("nlm_chunks", 0.0) + kms.get("nlm_tail", 0.0)
    leg = {"workload": "%d x %d RGGB u16 raw (%s), the same full export pipe" % (w, h, size), "steps": steps, "ms_per_step": round(ms, 3),
           "mpix_s": round(mpix / (ms * 1e-3), 2), "algorithmic_bytes_per_px": bpp,
           "pipe_hbm_frac": round(bpp * w * h / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "kernels_ms_per_step": kms,
           "nlmeans_ms_per_mpix": round(nlm_ms / mpix, 4),
           "nlmeans_chunk_rows": "69 (compute_slice_height(4000), nlmeans_core.c:264-295): nlm_chunks_v4 on the first 64 rows of every "
                                 "interior chunk + nlm_tail on the other five" if size == "24MP" else None}
    ex.close()
    if verify:
        leg["verify"] = verify_output(out, raw_host, w, h, with_filmic, "full")
        leg["verified"] = leg["verify"]["verified"]
    del out, raw
    return leg


DUMP_BYTES = 64_000_000  # --dump-outputs: the most it writes, all files together
DUMP_SAMPLE_DRAWS = 2_000_000  # pixels drawn (with replacement, then de-duplicated) when the frame exceeds the budget
DUMP_SEED = 20240517


def dump_outputs(dirpath, frame, width, height, prefix="", budget=DUMP_BYTES):
    """--dump-outputs: the exported RGBA u16 words of the last timed step, as a caller of dt_hip_pipe_process receives them.
    `frame` is (height, width, 4) 16-bit words: a device tensor (int16 view) or a host array.  Writes DIR/<prefix>export_rgba.npy
    in float32 (every u16 is exact): the whole frame (height, width, 4) when it fits the budget, else the (n, 4) words of a
    fixed seeded sample of pixels together with DIR/<prefix>export_rgba_pixel_index.npy (float64, row * width + column, sorted).
    The sample depends on the frame size only, so two builds run with the same arguments write the same pixels."""
    import numpy as np
    os.makedirs(dirpath, exist_ok=True)
    npix = width * height
    words = frame.reshape(npix, 4)
    idx = None
    if npix * 4 * 4 > budget:
        rng = np.random.default_rng(DUMP_SEED)
        draws = min(DUMP_SAMPLE_DRAWS, budget // (4 * 4 + 8))
        idx = np.unique(rng.integers(0, npix, draws))
        if isinstance(words, np.ndarray):
            words = words[idx]
        else:
            import torch
            words = words[torch.from_numpy(idx).to(words.device)]
    if not isinstance(words, np.ndarray):
        words = words.cpu().numpy()
    vals = np.ascontiguousarray(words).view(np.uint16).astype(np.float32)
    np.save(os.path.join(dirpath, prefix + "export_rgba.npy"), vals if idx is not None else vals.reshape(height, width, 4))
    if idx is not None:
        np.save(os.path.join(dirpath, prefix + "export_rgba_pixel_index.npy"), idx.astype(np.float64))


def band_digest(t):
    """64-bit digest of a band's exported words (host side, after the timed region)"""
    import xxhash
    return xxhash.xxh64(t.cpu().numpy().tobytes()).hexdigest()


def cgroup_cpu_quota():
    """the container's CPU quota in cores (cgroup v2 cpu.max / v1 cfs quota), None when unlimited or unreadable"""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else round(int(q) / float(per), 2)
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else round(q / float(per), 2)
    except (OSError, ValueError):
        return None


def read_kernel_events(l, devid):
    maxk = 96
    tags = (C.c_char_p * maxk)()
    ms = (C.c_float * maxk)()
    cnt = (C.c_int * maxk)()
    nk = l.dt_hip_events_profiling(devid, tags, ms, cnt, maxk)
    kernels = {}
    for i in range(min(nk, maxk)):
        kernels[tags[i].decode()] = {"ms_avg": ms[i] / max(cnt[i], 1), "launches": cnt[i]}
    return kernels


def self_spawn(args):
    """`python bench.py --gpus N` without a launcher: run the N ranks ourselves, one process per GPU, on 127.0.0.1"""
    import socket
    import subprocess
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < args.gpus:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible; there is no CPU fallback and no oversubscription"
                         % (args.gpus, have))
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def bands_mode(args):
    """BASELINE.json config 4 from ONE process: the frame cut into row bands, band k on device k % --gpus, walked by
    dt_hip_pipe_process_bands() (a host thread per band; halo rows, the wavelets' partial sums and the bilateral grid as
    peer copies between the devices, ordered by events).  Peer copies, not RCCL: one process owns every device."""
    import numpy as np
    import torch
    from ansel_amd import abi, lib, params, pipe, synth, tiled
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False and there is no CPU fallback")
    have = torch.cuda.device_count()
    if have < args.gpus:
        raise SystemExit("bench.py --mode bands --gpus %d: only %d GPU(s) visible" % (args.gpus, have))
    ndev = args.gpus
    nb = args.bands or ndev
    l = lib.init()
    devs = (C.c_int * ndev)(*range(ndev))
    peer_rc = l.dt_hip_peer_selftest(devs, ndev)
    peer_msg = None if peer_rc == 0 else l.dt_hip_last_error().decode()
    if peer_rc != 0:
        sys.stderr.write("bench.py: peer self-test FAILED: %s\n" % peer_msg)
    width, height = frame_size(args.size)
    npix = width * height
    with_filmic = have_filmic()
    raw_host = synth.bayer_mosaic_tiled(width, height, seed=1)
    lut_host = params.srgb_encode_lut()
    luts, pipes, ins, outs = [], [], [], []
    nodes0 = None
    for k in range(nb):
        d = k % ndev
        torch.cuda.set_device(d)
        lut = torch.from_numpy(lut_host).to("cuda:%d" % d)
        luts.append(lut)
        nodes = build_pipe(width, height, lut.data_ptr(), lut_host, with_filmic, args.pipe)
        nodes0 = nodes0 or nodes
        pipes.append(pipe.DevicePipe(d, nodes, fusion=not args.no_fusion))
    bands = tiled.plan_bands(width, height, nb, tiled.pipe_demosaic_method(nodes0))
    for k, b in enumerate(bands):
        d = "cuda:%d" % (k % ndev)
        ins.append(torch.from_numpy(np.ascontiguousarray(raw_host[b.row0:b.row0 + b.rows]).view(np.int16)).to(d))
        outs.append(torch.empty((b.rows, width, 4), dtype=torch.int16, device=d))
    a_p = (C.c_void_p * nb)(*[p.handle for p in pipes])
    a_b = (abi.Band * nb)(*bands)
    a_i = (C.c_void_p * nb)(*[t.data_ptr() for t in ins])
    a_o = (C.c_void_p * nb)(*[t.data_ptr() for t in outs])

    def step():
        lib.check(l.dt_hip_pipe_process_bands(a_p, nb, a_b, a_i, a_o), "dt_hip_pipe_process_bands")

    def sync():
        for d in range(ndev):
            torch.cuda.synchronize(d)

    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync()
    elapsed = time.perf_counter() - t0
    st = abi.BandStats()
    l.dt_hip_pipe_bands_stats(C.byref(st))
    verifying = args.full and not args.no_verify
    whole = None
    if args.dump_outputs or verifying:
        whole = np.concatenate([t.cpu().numpy().view(np.uint16) for t in outs], axis=0)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, whole, width, height)
    verify = None
    if verifying:
        class _H:  # verify_output() takes a tensor-like with .cpu().numpy()
            def cpu(self):
                return self

            def numpy(self):
                return whole
        verify = verify_output(_H(), raw_host, width, height, with_filmic, args.pipe)
    ms = elapsed / args.steps * 1e3
    bpp = pipe.algorithmic_bytes_per_pixel(nodes0)
    line = {
        "metric": "MPix/s full export pixelpipe (100 MP raw); % MI355X HBM roofline",
        "value": round(npix / 1e6 / (elapsed / args.steps), 2), "unit": "MPix/s", "n_gpus": ndev, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": "%d x %d RGGB u16 raw (%s), %s export pipe: %s; module defaults; ONE frame cut into %d row bands on %d "
                        "device(s) of one process (dt_hip_pipe_process_bands: peer copies ordered by events, not RCCL)"
                        % (width, height, args.size, args.pipe, " > ".join(n.op for n in nodes0), nb, ndev),
            "frame_mpix": round(npix / 1e6, 2), "bands": nb, "devices": ndev,
            "pipe_algorithmic_bytes_per_px": bpp,
            "pipe_hbm_frac_per_device": round(bpp * npix / ndev / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "exchange_stops_per_frame": st.exchange_stops, "peer_copies_last_frame": st.peer_copies,
            "peer_bytes_last_frame": st.peer_bytes, "host_wait_ms_all_bands_last_frame": round(st.host_wait_ns / 1e6, 3),
            "pairs_without_peer_access": st.pairs_without_peer_access,
            "peer_selftest": "ok" if peer_rc == 0 else peer_msg,
        },
        "roofline": None,
    }
    if verify is not None:
        line["verified"] = verify["verified"]
        line["verify"] = verify
    print(json.dumps(line), flush=True)
    for p in pipes:
        p.close()
    return 0


def main():
    args = parse()
    if args.mode == "bands":
        return bands_mode(args)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(self_spawn(args))
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%s ranks" % (args.gpus, env_world))
    import numpy as np
    import torch
    import torch.distributed as dist
    from ansel_amd import abi, lib, params, pipe, synth, tiled

    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False and there is no CPU fallback")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    l = lib.init()
    devid = local_rank
    stream = torch.cuda.current_stream(dev)
    lib.check(l.dt_hip_set_stream(devid, C.c_void_p(stream.cuda_stream)), "dt_hip_set_stream")

    width, height = frame_size(args.size)
    npix = width * height
    with_filmic = have_filmic()

    # ---- inputs resident in HBM before the timed region
    raw_host = synth.bayer_mosaic_tiled(width, height, seed=1 + rank)
    raw = torch.from_numpy(raw_host.view(np.int16)).to(dev)
    lut_host = params.srgb_encode_lut()
    lut = torch.from_numpy(lut_host).to(dev)
    nodes = build_pipe(width, height, lut.data_ptr(), lut_host, with_filmic, args.pipe)
    # intermediates belong to the executor: it draws them from the runtime's pool
    executor = pipe.DevicePipe(devid, nodes, fusion=not args.no_fusion)
    my_rows = height
    if args.mode == "tiled":
        # every rank synthesises the same frame and keeps only its band resident
        raw_host = synth.bayer_mosaic_tiled(width, height, seed=1)
        bands = tiled.plan_bands(width, height, world, tiled.pipe_demosaic_method(nodes))
        band = bands[rank]
        my_rows = band.rows
        raw = torch.from_numpy(np.ascontiguousarray(raw_host[band.row0:band.row0 + band.rows]).view(np.int16)).to(dev)
        out16 = torch.empty((band.rows, width, 4), dtype=torch.int16, device=dev)
        engine = tiled.HipBandEngine(executor, dev)

        def step():
            tiled.process_band(engine, bands, rank, raw.data_ptr(), out16.data_ptr(), width,
                               dist=dist if world > 1 else None)
    else:
        out16 = torch.empty((height, width, 4), dtype=torch.int16, device=dev)

        def step():
            # the C++ executor (dt_hip_pipe_process): raw u16 in HBM -> exported RGBA u16 in HBM
            executor.process(raw.data_ptr(), out16.data_ptr())

    def sync_all():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    sync_all()
    l.dt_hip_events_reset(devid)
    l.dt_hip_events_enable(devid, 1)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    l.dt_hip_events_enable(devid, 0)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # ---- per-kernel HIP-event timings of the timed region (recorded on the launch stream)
    kernels = read_kernel_events(l, devid)

    # ---- what the last timed step wrote (this rank's frame, or its band in --mode tiled), before anything else runs
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out16, width, my_rows, prefix="rank%d_" % rank if world > 1 else "",
                     budget=DUMP_BYTES // world)

    # ---- with --full, --mode tiled validates itself (after the timed region): every rank digests the band its timed steps
    #      wrote, rank 0 runs the SAME frame unsplit through the same executor and compares band by band -- the assembled bands
    #      are the unsplit frame or the line says so.  What the collectives moved and how many ranks RCCL saw go on the line too.
    tiled_check = None
    if args.mode == "tiled" and args.full:
        mine = band_digest(out16)
        if world > 1:
            digests = [None] * world
            dist.all_gather_object(digests, mine)
            logs = [None] * world
            dist.all_gather_object(logs, {k: list(v) for k, v in tiled.EXCHANGE_LOG.items()})
        else:
            digests, logs = [mine], [{k: list(v) for k, v in tiled.EXCHANGE_LOG.items()}]
        if rank == 0:
            whole_in = torch.from_numpy(raw_host.view(np.int16)).to(dev)
            whole_out = torch.empty((height, width, 4), dtype=torch.int16, device=dev)
            # the unsplit frame on this rank's executor (the same node list: a DevicePipe runs either way)
            executor.process(whole_in.data_ptr(), whole_out.data_ptr())
            torch.cuda.synchronize(dev)
            want = [band_digest(whole_out[b.row0:b.row0 + b.rows]) for b in bands]
            del whole_in, whole_out
            try:
                rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                rccl = None
            tiled_check = {"verified": digests == want, "bands_equal_unsplit": [a == b for a, b in zip(digests, want)],
                           "against": "the same frame unsplit through dt_hip_pipe_process on rank 0, xxh64 of every band's exported words",
                           "ranks_seen": dist.get_world_size() if world > 1 else 1, "rccl_version": rccl,
                           "exchanges_last_frame": [{k: {"calls": v[0], "bytes_sent": v[1]} for k, v in sorted(lg.items())} for lg in logs],
                           "band_rows": [int(b.rows) for b in bands]}

    # ---- with --full, after the timed region: the buffer those steps wrote, against the oracle
    verify = None
    ranks_check = None
    if args.full and args.mode == "batch" and world > 1 and not args.no_verify:
        # N > 1, one frame per GPU: every rank also runs RANK 0's frame once and the digests must agree -- together with rank
        # 0's comparison against the oracle below that pins every device's output, not only the first one's
        same_in = torch.from_numpy(synth.bayer_mosaic_tiled(width, height, seed=1).view(np.int16)).to(dev)
        same_out = torch.empty((height, width, 4), dtype=torch.int16, device=dev)
        executor.process(same_in.data_ptr(), same_out.data_ptr())
        torch.cuda.synchronize(dev)
        digests = [None] * world
        dist.all_gather_object(digests, band_digest(same_out))
        del same_in, same_out
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl = None
        ranks_check = {"ranks_seen": dist.get_world_size(), "rccl_version": rccl, "all_ranks_equal_on_rank0_frame": len(set(digests)) == 1}
    if args.full and rank == 0 and args.mode == "batch" and not args.no_verify:
        verify = verify_output(out16, raw_host, width, height, with_filmic, args.pipe)
        if ranks_check is not None:
            verify.update(ranks_check)
            verify["verified"] = bool(verify["verified"]) and ranks_check["all_ranks_equal_on_rank0_frame"]

    # ---- config 2's module list on the SAME frame, same run (config.light_pipe)
    light = None
    if args.full and rank == 0 and world == 1 and args.mode == "batch" and args.pipe != "light" and not args.no_light_pipe:
        lnodes = build_pipe(width, height, lut.data_ptr(), lut_host, with_filmic, "light")
        lexec = pipe.DevicePipe(devid, lnodes, fusion=not args.no_fusion)
        lout = torch.empty((height, width, 4), dtype=torch.int16, device=dev)  # `out16` keeps the timed steps' frame
        lexec.process(raw.data_ptr(), lout.data_ptr())
        torch.cuda.synchronize(dev)
        l.dt_hip_events_reset(devid)
        l.dt_hip_events_enable(devid, 1)
        t1 = time.perf_counter()
        for _ in range(args.light_steps):
            lexec.process(raw.data_ptr(), lout.data_ptr())
        torch.cuda.synchronize(dev)
        l_ms = (time.perf_counter() - t1) / args.light_steps * 1e3
        l.dt_hip_events_enable(devid, 0)
        lk = read_kernel_events(l, devid)
        l_bpp = pipe.algorithmic_bytes_per_pixel(lnodes)
        light = {
            "workload": "%d x %d RGGB u16 raw, export pipe: %s; module defaults" % (width, height, " > ".join(n.op for n in lnodes)),
            "steps": args.light_steps,
            "ms_per_step": round(l_ms, 3),
            "mpix_s": round(npix / 1e6 / (l_ms * 1e-3), 2),
            "algorithmic_bytes_per_px": l_bpp,
            "hbm_frac": round(l_bpp * npix / (l_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "launch_groups": lexec.num_groups,
            "kernels_ms_per_step": {k: round(v["ms_avg"] * v["launches"] / args.light_steps, 3) for k, v in sorted(lk.items())},
        }
        lexec.close()
        # ... and the same ten modules with the other demosaic the north star names, AMaZE, in RCD's place (3 steps)
        try:
            anodes = build_pipe(width, height, lut.data_ptr(), lut_host, with_filmic, "light", abi.DT_HIP_DEMOSAIC_AMAZE)
            aexec = pipe.DevicePipe(devid, anodes, fusion=not args.no_fusion)
            aexec.process(raw.data_ptr(), lout.data_ptr())
            torch.cuda.synchronize(dev)
            l.dt_hip_events_reset(devid)
            l.dt_hip_events_enable(devid, 1)
            t1 = time.perf_counter()
            for _ in range(3):
                aexec.process(raw.data_ptr(), lout.data_ptr())
            torch.cuda.synchronize(dev)
            a_ms = (time.perf_counter() - t1) / 3 * 1e3
            l.dt_hip_events_enable(devid, 0)
            ak = read_kernel_events(l, devid)
            light["with_amaze"] = {"ms_per_step": round(a_ms, 3), "mpix_s": round(npix / 1e6 / (a_ms * 1e-3), 2),
                                   "hbm_frac": round(l_bpp * npix / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                   "kernels_ms_per_step": {k: round(v["ms_avg"] * v["launches"] / 3, 3) for k, v in sorted(ak.items())}}
            aexec.close()
        except Exception as e:  # the leg is informative: the line does not depend on it
            light["with_amaze"] = {"error": str(e)[:200]}
        del lout

    # ---- the metric's pipe with diffuse or sharpen at the module's $DEFAULT (1 iteration, all speeds 0) instead of the timed preset
    default_diffuse = None
    if args.full and rank == 0 and world == 1 and args.mode == "batch" and args.pipe == "full" and not args.no_light_pipe:
        dnodes = build_pipe(width, height, lut.data_ptr(), lut_host, with_filmic, "full", diffuse=DIFFUSE_DEFAULT)
        dexec = pipe.DevicePipe(devid, dnodes, fusion=not args.no_fusion)
        dout = torch.empty((height, width, 4), dtype=torch.int16, device=dev)
        dexec.process(raw.data_ptr(), dout.data_ptr())
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(3):
            dexec.process(raw.data_ptr(), dout.data_ptr())
        torch.cuda.synchronize(dev)
        d_ms = (time.perf_counter() - t1) / 3 * 1e3
        d_bpp = pipe.algorithmic_bytes_per_pixel(dnodes)
        default_diffuse = {"diffuse": "module $DEFAULT: 1 iteration, all four speeds 0 (src/iop/diffuse.c:79-98)", "steps": 3,
                           "ms_per_step": round(d_ms, 3), "mpix_s": round(npix / 1e6 / (d_ms * 1e-3), 2),
                           "algorithmic_bytes_per_px": d_bpp,
                           "pipe_hbm_frac": round(d_bpp * npix / (d_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        dexec.close()
        del dout
    # ---- the same full pipe on the 24 MP frame of BASELINE configs 1 / 2 (6000 x 4000, the commonest sensor): its non-local-means
    #      chunks are 69 rows high -- until round 5 the grid of the half-rate second version (round 4's review, "weak" item 4: no
    #      record ran the full pipe at 24 MP); verified against the oracle like the timed frame
    full24 = None
    if args.full and rank == 0 and world == 1 and args.mode == "batch" and args.pipe == "full" and args.size == "100MP" and not args.no_light_pipe:
        full24 = full_pipe_leg(torch, np, pipe, synth, l, devid, dev, "24MP", lut, lut_host, with_filmic, not args.no_fusion,
                               verify=not args.no_verify)
    ceiling = measured_ceiling(torch, dev) if args.full and rank == 0 else None

    # ---- the same step with the boundary's two PCIe legs (never `value`): sensor buffer in pinned host memory ->
    #      basebuffer upload -> pipe -> exported frame back into pinned host memory
    host_ms = None
    host_overlap_ms = None
    host_rows_ms = None
    host_rows_writer_ms = None
    # (round 6: also for the metric's own workload, --pipe full -- the sequential and the overlapped leg; the two writer-side legs
    #  stay with the light pipe, where the bus and not the kernels is the bound)
    if args.full and rank == 0 and world == 1 and args.mode == "batch" and not args.no_host_legs and args.pipe in ("light", "full"):
        nb_in, nb_out = raw_host.nbytes, npix * 8
        pin_in, pin_out = l.dt_hip_alloc_host_pinned(nb_in), l.dt_hip_alloc_host_pinned(nb_out)
        if pin_in and pin_out:
            C.memmove(pin_in, raw_host.ctypes.data, nb_in)
            fullp = abi.Piece.make(width, height, channels=1, datatype=abi.DT_HIP_TYPE_UINT16)
            times = []
            for _ in range(3):
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                lib.check(l.dt_hip_iop_basebuffer_process(devid, C.byref(fullp), width, height, 2, pin_in, raw.data_ptr()), "basebuffer")
                executor.process(raw.data_ptr(), out16.data_ptr())
                lib.check(l.dt_hip_read_host_from_device(devid, pin_out, out16.data_ptr(), width, height, 8), "read")
                times.append(time.perf_counter() - t1)
            host_ms = min(times) * 1e3
            # the same with upload / kernels / download of consecutive frames overlapped (dt_hip_batch_*, 3 slots)
            batch = l.dt_hip_batch_new(executor.handle, 3, nb_in, nb_out)
            if batch:
                nfr = 8
                for k in range(nfr + 3):
                    if k == 3:  # the first three fill the pipeline
                        l.dt_hip_batch_drain(batch)
                        torch.cuda.synchronize(dev)
                        t1 = time.perf_counter()
                    rc = l.dt_hip_batch_submit(batch, pin_in, pin_out)
                    assert rc >= 0, l.dt_hip_last_error()
                l.dt_hip_batch_drain(batch)
                host_overlap_ms = (time.perf_counter() - t1) / nfr * 1e3
                l.dt_hip_batch_free(batch)
            # ... and with the scanline packing of the format writer done by the chain ("export_rows": RGB u16
            # rows, 6 B/px instead of 8 over the bus)
            rows_exec = None if args.pipe != "light" else pipe.DevicePipe(devid, nodes + [pipe.Node("export_rows", abi.ExportRowsData(16, 3), nodes[-1].piece)],
                                        fusion=not args.no_fusion)
            batch = l.dt_hip_batch_new(rows_exec.handle, 3, nb_in, npix * 6) if rows_exec is not None else None
            if batch:
                nfr = 8
                for k in range(nfr + 3):
                    if k == 3:
                        l.dt_hip_batch_drain(batch)
                        torch.cuda.synchronize(dev)
                        t1 = time.perf_counter()
                    rc = l.dt_hip_batch_submit(batch, pin_in, pin_out)
                    assert rc >= 0, l.dt_hip_last_error()
                l.dt_hip_batch_drain(batch)
                host_rows_ms = (time.perf_counter() - t1) / nfr * 1e3
                # ... and with the fourth leg: a writer (dt_hip_batch_set_writer -- the format's write_image(), imageio_core.c:965)
                # that copies the frame's scanlines out of the pinned buffer, as an uncompressed TIFF's write() does, on the
                # batch's writer thread while the next frames are on the device
                sink = np.empty(npix * 6, np.uint8)
                WRITER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_size_t)

                def write_image(user, seq, host_out, nbytes):
                    C.memmove(sink.ctypes.data, host_out, nbytes)
                    return 0

                cb = WRITER(write_image)
                # host_out is the WRITER's until the slot's wait returns (include/ansel_hip.h): one pinned buffer per slot, rotated
                # as tests/test_gpu_batch.py and examples/export_pipe.c do (the first version of this leg handed all three slots
                # the same buffer: the writer copied it while the next frame's download overwrote it)
                pin_outs = [pin_out] + [l.dt_hip_alloc_host_pinned(npix * 6) for _ in range(2)]
                if all(pin_outs) and l.dt_hip_batch_set_writer(batch, cb, None) == 0:
                    for k in range(nfr + 3):
                        if k == 3:
                            l.dt_hip_batch_drain(batch)
                            t1 = time.perf_counter()
                        rc = l.dt_hip_batch_submit(batch, pin_in, pin_outs[k % 3])
                        assert rc >= 0, l.dt_hip_last_error()
                    assert l.dt_hip_batch_drain(batch) == 0
                    host_rows_writer_ms = (time.perf_counter() - t1) / nfr * 1e3
                for pb in pin_outs[1:]:
                    if pb:
                        l.dt_hip_free_host_pinned(pb)
                l.dt_hip_batch_free(batch)
            if rows_exec is not None:
                rows_exec.close()
        l.dt_hip_free_host_pinned(pin_in)
        l.dt_hip_free_host_pinned(pin_out)

    if rank == 0:
        from ansel_amd import modinfo
        # algorithmic bytes per pixel and launch of each tagged kernel: a fused
        # group is credited with the algorithmic bytes of the modules it executes
        tag_bpp = {"rawprepare_1f": 6, "temperature_1f": 8, "highlights_clip_1f": 8, "rcd_tiles": 20, "rcd_border": 0,
                   "ppg_full": 20, "amaze_tiles": 20, "exposure": 32, "colorin": 32, "channelmixerrgb": 32, "filmicrgb": 32,
                   "colorout": 32, "export_u16": 24, "dn_precondition": 32, "dn_decompose": 48, "dn_synthesize": 48,
                   "dn_finish": 48 + 32, "diffuse_decompose": 48, "diffuse_pde": 48, "nlm_chunks": 32, "rgb_to_lab": 32,
                   "lab_to_rgb": 32, "bilat_splat": 16, "bilat_slice": 32, "bilat_blur": 0, "bilat_lightness": 0}
        ops = [n.op for n in nodes]
        if not args.no_fusion:
            tag_bpp["raw_chain"] = sum(sum(pipe.MODULE_BPP[o]) for o in ops if o in ("rawprepare", "temperature", "highlights"))
            if args.pipe == "light":
                tag_bpp["rgb_chain_u16"] = sum(sum(pipe.MODULE_BPP[o]) for o in ops
                                               if o in ("exposure", "colorin", "channelmixerrgb", "filmicrgb", "colorout", "export_u16"))
            else:
                # denoise (profiled)'s last kernel carries exposure > colorin > calibration; the last PDE pass of diffuse
                # carries rgb_to_lab; the run behind the Lab section carries lab_to_rgb > filmic > colorout > u16
                tag_bpp["dn_finish_chain"] = 48 + 32 + 3 * 32
                tag_bpp["rgb_chain_u16"] = 32 + 2 * 32 + 24
                # round 6: local contrast's slice (32 B/px as a pass of its own) is the first stage of that run when the module sits in front of it
                if "bilat" in ops and ops.index("bilat") + 1 < len(ops) and ops[ops.index("bilat") + 1] == "lab_to_rgb":
                    tag_bpp["rgb_chain_u16"] += 32
        pmc, pmc_src = pmc_table(args)
        sclk, sclk_src = sclk_table(args)
        # the committed counter tables were taken on ONE build of the library: say whether it is the one running (round 5's advisor:
        # a kernel whose traffic changes without a re-profile made the figures derived from them stale without warning)
        lib_sha16 = _sha16(os.path.join(ROOT, "ansel_amd", "libansel_hip.so"))
        tables_sha16 = _table_sha16(pmc_src)
        mpix_mine = my_rows * width / 1e6
        ms_per_step = elapsed / args.steps * 1e3
        pipe_bpp = pipe.algorithmic_bytes_per_pixel(nodes)
        kernel_ms = sum(v["ms_avg"] * v["launches"] for v in kernels.values()) / args.steps
        # what binds each kernel of the step.  Per LAUNCH: hbm_frac = algorithmic bytes / time / 8 TB/s (the contract's
        # figure -- > 1 is possible for a fused group, whose credit is for bytes NOT moved); hbm_frac_moved = the bytes
        # the PMC counters saw / time / 8 TB/s (physical, always < 1); valu_frac = VALU issue floor / time
        per_kernel = {}
        for k, v in sorted(kernels.items()):
            per_launch = v["launches"] / float(args.steps)
            e = {"ms": round(v["ms_avg"], 4), "launches_per_step": round(per_launch, 2),
                 "ms_per_step": round(v["ms_avg"] * per_launch, 4), "bound": KERNEL_BOUND.get(k, "hbm")}
            # hbm_frac: the bytes the launch MOVED (PMC counters, committed summary) / its time / 8 TB/s -- physical, never above 1.
            # hbm_frac_algorithmic: SURVEY 8d's credit for the modules the launch executes / its time / 8 TB/s -- above 1 for a
            # fused group, whose credit is for bytes fusion does NOT move (round 4's review, item 8: a figure above 1 under the name
            # hbm_frac read as a defect)
            if tag_bpp.get(k):
                e["algorithmic_bytes_per_px"] = tag_bpp[k]
                e["hbm_frac_algorithmic"] = round(tag_bpp[k] * my_rows * width / (v["ms_avg"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            moved = traffic_of(pmc, k)
            if moved is not None:
                e["hbm_bytes_moved"] = moved
                e["hbm_frac"] = round(moved / (v["ms_avg"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                if tag_bpp.get(k):
                    e["moved_over_algorithmic"] = round(moved / float(tag_bpp[k] * my_rows * width), 3)
            floor = valu_floor_ms(k, mpix_mine)
            if floor is not None and k == "dn_decompose":
                # the tag's launches are of two kinds since round 6 -- seven decompositions and seven that leave at once (the
                # four-channel sequence behind the alpha flag) --: the floor of a STEP over the step's time, as a per-launch mean
                floor = valu_floor_step_ms(k, mpix_mine) / max(per_launch, 1.0)
            if floor is not None:
                # the instruction mix at the ARCHITECTURAL issue rates (2 / 4 / 8 cycles per full- / half- / quarter-rate wave64
                # instruction: what profiles/r05_valu_issue_cycles.json measures with the clock read beside it) at 2.4 GHz ...
                e["valu_issue_floor_ms"] = round(floor, 4)
                e["valu_frac"] = round(floor / v["ms_avg"], 4)
                clk = sclk_of(sclk, k)
                if clk:  # ... and at the clock the chip sustained during this kernel's launches (GRBM_GUI_ACTIVE / duration)
                    e["sclk_mhz"] = clk
                    e["valu_frac_at_sustained_clock"] = round(floor * 2400.0 / clk / v["ms_avg"], 4)
            per_kernel[k] = e
        # (denoise (profiled)'s wavelets likewise since round 6: the decompositions of bands 1 .. store their coarse plane only -- 16 B/px
        # less than SURVEY 8d's 48 each -- and dn_finish forms the details from consecutive coarse planes, reading the same nine planes)
        # diffuse or sharpen as a pair: the analysis stores ONE plane per scale (the PDE forms the detail from two low-pass
        # planes where it reads them), so its launches move 16 B/px less and the PDE's 16 more than SURVEY 8d's per-stage credit
        if "diffuse_pde" in per_kernel and "diffuse_decompose" in per_kernel \
           and "hbm_bytes_moved" in per_kernel["diffuse_pde"] and "hbm_bytes_moved" in per_kernel["diffuse_decompose"]:
            pd, dd = per_kernel["diffuse_pde"], per_kernel["diffuse_decompose"]
            per_kernel["diffuse_pair_moved_over_algorithmic"] = round(
                (pd["hbm_bytes_moved"] + dd["hbm_bytes_moved"]) / float((tag_bpp["diffuse_pde"] + tag_bpp["diffuse_decompose"]) * my_rows * width), 3)
        moved_per_step = sum(e["hbm_bytes_moved"] * e["launches_per_step"] for e in per_kernel.values()
                             if isinstance(e, dict) and "hbm_bytes_moved" in e)
        dominant = max((k for k in kernels if tag_bpp.get(k)), key=lambda k: kernels[k]["ms_avg"] * kernels[k]["launches"])
        dom = kernels[dominant]
        dom_bytes = tag_bpp[dominant] * my_rows * width  # rank 0's share of the frame in tiled mode
        achieved = dom_bytes / (dom["ms_avg"] * 1e-3) / 1e9
        traffic = traffic_of(pmc, dominant)
        line = {
            "metric": "MPix/s full export pixelpipe (100 MP raw); % MI355X HBM roofline",
            "value": round((1 if args.mode == "tiled" else world) * npix / 1e6 / (elapsed / args.steps), 2),
            "unit": "MPix/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong" if args.mode == "tiled" else "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": "%d x %d RGGB u16 raw (%s), %s export pipe: %s; module defaults%s; %s"
                            % (width, height, args.size, args.pipe, " > ".join(ops),
                               "" if args.pipe == "light" else " except diffuse or sharpen = the reference's 'lens deblur: soft' preset at %d "
                               "of its 8 iterations (%d B-spline analyses + %d PDE passes per frame; config.default_diffuse has the "
                               "module's $DEFAULT)" % (DIFFUSE_TIMED[1], 5 * DIFFUSE_TIMED[1], 5 * DIFFUSE_TIMED[1]),
                               "one frame cut into %d row bands, one per GPU (halo rows and the reductions over RCCL)" % world
                               if args.mode == "tiled" else "one frame per GPU"),
                "frame_mpix": round(npix / 1e6, 2),
                "executor": "dt_hip_pipe_process, %d launch groups (fusion %s)" % (executor.num_groups, "off" if args.no_fusion else "on"),
                "pipe_algorithmic_bytes_per_px": pipe_bpp,
                # the metric's second half: the whole step against the HBM roofline of its algorithmic bytes
                "pipe_hbm_frac": round(pipe_bpp * my_rows * width / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "pipe_kernel_ms": round(kernel_ms, 4),
                "kernels_ms_per_step": {k: round(v["ms_avg"] * v["launches"] / args.steps, 3) for k, v in sorted(kernels.items())},
                "kernel_bounds": per_kernel,
                "pmc_source": pmc_src,
                "lib_sha16": lib_sha16,
                # True: traffic / hbm_frac / sclk_mhz / valu_frac_at_sustained_clock / pipe_frac_counter_bytes describe THIS build;
                # False: a build since the tables were taken (re-run tools/profile_round.sh); None: tables without a recorded build
                "counter_tables_match_this_build": None if tables_sha16 is None else tables_sha16 == lib_sha16,
                "light_pipe": light,
                "default_diffuse": default_diffuse,
                "full_pipe_24MP": full24,
                # not `value`: one frame from pinned host memory to pinned host memory over PCIe
                "host_to_host_ms": None if host_ms is None else round(host_ms, 3),
                "host_to_host_overlapped_ms": None if host_overlap_ms is None else round(host_overlap_ms, 3),
                "host_to_host_overlapped_rgb_rows_ms": None if host_rows_ms is None else round(host_rows_ms, 3),
                "host_to_host_overlapped_rgb_rows_and_writer_ms": None if host_rows_writer_ms is None else round(host_rows_writer_ms, 3),
                # which leg binds a stream of exports of this frame: the overlapped host-to-host time over the kernels' own (~1: the
                # kernels; well above 1: the bus)
                "host_to_host_overlapped_over_step": None if host_overlap_ms is None else round(host_overlap_ms / ms_per_step, 3),
                "host": {"nproc": os.cpu_count(), "cpu_quota": cgroup_cpu_quota(), "affinity": len(os.sched_getaffinity(0))},
            },
            "roofline": {
                # the contract's figure for the launch with the largest share of the step: algorithmic bytes of the
                # module(s) it executes / its average duration (HIP events on the launch stream) / HBM peak
                # what binds the dominant launch (the contract's "hbm" | "mfma" does not cover a kernel bound by VALU issue and
                # the LDS pipe; achieved / peak / frac below stay the HBM figures the contract asks for)
                "bound": per_kernel.get(dominant, {}).get("bound", "hbm"),
                "kernel": dominant,
                "share_of_step": round(dom["ms_avg"] * dom["launches"] / args.steps / max(kernel_ms, 1e-9), 3),
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                # the ceiling measured in this run on this device: device-to-device copy and triad (GB/s of bytes moved)
                "peak_measured": ceiling,
                "traffic": traffic,
                "traffic_source": pmc_src if traffic is not None else None,
                # ... and what actually binds this launch (config.kernel_bounds has every kernel of the step)
                "binds": per_kernel.get(dominant, {}).get("bound"),
                "valu_frac": per_kernel.get(dominant, {}).get("valu_frac"),
                "valu_frac_at_sustained_clock": per_kernel.get(dominant, {}).get("valu_frac_at_sustained_clock"),
                "sclk_mhz": per_kernel.get(dominant, {}).get("sclk_mhz"),
                "sclk_source": sclk_src,
                # "for NLM report achieved fraction of fp32 VALU peak and of HBM, and say which binds"
                "fp32_valu": fp32_valu_figure(dominant, dom, my_rows * width, nodes),
                # the whole step, both ways: sum of ALGORITHMIC bytes / step time / peak (= config.pipe_hbm_frac: the metric's figure;
                # it credits the pipe with bytes that fusion never moves) and the bytes the PMC counters saw the step MOVE / step time / peak
                "pipe_frac": round(pipe_bpp * my_rows * width / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "pipe_frac_counter_bytes": None if not moved_per_step else round(moved_per_step / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "pipe_counter_bytes_per_step": None if not moved_per_step else int(moved_per_step),
                "pipe_frac_of_measured_copy": None if not ceiling else round(pipe_bpp * my_rows * width / (ms_per_step * 1e-3) / 1e9 / ceiling["copy_GBs"], 4),
            },
        }
        if tiled_check is not None:
            line["verified"] = tiled_check["verified"]
            line["verify"] = tiled_check
        if verify is not None:
            line["verified"] = verify["verified"]
            line["verify"] = verify
        if args.full and world == 1 and not args.no_cpu_baseline:
            sample = args.cpu_sample or "24MP"
            cb = cpu_baseline_in_child(sample, with_filmic, args.pipe, (width, height))
            if cb is not None:
                line["cpu_baseline"] = cb
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
