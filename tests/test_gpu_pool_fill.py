"""-m gpu: no module's output may depend on what the runtime's pool held.

The pool hands a released block to the next allocation of the same rounded size, so the second call of a module at a
shape finds the first call's planes, offsets and partial sums in its scratch, and the first call finds the zeros of a
fresh allocation: a kernel that skips a border row, a padded segment or a ragged last chunk reads a correct or a neutral
value there, and every other test passes.  dt_hip_test_pool_fill() (csrc/runtime.cpp; hc.pool_fill()) fills every block
the pool hands out with one 32-bit word first.  Each case below runs under four words:

  00000000  the control: what a fresh allocation gives
  ffffffff  NaN as binary32 and binary64, -1 / 65535 / 255 as integers
  7149f2ca   1.0e30f: finite, and no clamp or comparison swallows it as they swallow a NaN
  f149f2ca  -1.0e30f: half the clamps are one-sided; a zero weight swallows either (0 * 1e30 = 0) but not the NaN

and must be what it is with the hook off: the oracle's words (the exporters: their host twins' bytes), with the masks
the case's own test uses and no tolerance.  The cases are the existing tests' functions and builders, called at the
smallest of their shapes that has two tiles, chunks or strips and a ragged last one; their comparisons are not restated
here.  The output buffer holds the word as well, on the device and in the oracle, in the cases that go through
edge_cases.case() (2 x len(MODULES) of them; not under the blend, whose output is an input) and in rcd-207x131-roi11.
Every other named case is another test's function and keeps the output that test chose: where it goes through
hc.run_hip() that is an upload of zeros (-7.0 in the demosaic cases of edge_cases), so those cases put the word into the
modules' scratch only; where it takes its output with lib.DeviceBuffer(0, n) without an upload (the executor's walks,
the bands, the tilers, the encoders) the output holds the word too.

The buffers whose words are addresses (offsets, lengths, counters, flags) were read through before the first run:
DESIGN.md section 3 has the table."""
import functools
import struct

import numpy as np
import pytest

import hipcheck as hc
from ansel_amd import abi, lib

pytestmark = pytest.mark.gpu


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


PATTERNS = [0x00000000, 0xFFFFFFFF, _bits(1.0e30), _bits(-1.0e30)]
assert PATTERNS[2:] == [0x7149F2CA, 0xF149F2CA]


@pytest.fixture(autouse=True, scope="module")
def _hook_off_behind_the_module():
    """whatever happened in here, the hook is left as the process runs (off, unless ANSEL_TEST_POOL_FILL asks for it)"""
    yield
    hc.pool_fill_default()


# ---- the hook itself ------------------------------------------------------------------------------------------------
def _words(nbytes, asked=None):
    """a block of the pool that nothing is uploaded to -- `asked` bytes asked for, `nbytes` its rounded size -- read back
    whole and released"""
    b = lib.DeviceBuffer(0, nbytes if asked is None else asked)
    assert hc.hip().dt_hip_get_mem_object_size(b.ptr) == nbytes
    b.nbytes = nbytes
    out = b.to_numpy((nbytes // 4,), np.uint32)
    b.release()
    return out


@pytest.mark.parametrize("pattern", PATTERNS[1:], ids=["p%08x" % p for p in PATTERNS[1:]])
def test_the_fill_reaches_fresh_and_pooled_blocks_and_ends_with_the_with(pattern):
    hc.hip()
    # a size in 256-byte granules that nothing else in the suite asks for, one per pattern: its first block is a fresh one
    nbytes = (4 << 20) + 1024 * (1 + PATTERNS.index(pattern)) + 256
    other = ~pattern & 0xFFFFFFFF
    outer = hc._state.get("fill")  # None, or the pattern the whole process runs under
    with hc.pool_fill(pattern):
        assert (_words(nbytes) == pattern).all(), "a size never allocated before"
        # the block just released holds the pattern already: overwrite it, release it, take it again
        b = lib.DeviceBuffer.from_numpy(0, np.full(nbytes // 4, other, np.uint32))
        ptr = b.ptr
        b.release()
        b = lib.DeviceBuffer(0, nbytes)
        assert b.ptr == ptr, "the pool did not hand the released block out again"
        got = b.to_numpy((nbytes // 4,), np.uint32)
        b.release()
        assert (got == pattern).all(), "a size just released"
        # the whole rounded block, not only the bytes asked for
        lib.DeviceBuffer.from_numpy(0, np.full(nbytes // 4, other, np.uint32)).release()
        assert (_words(nbytes, asked=nbytes - 252) == pattern).all(), "the rounded tail of a block"
        lib.DeviceBuffer.from_numpy(0, np.full(nbytes // 4, other, np.uint32)).release()
    assert (_words(nbytes) == (other if outer is None else outer)).all(), "the fill did not end with the with"


def test_nested_fills_restore_the_outer_pattern():
    hc.hip()
    nbytes = (4 << 20) + 8192 + 256
    with hc.pool_fill(0x11111111):
        with hc.pool_fill(0x22222222):
            assert (_words(nbytes) == 0x22222222).all()
        assert (_words(nbytes) == 0x11111111).all()


# ---- the cases ------------------------------------------------------------------------------------------------------
class _Dispatch:
    """what the `dispatch` fixture of the modules' tests hands them: dt_hip_test_dispatch() keys, cleared by clear()"""

    def __init__(self):
        self.keys = []

    def __call__(self, key, value=1):
        lib.test_dispatch(key, value)
        self.keys.append(key)

    def clear(self):
        for k in self.keys:
            lib.test_dispatch(k, 0)


def _with_dispatch(fn, *args):
    """fn(*args, dispatch), as pytest calls a test that takes the `dispatch` fixture"""
    def run(_pattern):
        d = _Dispatch()
        try:
            fn(*args, d)
        finally:
            d.clear()
    return run


def _forced(key, fn, *args):
    """fn(*args) with the launches sent to the fallback kernel `key`"""
    def run(_pattern):
        d = _Dispatch()
        try:
            d(key)
            fn(*args)
        finally:
            d.clear()
    return run


def _call(fn, *args):
    return lambda _pattern: fn(*args)


@functools.lru_cache(maxsize=None)
def _tables():
    import pipe_cases as pc
    hc.hip()
    return pc.Tables(True), pc.Tables(False)


@functools.lru_cache(maxsize=None)
def _jpeg_noise():
    import jpeg_ref as jr
    img = jr.frame("noise", 1001, 777, seed=5)
    return img, jr.encode(img, 95, 0, 1)


def _jpeg_noise_case(_pattern):
    """1001 x 777 noise at quality 95: several chunks of byte stuffing, several workgroups' partial sums"""
    import test_gpu_jpeg as tj
    img, want = _jpeg_noise()
    assert tj.encode_dev(img, 95, 0, 1) == want


def _batch_ending_in_a_demosaic(_pattern):
    """a batch owns its slots' output buffers, the host cannot put anything there: where the pipe's last node leaves the
    fourth channel alone (RCD: on the border ring), every frame must carry the zeros of oracle_chain(fill=0.0) there"""
    import pipe_cases as pc
    from ansel_amd import pipe, synth
    w, h = 207, 131
    src = ((synth.bayer_mosaic(w, h, seed=3).astype(np.float32) - np.float32(synth.BLACK))
           / np.float32(synth.WHITE - synth.BLACK)).astype(np.float32)
    cfa = abi.Piece.make(w, h, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=(1.0, 1.0, 1.0, 1.0))
    nodes = [pipe.Node("demosaic", abi.DemosaicData(0, 0, abi.DT_HIP_DEMOSAIC_RCD, 0.0), cfa)]
    want = pc.oracle_chain(nodes, src)
    for k, got in enumerate(pc.device_batch(nodes, src, depth=2, frames=3)):
        assert pc.count_differing(got, want) == 0, "frame %d" % k


def _cases():
    import blend_cases
    import edge_cases as ec
    import pipe_cases as pc
    import png_ref as pr
    import test_gpu_amaze as tam
    import test_gpu_basebuffer as tbb
    import test_gpu_basic as tba
    import test_gpu_batch as tbt
    import test_gpu_bilat as tbi
    import test_gpu_c_example as tce
    import test_gpu_blend as tbl
    import test_gpu_color as tco
    import test_gpu_demosaic as tde
    import test_gpu_denoiseprofile as tdn
    import test_gpu_diffuse as tdi
    import test_gpu_diffuse_three_float as td3
    import test_gpu_edge_sizes as tes
    import test_gpu_export_rows as ter
    import test_gpu_finalscale as tfs
    import test_gpu_fused_variants as tfv
    import test_gpu_host_tiling as tht
    import test_gpu_jpeg as tj
    import test_gpu_nlmeans as tnl
    import test_gpu_pipe as tpi
    import test_gpu_pipe_generated as tpg
    import test_gpu_png as tpn
    import test_gpu_raw_unpack as tru
    import test_gpu_tiff as tti
    import test_gpu_tiled as ttl

    D = abi
    c = []
    # every module, small: 36 x 34 is the smallest frame on which all of them are defined
    for w, h in ((36, 34), (207, 131)):
        for m in ec.MODULES:
            c.append(("%s-%dx%d" % (m, w, h), lambda p, m=m, w=w, h=h: tes.check_case(m, w, h, out_fill=p)))
    # the demosaics: RCD's tile is 112 x 112 (2 x 2 ragged tiles)
    c += [
        ("rcd-207x131-roi11", lambda p: tde.check_rcd(207, 131, (1, 1), out_fill=p)),
        ("ppg-65x40", _call(tde.test_ppg, 65, 40)),
        ("vng4-19x17", _call(tde.test_vng4, 19, 17, (0, 0))),
        ("vng4-207x131", _call(tde.test_vng4, 207, 131, (1, 1))),
        ("amaze-130x97", _call(tam.test_amaze, 130, 97, 0x94949494)),
        ("amaze-273x273", _call(tam.test_amaze, 273, 273, 0x16161616)),
        ("amaze_unfused-273x273", _forced("amaze_unfused", tam.test_amaze, 273, 273, 0x94949494)),
        ("amaze_slab-273x273", _forced("amaze_slab", tam.test_amaze, 273, 273, 0x94949494)),
        ("amaze_slab-130x97", _forced("amaze_slab", tam.test_amaze, 130, 97, 0x16161616)),
        ("dual-207x131", _call(tde.test_dual_demosaic, 207, 131, (1, 1), D.DT_HIP_DEMOSAIC_RCD, 1, 2, 0.05)),
        ("green_eq_favg-207x131", _call(tde.test_full_average_green_equilibration, 207, 131, (1, 1), 2, D.DT_HIP_DEMOSAIC_RCD)),
        ("green_eq_favg_lavg-207x131", _call(tde.test_full_average_green_equilibration, 207, 131, (1, 1), 3, D.DT_HIP_DEMOSAIC_PPG)),
        ("median_smoothing-120x96", _call(tde.test_demosaic_optional_steps, 120, 96, (0, 1), D.DT_HIP_DEMOSAIC_PPG, 1, 2, 0.02, 0.08)),
        ("passthrough_mono", _call(tde.test_passthrough, 207, 131, (1, 1), D.DT_HIP_DEMOSAIC_PASSTHROUGH_MONOCHROME, 0, 0)),
        ("passthrough_color", _call(tde.test_passthrough, 207, 131, (1, 1), D.DT_HIP_DEMOSAIC_PASSTHROUGH_COLOR, 1, 2)),
        ("highlights-66x34-25", _call(tba.test_highlights_clip_bayer, 66, 34, 25)),
    ]
    # non-local means: the body a frame takes follows its chunk grid (tests/test_gpu_nlmeans.py)
    g0 = tnl.R6_GRIDS[0]
    c += [
        ("nlm-73x61", _call(tnl.test_nlmeans, 73, 61, 2.0, 50.0, 0.5, 1.0)),
        ("nlm-330x168-v3-v2", _with_dispatch(tnl.test_nlmeans_third_version_chunk_grids, 330, 168, 0.5, 1.0)),
        ("nlm-260x192-fused", _with_dispatch(tnl.test_nlmeans_fused_variant_chunk_grids, 260, 192, 0.5, 1.0)),
        ("nlm-330x168-nlm_fused", _with_dispatch(tnl.test_nlmeans_fused_variant_on_the_third_versions_grids, 330, 168)),
        ("nlm-260x207-tall", _with_dispatch(tnl.test_nlmeans_tall_chunk_grids, 260, 207, 0.5, 1.0)),
        ("nlm-radius1", _with_dispatch(tnl.test_nlmeans_patch_radius_one_on_the_third_version, *g0)),
        ("nlm-radius5", _call(tnl.test_nlmeans_large_patch_radius_takes_the_fallback_kernels, 5.0)),
        ("dn_nlm", _with_dispatch(tnl.test_denoiseprofile_nlmeans_on_the_third_version, g0[0], g0[1], dict())),
    ]
    # denoise (profiled), wavelets: the smallest frame of its CASES; the auto mode; the band job given up half way
    small = min(range(len(tdn.CASES)), key=lambda k: tdn.CASES[k][1][0] * tdn.CASES[k][1][1])
    c += [
        ("dn_wavelets-smallest", _call(tdn.test_denoiseprofile_matches_oracle, small)),
        ("dn_wavelets-auto", _call(tdn.test_auto_modes_run_like_their_manual_mode, D.DT_HIP_DENOISEPROFILE_WAVELETS_AUTO,
                                   D.DT_HIP_DENOISEPROFILE_WAVELETS)),
        ("dn_band_job_abandoned", _call(tdn.test_band_job_given_up_inside_the_wavelets_returns_its_planes)),
        ("bilat-123x457-8-5", _call(tbi.test_bilat, 123, 457, 8.0, 5.0, -0.5)),
        ("bilat-123x457-0.3-2", _call(tbi.test_bilat, 123, 457, 0.3, 2.0, 1.5)),
        ("local_laplacian-257x130", _call(tbi.test_local_laplacian, 257, 130, 0.5, 0.5, 0.25, 0.5)),
    ]
    # diffuse or sharpen
    soft = "lens_deblur_soft"
    c += [
        ("diffuse-256x192-it1", _call(tdi.test_diffuse_matches_cpu, soft, dict(iterations=1), (256, 192), "scene")),
        ("diffuse-256x192-it3", _call(tdi.test_diffuse_matches_cpu, soft, dict(iterations=3), (256, 192), "scene-patches")),
        ("diffuse-256x192-threshold", _call(tdi.test_diffuse_matches_cpu, soft, dict(iterations=2, threshold=0.6), (256, 192), "scene")),
        ("diffuse-inpaint", _call(tdi.test_diffuse_luminance_masked_inpainting, "inpaint_highlights", dict(iterations=2, threshold=1.41),
                                  (256, 192), "scene")),
        ("diffuse-three_float", _call(td3.test_three_float_sequence_equals_the_oracle, soft, dict(iterations=3), (256, 192), False)),
        ("diffuse-three_float-in_place", _call(td3.test_three_float_sequence_equals_the_oracle, soft, dict(iterations=3), (256, 192), True)),
        ("diffuse-one_iteration-in_place", _call(td3.test_three_float_sequence_equals_the_oracle, soft, dict(iterations=1), (256, 192), True)),
        ("diffuse-float4-alpha", _call(td3.test_alpha_words_not_plus_zero_take_the_float4_sequence, "one_word", td3.FLOAT4, soft,
                                       dict(iterations=2), False)),
        ("diffuse-float4-alpha-in_place", _call(td3.test_alpha_words_not_plus_zero_take_the_float4_sequence, "minus_zero", td3.FLOAT4,
                                                "default", dict(iterations=2), True)),
    ]
    # the resamplers, the blend's mask operations, the other pointwise paths
    blur, feather = tbl.BLUR_CASES[0], tbl.FEATHER_CASES[0]
    detail = tbl.DETAIL_CASES[0]
    c += [
        ("finalscale-301x199-0.37", _call(tfs.test_finalscale, 2, 301, 199, 0.37)),
        ("finalscale-97x61-2.75", _call(tfs.test_finalscale, 2, 97, 61, 2.75)),
        ("initialscale-33x29-0.2", _call(tfs.test_initialscale, 2, 33, 29, 0.2, 1, 2, 5, 3)),
        ("blend-blur-131x67", _call(tbl.test_blend_mask_blur, blur[0], blur[1], blur[2], 131, 67)),
        ("blend-blur-40x3", _call(tbl.test_blend_mask_blur, blur[0], blur[1], blur[2], 40, 3)),
        ("blend-feather-131x67", _call(tbl.test_blend_mask_feathering, feather[0], feather[1], feather[2], 131, 67)),
        ("blend-feather-40x3", _call(tbl.test_blend_mask_feathering, feather[0], feather[1], feather[2], 40, 3)),
        ("detailmask-37x23", _call(tbl.test_detailmask_stage, 37, 23, (1.0, 1.0, 1.0))),
        ("blend-details_threshold", _call(tbl.test_blend_details_threshold_from_the_raw_detail_mask, *detail)),
        ("lab_glue-tone_curves", _call(tco.test_lab_glue_linear_and_with_the_tone_curves_of_the_work_profile, "scene", (1, 1, 1))),
        ("raw_unpack-131x7-12", _call(tru.test_raw_unpack, 12, D.RAW_PACK_MSB, 131, 7, 5)),
        ("pack_rows-131x67", _call(ter.test_pack_rows, 131, 67, np.uint16, 16, 3)),
        ("basebuffer", _call(tbb.test_basebuffer_crop_upload, np.uint16, 2, (16, 8, 200, 150))),
    ]
    # the executor
    pairs = tfv._PAIR_NAMES
    c += [
        ("pipe-light-400x300", _call(tpi.test_fused_pipe_equals_modulewise_and_cpu, 400, 300)),
        ("pipe-denoise", _call(tpi.test_denoise_pipe_executor_equals_modulewise_and_oracle)),
        ("pipe-config3-nlmeans-cells", _call(tpi.test_full_config3_pipe_with_nlmeans)),
    ]
    c += [("pipe-generated-%d" % s, _call(tpg.test_generated_pipe, s)) for s in pc.SEEDS[:3]]
    # what the whole suite under ffffffff found: a demosaic's fourth channel, left to the caller, came out of
    # the pool where the executor is the caller and no later node writes it -- seed 43, and the C example's pipe (no colorin)
    c += [
        ("pipe-generated-43", _call(tpg.test_generated_pipe, 43)),
        ("pipe-c_example", _call(tce.test_c_example_exports_the_same_bytes)),
    ]
    c += [
        ("pipe-generated-scaled-%d" % pc.SCALED_SEEDS[0], _call(tpg.test_generated_pipe_at_a_region_scale, pc.SCALED_SEEDS[0])),
        ("pipe-pair-" + pairs[0], lambda p: tfv.test_fused_pairs_and_their_fallbacks(_tables(), pairs[0])),
        ("pipe-pair-wavelets+run_with_filmic", lambda p: tfv.test_fused_pairs_and_their_fallbacks(_tables(), "wavelets+run_with_filmic")),
    ]
    # row bands (two drivers), a band walk given up, the host tilers, a batch of frames
    c += [
        ("bands-400x640-2-everything", _call(ttl.test_full_pipe_bands_equal_the_unsplit_frame, 400, 640, 2, "everything")),
        ("bands-400x640-2-everything-c_driver", _call(ttl.test_c_driver_full_pipe_equals_the_unsplit_frame, 400, 640, 2, "everything")),
        ("bands-oracle", _call(ttl.test_full_pipe_bands_equal_the_oracle)),
        ("bands-abort", _call(ttl.test_band_abort_frees_what_a_stopped_walk_holds, "everything")),
        ("host_tiling-diffuse", _call(tht.test_host_tiling_equals_the_oracle_over_the_same_tiles, "diffuse", False, 333, 517, 0.12)),
        ("host_tiling-demosaic", _call(tht.test_host_tiling_equals_the_oracle_over_the_same_tiles, "demosaic", False, 333, 517, 0.12)),
        ("host_tiling-finalscale", _call(tht.test_roi_host_tiling_of_finalscale_equals_the_oracle_over_the_same_tiles, 1201, 803, 0.37, 0.15, 2)),
        ("batch-depth2", _call(tbt.test_batch_of_frames_equals_serial, 2)),
        ("batch-ends-in-demosaic", _batch_ending_in_a_demosaic),
    ]
    # the exporters: byte for byte their host twins
    c += [("jpeg-17x33-ss%d-opt%d" % (ss, opt), _call(tj.test_bytes_equal_reference, 17, 33, ss, opt)) for ss in (0, 1, 2) for opt in (0, 1)]
    c += [
        ("jpeg-1001x777-noise-q95", _jpeg_noise_case),
        ("jpeg-capacity", _call(tj.test_capacity_exact_and_one_short)),
    ]
    c += [("png-%dx%d-%d" % (w, h, depth), _call(tpn.test_device_file_equals_host_build, w, h, depth))
          for (w, h) in sorted(pr.SIZES, key=lambda s: s[0] * s[1])[:2] for depth in (8, 16)]
    scan = next(e for e in tpn.EDGES if e[0] == "scan_257")
    c += [
        ("png-scan_257", _call(tpn.test_edge_frame_device_file_equals_host_build, *scan)),
        ("png-table_builder", _call(tpn.test_table_builder_device_equals_host_and_holds_the_code_properties)),
        ("tiff-37x13_rps5_8_3", _call(tti.test_device_file_equals_host_build, "37x13_rps5_8_3")),
        ("tiff-three_segments", _call(tti.test_device_file_equals_host_build, "three_segments")),
        ("tiff-predictor3", _call(tti.test_device_file_equals_host_build, "37x13_rps5_32_3")),
        ("tiff-capacity_short", _call(tti.test_capacity_short, "37x13_rps5_8_3", 6)),
    ]
    return c


CASES = _cases()
_BY_NAME = dict(CASES)
assert len(_BY_NAME) == len(CASES)


# (the pattern is the outer loop: the control runs first)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
@pytest.mark.parametrize("pattern", PATTERNS, ids=["p%08x" % p for p in PATTERNS])
def test_output_does_not_depend_on_what_the_pool_held(pattern, name):
    h = hc.hip()
    if h.dt_hip_finish(0) != 1:  # a fault in an earlier case: nothing more is started on the device
        pytest.exit("the device's stream reports an error (%s): stopping here" % h.dt_hip_last_error().decode(), returncode=3)
    with hc.pool_fill(pattern):
        _BY_NAME[name](pattern)
