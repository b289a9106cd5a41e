"""not gpu: the one rule that picks the strip length of the strip kernels (hip_common.h strip_rows()), its test override,
and the frames tests/test_gpu_strip_rows.py runs under the override.

The rule keeps a workgroup on its 256 columns for the longest strip -- 32, 16, 8 or 4 rows -- that still leaves 2048
workgroups.  Frames of the size the module tests can afford get 4; the frames of the benchmark, and every real export, get
32.  So the tests force the length ("strip_rows" of dt_hip_test_dispatch()), and this file pins on the CPU (1) that the rule
without an override is the loop the four launch sites used to spell out, (2) what the override accepts, (3) that no launch
site kept a copy of the loop, and (4) that the small frames of tests/strip_cases.py really give the strips they are there
for: several strips a class, partial last ones, the empty one, and strips long enough to turn the rings over."""
import ctypes as C
import os
import re

import pytest

import checkers as ck
import strip_cases as sc
from ansel_amd import abi, lib, params, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BENCH_FRAMES = [(6000, 4000), (8256, 5504), (9504, 6336), (11648, 8736)]
MODULE_TEST_FRAME = (1536, 1100)  # the largest frame of the module tests
DILATIONS = (1, 2, 4, 8, 16, 32, 64)


def old_loop(gx, classes, per_class, longest=32):
    """the loop launch_decompose(), pde_strip_launch(), bspline_launch_decompose() and bspline_launch_decompose3() each had"""
    strip = longest
    while strip > 4 and gx * classes * ((per_class + strip - 1) // strip) < 2048:
        strip //= 2
    return strip


def site_grids(w, h, mult):
    """(gx, classes, per_class) of every launch site for one frame and dilation: a workgroup a span of 256 columns (the
    wavelets, the PDE, the three-float analysis), and the float4 analysis' column groups (bspline_launch_decompose())"""
    classes, per_class = min(h, mult), (h + mult - 1) // mult
    steps = (w + mult - 1) // mult
    if mult <= 4:
        per_group = 256 // mult
        gx_bspline = (steps + per_group - 1) // per_group
    else:
        gx_bspline = ((steps + 31) // 32) * (mult // 8)
    return [((w + 255) // 256, classes, per_class), (gx_bspline, classes, per_class)]


@pytest.fixture
def strip_override():
    def force(value):
        lib.test_dispatch("strip_rows", value)
    yield force
    lib.test_dispatch("strip_rows", 0)


def _pinned_grid():
    grid = []
    for w, h in BENCH_FRAMES + [MODULE_TEST_FRAME, (640, 401), (520, 131), (300, 200), (259, 131), (300, 97), (1, 1), (257, 19)]:
        for mult in DILATIONS + (128, 256, 512):
            grid += site_grids(w, h, mult)
    # and the corners of the rule itself: either side of 2048 workgroups at every length
    for gx in (1, 2, 3, 7, 8, 24, 46, 47, 64, 2047, 2048, 2049, 70000):
        for classes in (1, 2, 3, 16, 64):
            for per_class in (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4000, 70000):
                grid.append((gx, classes, per_class))
    return grid


def test_the_rule_is_the_loop_the_launch_sites_had():
    lib.test_dispatch("strip_rows", 0)
    seen = set()
    for gx, classes, per_class in _pinned_grid():
        got = lib.test_strip_rows(gx, classes, per_class)
        assert got == old_loop(gx, classes, per_class), (gx, classes, per_class, got)
        seen.add(got)
    assert seen == {4, 8, 16, 32}


def test_bench_frames_get_32_rows_and_the_module_tests_frames_4():
    """why the override exists: no frame a module test can afford reaches the strip length every real frame runs at"""
    lib.test_dispatch("strip_rows", 0)
    for w, h in BENCH_FRAMES:
        for mult in DILATIONS:
            for gx, classes, per_class in site_grids(w, h, mult):
                assert lib.test_strip_rows(gx, classes, per_class) == 32, (w, h, mult, gx)
    for w, h in [MODULE_TEST_FRAME, (640, 401)]:
        for mult in DILATIONS:
            for gx, classes, per_class in site_grids(w, h, mult):
                assert lib.test_strip_rows(gx, classes, per_class) == 4, (w, h, mult, gx)


def test_the_override(strip_override):
    w, h = MODULE_TEST_FRAME
    grids = [g for mult in DILATIONS for g in site_grids(w, h, mult)] + [g for mult in DILATIONS for g in site_grids(11648, 8736, mult)]
    for value in (4, 8, 16, 32):
        strip_override(value)
        assert [lib.test_strip_rows(*g) for g in grids] == [value] * len(grids)
    strip_override(0)
    assert [lib.test_strip_rows(*g) for g in grids] == [old_loop(*g) for g in grids]
    strip_override(16)
    l = lib.load()
    for refused in (5, 64, 1, 2, 3, 12, 33, -4, -32, 128):
        assert l.dt_hip_test_dispatch(b"strip_rows", refused) == abi.DT_HIP_INVALID_ARG, refused
        assert lib.test_strip_rows(*grids[0]) == 16  # a refused value leaves what was set
    with pytest.raises(lib.AnselHipError):
        lib.test_dispatch("strip_rows", 64)
    # the other keys take any value, as before
    assert l.dt_hip_test_dispatch(b"amaze_blocks", 5) == abi.DT_HIP_SUCCESS
    assert l.dt_hip_test_dispatch(b"amaze_blocks", 0) == abi.DT_HIP_SUCCESS


def test_no_launch_site_keeps_a_copy_of_the_rule():
    csrc = os.path.join(ROOT, "ansel_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".cpp", ".h"))
               and "while(strip > 4" in open(os.path.join(csrc, f), errors="replace").read()]
    assert holders == ["hip_common.h"], holders
    # ... and the five sites call it
    calls = {f: len(re.findall(r"\bstrip_rows\(", open(os.path.join(csrc, f)).read()))
             for f in ("denoiseprofile.hip", "diffuse.hip", "diffuse_bspline.hip")}
    assert calls == {"denoiseprofile.hip": 1, "diffuse.hip": 1, "diffuse_bspline.hip": 3}, calls


# ---- the frames of tests/strip_cases.py ---------------------------------------------------------------------------------
def test_frames_are_small_and_the_rule_gives_them_4_rows():
    lib.test_dispatch("strip_rows", 0)
    for w, h, bands in sc.WAVELET_FRAMES:
        assert w * h < 300000
        for mult in sc.wavelet_dilations(bands):
            assert lib.test_strip_rows((w + 255) // 256, min(h, mult), (h + mult - 1) // mult) == 4
    for _, _, (w, h), scales in sc.DIFFUSE_FRAMES:
        assert w * h < 300000
        for mult in sc.diffuse_dilations(scales):
            for g in site_grids(w, h, mult):
                # (the float4 analysis has 2048 workgroups of one row each where a class is one row: no strip to speak of)
                assert min(lib.test_strip_rows(*g), g[2]) <= 4, (w, h, mult, g)
    assert sc.WAVELET_BAND_FRAME in sc.WAVELET_FRAMES


def test_frames_run_the_dilations_the_list_says():
    """the wavelet bands and the scales of diffuse-or-sharpen as the library and the oracle count them (host code)"""
    l = lib.load()
    for w, h, bands in sc.WAVELET_FRAMES:
        t = abi.Tiling()
        d = params.denoiseprofile()
        l.dt_hip_iop_denoiseprofile_tiling(C.byref(abi.Piece.make(w, h, processed_maximum=synth.WB_COEFFS)), C.byref(d), C.byref(t))
        assert t.overlap == 1 << bands, (w, h, t.overlap)
        assert w >= 4 << (bands - 1) and h >= 2 << (bands - 1)  # the module runs (neither copies through nor refuses)
    for preset, over, (w, h), scales in sc.DIFFUSE_FRAMES:
        d = params.diffuse(preset, **over)
        assert ck.oracle().oracle_diffuse_scales(C.byref(abi.Piece.make(w, h)), C.byref(d)) == scales, (preset, scales)


def test_class_arithmetic_on_the_frame_checked_by_hand():
    """520 x 131: dilation 4 has classes of 33, 33, 33 and 32 rows; at 32 rows a strip that is a last strip of one row and,
    for the class of 32, a second strip that is empty"""
    assert sc.class_rows(131, 4) == [33, 33, 33, 32]
    assert sc.strip_lengths(33, 33, 32) == [32, 1] and sc.strip_lengths(32, 33, 32) == [32, 0]
    assert sc.kinds_of(131, 4, 0, 32) == {sc.PARTIAL_LAST, sc.LAST_OF_ONE, sc.RING_TWICE}
    assert sc.kinds_of(131, 4, 3, 32) == {sc.EMPTY_STRIP, sc.RING_TWICE}
    assert sc.class_rows(131, 1) == [131] and sc.strip_lengths(131, 131, 32) == [32, 32, 32, 32, 3]
    assert sc.class_rows(131, 32)[:4] == [5, 5, 5, 4] and sc.kinds_of(131, 32, 3, 8) == {sc.SHORT_SINGLE}
    assert sc.class_rows(3, 8) == [1, 1, 1]  # fewer rows than classes
    # every row of a frame is in exactly one strip of one class
    for h in (131, 200, 97, 1, 7):
        for mult in (1, 2, 4, 8, 16, 32, 64):
            for strip in sc.FORCED:
                assert sum(sum(lengths) for _, _, _, lengths, _ in sc.strips_of(h, (mult,), strip)) == h


@pytest.mark.parametrize("strip", sc.FORCED)
def test_frames_hold_every_kind_of_strip(strip):
    """a condition on the INPUTS of tests/test_gpu_strip_rows.py: at each forced length the wavelets' frames, and the frames
    added for diffuse-or-sharpen at the dilations 1 .. 16 of its three-float sequence (analysis and PDE alike), hold a
    (dilation, class) with several strips and a partial last one, one whose last strip is a single row, one whose class is
    a whole number of strips beside a longer class (the grid's empty strip), one single short strip, and a strip of 13 rows
    or more -- at 8 rows a strip, where 13 cannot be, a full strip (strip_cases.required_kinds())"""
    required = set(sc.required_kinds(strip))
    assert len(required) == 5
    for name, family in (("wavelets", sc.wavelet_family()), ("diffuse, analysis", sc.diffuse_family(low_only=True)),
                         ("diffuse, PDE", sc.diffuse_family(pde=True, low_only=True))):
        missing = required - sc.kinds_in(family, strip)
        assert not missing, (name, strip, sorted(missing))
    assert sc.RING_TWICE in sc.required_kinds(16) and sc.RING_TWICE in sc.required_kinds(32)
