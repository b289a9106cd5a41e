"""-m gpu: the modules whose code branches on the regions' scale, run at roi_in.scale = roi_out.scale != 1 through the C-ABI and
compared bit for bit with the oracle (and with the reference's own code where oracle/_ref is built).

An export below full size runs the RGBA modules at a scale below 1, one with upscaling above 1.  The scales are those of S:
0.37 and 0.81 (the generated pipes' finalscale factors), 0.5, 1.5, 2.0 and 2.6 (past the clamp at 2 of non-local means).  Every
case also holds its output against the oracle's output at scale 1 on the same input: a kernel that ignored the scale would
agree with that one.  Where the reference itself clamps the scale (denoise (profiled) takes min(scale, 1), non-local means
min(scale, 2)) the clamped scales must give the SAME words as the clamp's -- stated case by case below.

dt_hip_test_nlm_last() (ansel_amd/lib.py test_nlm_last()) reports which body a non-local-means launch took.  What it reported
on gfx950 for denoise (non-local means), chunk = slice_width x slice_height of the frame, P = ceil(radius s), K = ceil(7 s),
offsets (2 K + 1)^2, reach P + 1 + (int)(s K), s = min(scale, 2):

# (width, height) chunk    scale  radius -> body       tight deep  P  offsets reach  border/chunks
# (260, 192)      72 x 64  0.37   1, 2   -> v2         1     1     1    49     3     10 / 12
#                          0.37   3      -> v2         1     1     2    49     4     10 / 12
#                          0.5    1, 2   -> v2         1     1     1    81     4     10 / 12
#                          0.5    3      -> v2         1     0     2    81     5     10 / 12
#                          0.81   1      -> v2         1     0     1   169     6     10 / 12
#                          0.81   2      -> v2         1     0     2   169     7     10 / 12
#                          0.81   3      -> v2         0     0     3   169     8     10 / 12
#                          1.5    1 2 3  -> global     0     0   2 3 5 529  19 20 22   0 / 12
#                          2, 2.6 1 2 3  -> global     0     0   2 4 6 841  31 33 35   0 / 12
# (260, 207)      72 x 69  as (260, 192) with deep 0 throughout (69 rows: two tables)
# (150, 131)      64 x 66  0.37 .. 0.81  -> v2         1     0     as above           6 / 6 (every chunk on the ring)
#                          1.5 .. 2.6    -> global
# (73, 61)        64 x 61  0.37 .. 0.81  -> v2         1     1 (0 at 0.81, radius 3)  2 / 2
#                          1.5    1      -> staged     0     0     2   529    19      0 / 2
#                          1.5    2, 3   -> global;  2, 2.6 -> global
# (73, 61)        64 x 61  0.81   4      -> pipelined  1     0     4   169     9      0 / 2
#
# The last line is not one of the frames x radii the others are drawn from: the second version takes every pipelined launch
# whose patch radius is 1 .. 3, so the pipelined body alone needs P = 4 with a reach of at most 12 -- radius 4 at 0.81, on the
# smallest of the frames.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import checkers as ck
import edge_cases as ec
import hipcheck as hc
import pipe_cases as pc
from ansel_amd import abi, lib, params, pipe, synth
from test_gpu_diffuse_three_float import FLOAT4, FLOAT4_ONLY, THREE
from test_gpu_diffuse_three_float import _run as _diffuse_with_probe

pytestmark = pytest.mark.gpu

S = (0.37, 0.5, 0.81, 1.5, 2.0, 2.6)


def _piece(w, h, s, **kw):
    return abi.Piece.make(w, h, roi_in=abi.Roi.make(0, 0, w, h, s), roi_out=abi.Roi.make(0, 0, w, h, s), **kw)


def _oracle(op, piece, d, img, pre=None):
    want = np.zeros_like(img) if pre is None else pre.copy()
    assert ck.call(ck.oracle(), "oracle_" + op, piece, d, img, want) == 0, op
    return want


def _same_words(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))


def _check(op, piece, d, img, got=None, exact_ref=True, pre=None):
    """device == oracle, tolerance 0; == the reference's own code too where it is built and is a function of its input"""
    if got is None:
        got = hc.run_hip("dt_hip_iop_%s_process" % op, piece, d, img, img.shape, pre_fill=pre)
    want = _oracle(op, piece, d, img, pre)
    diff = ck.ulp_diff(got, want)
    assert int((diff > 0).sum()) == 0, "%s: %d values differ, max %d ulp" % (op, int((diff > 0).sum()), int(diff.max()))
    ref = ck.ref()
    if ref is not None and exact_ref:
        r = np.zeros_like(img) if pre is None else pre.copy()
        assert ck.call(ref, "ref_" + op, piece, d, img, r) == 0
        assert int((ck.ulp_diff(got, r) > 0).sum()) == 0, op + " (vs reference)"
    return got


@pytest.fixture
def dispatch():
    """dt_hip_test_dispatch(): a fallback kernel on a frame the primary kernel takes; cleared behind the test"""
    keys = []

    def force(key, value=1):
        lib.test_dispatch(key, value)
        keys.append(key)
    yield force
    for k in keys:
        lib.test_dispatch(k, 0)


# ---- denoise (non-local means) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lab_image(w, h, seed=17):
    rng = np.random.default_rng(seed)
    rgb = synth.rgba_image(w, h, seed=seed, lo=0.0, hi=1.0)
    lab = np.zeros((h, w, 4), np.float32)
    lab[..., 0] = 100.0 * rgb[..., 1] + rng.normal(0, 1.5, (h, w))
    lab[..., 1] = 80.0 * (rgb[..., 0] - rgb[..., 1]) + rng.normal(0, 2.0, (h, w))
    lab[..., 2] = 80.0 * (rgb[..., 1] - rgb[..., 2]) + rng.normal(0, 2.0, (h, w))
    lab[::7, ::5, 0] = -3.0
    lab[3::11, 2::9, 0] = 140.0
    lab[..., 3] = 0.25
    lab = np.ascontiguousarray(lab.astype(np.float32))
    lab.setflags(write=False)
    return lab


NLM_FRAMES = ((260, 192), (260, 207), (150, 131), (73, 61))
NLM_CASES = [(w, h, r, s) for (w, h) in NLM_FRAMES for r in (1.0, 2.0, 3.0) for s in S] + [(73, 61, 4.0, 0.81)]


def _nlm_data(radius):
    return abi.NlmeansData(radius, 50.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def _nlm_at_scale_one(w, h, radius):
    return _oracle("nlmeans", abi.Piece.make(w, h), _nlm_data(radius), _lab_image(w, h))


@pytest.mark.parametrize("w,h,radius,scale", NLM_CASES)
def test_nlmeans(w, h, radius, scale, dispatch):
    img = _lab_image(w, h)
    piece, d = _piece(w, h, scale), _nlm_data(radius)
    got = _check("nlmeans", piece, d, img)
    last = lib.test_nlm_last()
    assert (last["radius"], last["npatch"], last["reach"]) == pc.nlmeans_figures(radius, scale), last
    assert last["body"] not in ("tall", "v4", "v3"), last  # the offsets of a scaled grid are not a regular grid
    dispatch("nlm_v2")
    again = hc.run_hip("dt_hip_iop_nlmeans_process", piece, d, img, img.shape)
    assert _same_words(again, got)
    assert not _same_words(got, _nlm_at_scale_one(w, h, radius))
    if scale == 2.6:  # min(scale, 2)
        assert _same_words(got, _oracle("nlmeans", _piece(w, h, 2.0), d, img))


def test_nlmeans_bodies_taken_at_a_scale():
    """over the cases of test_nlmeans: the second version tight and deep, loose or shallow, the pipelined, the staged and the
    global body, and a launch with interior chunks -- each at a scale != 1 (launches only: test_nlmeans compares them)"""
    seen = []
    for w, h, radius, scale in NLM_CASES:
        img = _lab_image(w, h)
        hc.run_hip("dt_hip_iop_nlmeans_process", _piece(w, h, scale), _nlm_data(radius), img, img.shape)
        last = lib.test_nlm_last()
        seen.append(last)
        print("nlm_last (%d, %d) scale %g radius %g -> %s" % (w, h, scale, radius, last))
    v2 = [x for x in seen if x["body"] == "v2"]
    assert any(x["tight"] and x["deep"] for x in v2)
    assert any(not x["tight"] or not x["deep"] for x in v2)
    assert any(not x["tight"] for x in v2) and any(not x["deep"] for x in v2)
    assert {x["body"] for x in seen} == {"v2", "pipelined", "staged", "global"}, {x["body"] for x in seen}
    assert any(x["nchunks"] > x["n_border"] > 0 for x in v2)
    assert any(x["nchunks"] == x["n_border"] for x in v2)


# ---- denoise (profiled), non-local-means mode -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noisy(w, h, seed):
    rng = np.random.default_rng(seed)
    img = synth.rgba_image(w, h, seed=seed, lo=0.0, hi=0.9)
    img[..., :3] += rng.normal(0.0, 0.01, size=(h, w, 3)).astype(np.float32) * np.sqrt(np.maximum(img[..., :3], 0.01))
    img = np.ascontiguousarray(img.astype(np.float32))
    img.setflags(write=False)
    return img


DN_NLM = (dict(), dict(radius=2, nbhood=5, scattering=0.6, central_pixel_weight=0.5))


@functools.lru_cache(maxsize=None)
def _dn_nlm_at_scale_one(w, h, k):
    d = params.denoiseprofile(mode=abi.DT_HIP_DENOISEPROFILE_NLMEANS, **DN_NLM[k])
    return _oracle("denoiseprofile", abi.Piece.make(w, h, processed_maximum=synth.WB_COEFFS), d, _noisy(w, h, 53))


@pytest.mark.parametrize("scale", S)
@pytest.mark.parametrize("w,h", [(260, 192), (170, 150)])
@pytest.mark.parametrize("k", range(len(DN_NLM)))
def test_denoiseprofile_nlmeans(k, w, h, scale, dispatch):
    img = _noisy(w, h, 53)
    d = params.denoiseprofile(mode=abi.DT_HIP_DENOISEPROFILE_NLMEANS, **DN_NLM[k])
    piece = _piece(w, h, scale, processed_maximum=synth.WB_COEFFS)
    got = _check("denoiseprofile", piece, d, img)
    last = lib.test_nlm_last()
    P, K, reach, scattering = pc.dn_nlmeans_figures(d, scale)
    assert (last["radius"], last["npatch"], last["reach"]) == (P, (2 * K + 1) ** 2, reach), (last, P, K, reach)
    if scale < 1.0 and k == 0:
        assert scattering > 0.0  # derived from the scale: nonzero although the user's is 0 (the offsets keep the user's reach)
    dispatch("nlm_v2")
    again = hc.run_hip("dt_hip_iop_denoiseprofile_process", piece, d, img, img.shape)
    assert _same_words(again, got)
    # denoiseprofile.c:1604 takes min(scale, 1): above 1 the module IS the scale-1 module, below it is not
    assert _same_words(got, _dn_nlm_at_scale_one(w, h, k)) == (scale > 1.0)


# ---- denoise (profiled), wavelets ---------------------------------------------------------------------------------------------
DN_WAVELETS = (dict(), dict(color_mode=abi.DT_HIP_DENOISEPROFILE_RGB), dict(use_new_vst=False), dict(use_new_vst=False, fix=False),
               dict(color_mode=abi.DT_HIP_DENOISEPROFILE_RGB, wb_adaptive=False, strength=1.7, shadows=0.6, bias=-3.0),
               dict(wb=(0.0, 0.0, 0.0, 0.0), strength=0.4), dict(force=[[0.5, 0.6, 0.7, 0.4, 0.3, 0.8, 0.2]] * 6))


def _dn_bands(piece, d):
    f = ck.oracle().oracle_denoiseprofile_bands
    f.restype = C.c_int
    return f(C.byref(piece), C.byref(d))


@functools.lru_cache(maxsize=None)
def _dn_wavelets_at_scale_one(w, h, k):
    d = params.denoiseprofile(**DN_WAVELETS[k])
    return _oracle("denoiseprofile", abi.Piece.make(w, h, processed_maximum=synth.WB_COEFFS), d, _noisy(w, h, 40 + k))


@pytest.mark.parametrize("scale", (0.37, 0.5, 0.81))
@pytest.mark.parametrize("w,h", [(200, 150), (503, 397)])
@pytest.mark.parametrize("k", range(len(DN_WAVELETS)))
def test_denoiseprofile_wavelets(k, w, h, scale):
    """the band count and p[i] = shadows + 0.1 logf(in_scale / wb), the gain and the bias follow the scale (setup())"""
    img = _noisy(w, h, 40 + k)
    d = params.denoiseprofile(**DN_WAVELETS[k])
    piece = _piece(w, h, scale, processed_maximum=synth.WB_COEFFS)
    # (the reference's band statistics are an OpenMP float reduction: test_gpu_denoiseprofile.py bounds that comparison)
    got = _check("denoiseprofile", piece, d, img, exact_ref=False)
    assert not _same_words(got, _dn_wavelets_at_scale_one(w, h, k))
    bands, one = _dn_bands(piece, d), _dn_bands(abi.Piece.make(w, h, processed_maximum=synth.WB_COEFFS), d)
    assert 1 <= bands <= one
    if scale == 0.37:  # log2 of the support grows by log2(1 / 0.37) = 1.43: at least one band fewer on either frame
        assert bands < one, (bands, one)
    t = abi.Tiling()
    lib.load().dt_hip_iop_denoiseprofile_tiling(C.byref(piece), C.byref(d), C.byref(t))
    assert t.overlap == 1 << bands


# ---- diffuse or sharpen -----------------------------------------------------------------------------------------------------------
# the presets of tests/test_gpu_diffuse.py on those of its frames that stay below 120 kpixels; alpha: the fourth channel's plane
DIFFUSE = (("default", {}, (333, 217), "blank"),
           ("default", dict(sharpness=0.5, radius=16, first=0.3, third=-0.2), (333, 217), "dense"),
           ("lens_deblur_soft", dict(iterations=4), (257, 191), "blank"),
           ("lens_deblur_soft", dict(iterations=2, anisotropy_first=-2.0, anisotropy_second=1.5, anisotropy_fourth=-3.0,
                                     variance_threshold=-0.5, regularization=2.5), (417, 283), "blank"),
           ("fast_local_contrast", {}, (333, 217), "blank"),
           ("fast_local_contrast", dict(radius=100, radius_center=40), (255, 33), "dense"),
           ("lens_deblur_soft", dict(iterations=2), (37, 29), "blank"),
           ("default", dict(radius=16), (9, 70), "blank"))
DIFFUSE_CASES = [(k, s, i) for k in range(len(DIFFUSE)) for s in (0.37, 0.5, 2.0) for i in (1.0, 1.7)]


@functools.lru_cache(maxsize=None)
def _diffuse_image(k):
    w, h = DIFFUSE[k][2]
    img = synth.rgba_image(w, h, seed=6, lo=-0.02, hi=1.5)
    if DIFFUSE[k][3] == "dense":
        rng = np.random.default_rng(h * 7 + w)
        img[..., 3] = rng.random((h, w), dtype=np.float32) * np.float32(1.3) - np.float32(0.1)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _diffuse_at_scale_one(k):
    preset, over, (w, h), _ = DIFFUSE[k]
    return _oracle("diffuse", abi.Piece.make(w, h), params.diffuse(preset, **over), _diffuse_image(k))


def _diffuse_scales(k, scale, iscale):
    preset, over, (w, h), _ = DIFFUSE[k]
    f = ck.oracle().oracle_diffuse_scales
    f.restype = C.c_int
    return f(C.byref(_piece(w, h, scale)), C.byref(params.diffuse(preset, iscale=iscale, **over)))


_DIFFUSE_SEQUENCES = {}


@pytest.mark.parametrize("k,scale,iscale", DIFFUSE_CASES)
def test_diffuse(k, scale, iscale):
    """zoom = iscale / roi_in.scale enters the scale count, the low-pass chain and the per-band radii"""
    preset, over, (w, h), alpha = DIFFUSE[k]
    img = _diffuse_image(k)
    piece, d = _piece(w, h, scale), params.diffuse(preset, iscale=iscale, **over)
    got, seq = _diffuse_with_probe(piece, d, img)
    _check("diffuse", piece, d, img, got=got)
    _DIFFUSE_SEQUENCES[(k, scale, iscale)] = seq
    assert seq in (THREE, FLOAT4, FLOAT4_ONLY), hex(seq)
    assert seq != THREE or alpha == "blank"
    # (the module's defaults have four zero speeds and no sharpening: the PDE adds nothing and the bands sum back to the input, up
    # to the rounding of that sum -- the same words as at scale 1 in ten of the twelve cases with them, 47 words up to 8 ulp off
    # in the two that run three scales instead of five.  Nothing of the scale is left to see there: those cases are held to the
    # oracle at their own scale, above, and to nothing else)
    if any((d.first, d.second, d.third, d.fourth, d.sharpness)):
        assert not _same_words(got, _diffuse_at_scale_one(k))
    t = abi.Tiling()
    lib.load().dt_hip_iop_diffuse_tiling(C.byref(piece), C.byref(d), C.byref(t))
    assert t.overlap == 1 << _diffuse_scales(k, scale, iscale)


def test_diffuse_cases_move_the_scale_count_both_ways_and_take_both_sequences():
    fewer = more = 0
    for k, scale, iscale in DIFFUSE_CASES:
        n, one = _diffuse_scales(k, scale, iscale), _diffuse_scales(k, 1.0, 1.0)
        fewer += n < one
        more += n > one
    assert fewer and more, (fewer, more)
    for k, scale, iscale in DIFFUSE_CASES:  # (run alone: the sequences come from the launches themselves)
        if (k, scale, iscale) not in _DIFFUSE_SEQUENCES:
            preset, over, (w, h), _ = DIFFUSE[k]
            _DIFFUSE_SEQUENCES[(k, scale, iscale)] = _diffuse_with_probe(_piece(w, h, scale), params.diffuse(preset, iscale=iscale, **over),
                                                                        _diffuse_image(k))[1]
    seqs = set(_DIFFUSE_SEQUENCES.values())
    assert THREE in seqs and (FLOAT4 in seqs or FLOAT4_ONLY in seqs), seqs


# ---- local contrast -------------------------------------------------------------------------------------------------------------
def _bilat_grid(w, h, ss, scale=1.0, iscale=1.0):
    """(entries along x, along y) of dt_bilateral_grid_size(), bilateral.c:50-74, as the oracle (pinned to the reference) sizes it"""
    dims, sig = (C.c_int * 3)(), (C.c_float * 2)()
    ck.oracle().oracle_bilat_grid(C.byref(_piece(w, h, scale)), C.byref(abi.BilatData.bilateral(ss, 25.0, 0.33, iscale=iscale)), dims, sig)
    return dims[0], dims[1]


@functools.lru_cache(maxsize=None)
def _bilat_at_scale_one(w, h, ss):
    return _oracle("bilat", abi.Piece.make(w, h), abi.BilatData.bilateral(ss, 25.0, 0.33), _lab_image(w, h, 29))


def _bilat_refused(piece, d, img):
    """a grid line shorter than the four entries blur_line() touches: refused on both sides (as edge_cases at scale 1)"""
    out = np.zeros_like(img)
    assert ck.call(ck.oracle(), "oracle_bilat", piece, d, img, out) != 0
    l = hc.hip()
    din, dout = lib.DeviceBuffer.from_numpy(0, img), lib.DeviceBuffer.from_numpy(0, out)
    assert l.dt_hip_iop_bilat_process(0, C.byref(piece), C.byref(d), din.ptr, dout.ptr) == abi.DT_HIP_INVALID_ARG
    assert l.dt_hip_finish(0) == 1
    din.release()
    dout.release()


@pytest.mark.parametrize("iscale", (1.0, 1.7))
@pytest.mark.parametrize("scale", (0.5, 2.0))
@pytest.mark.parametrize("ss", (8.0, 50.0))
def test_bilat_bilateral(ss, scale, iscale):
    """sigma_s / (iscale / roi_in.scale) sets the grid (bilat.c:339)"""
    w, h = 300, 200
    img = _lab_image(w, h, 29)
    d = abi.BilatData.bilateral(ss, 25.0, 0.33, iscale=iscale)
    piece = _piece(w, h, scale)
    if min(_bilat_grid(w, h, ss, scale, iscale)) < 4:
        return _bilat_refused(piece, d, img)
    # (the reference's splat sums per OpenMP slice: test_gpu_bilat.py bounds that comparison)
    got = _check("bilat", piece, d, img, exact_ref=False)
    assert np.array_equal(got[..., 1:], img[..., 1:])
    assert not _same_words(got, _bilat_at_scale_one(w, h, ss))


def test_bilat_bilateral_with_the_blur_split():
    """the blur's x-pass in a launch of its own (the "bilat_blur_split" test hook) on a scaled grid"""
    w, h = 300, 200
    img = _lab_image(w, h, 29)
    d = abi.BilatData.bilateral(8.0, 25.0, 0.33, iscale=1.7)
    lib.test_dispatch("bilat_blur_split", 1)
    try:
        got = _check("bilat", _piece(w, h, 0.5), d, img, exact_ref=False)
    finally:
        lib.test_dispatch("bilat_blur_split", 0)
    assert not _same_words(got, _bilat_at_scale_one(w, h, 8.0))


def test_bilat_grid_that_only_the_scale_makes_too_short_is_refused():
    """123 x 457, sigma_s 50: four entries along x at scale 1, three at scale 2 (sigma 100)"""
    w, h = 123, 457
    assert min(_bilat_grid(w, h, 50.0)) == 4 and min(_bilat_grid(w, h, 50.0, 2.0)) == 3
    img = _lab_image(w, h, 29)
    d = abi.BilatData.bilateral(50.0, 25.0, 0.33)
    _check("bilat", abi.Piece.make(w, h), d, img, exact_ref=False)
    _bilat_refused(_piece(w, h, 2.0), d, img)


def test_bilat_cases_take_grids_of_several_sizes():
    grids = {_bilat_grid(300, 200, ss, s, i) for ss in (8.0, 50.0) for s in (0.5, 2.0) for i in (1.0, 1.7)}
    ones = {_bilat_grid(300, 200, ss) for ss in (8.0, 50.0)}
    assert len(grids) >= 6 and not grids & ones, (grids, ones)


def test_local_laplacian_does_not_read_the_scale():
    w, h = 300, 200
    img = _lab_image(w, h, 33)
    d = abi.BilatData.local_laplacian()
    pre = np.full(img.shape, -5.0, np.float32)
    got = _check("bilat", _piece(w, h, 0.5), d, img, pre=pre)
    assert _same_words(got, _oracle("bilat", abi.Piece.make(w, h), d, img, pre))


# ---- rawprepare: csx / csy = round(x * scale), stated in pointwise.hip and again in pipe_fused.hip ---------------------------------
RAW_W, RAW_H, RAW_MX, RAW_MY = 132, 70, 16, 6  # output, and the margin of the input around it: both widths multiples of 4
# (8, 2): round(8 s) is 4 at 0.5 and 12 at 1.5, multiples of 4 -- the crops the fused CFA group takes; (1, 1) and (3, 2) give
# 1 2 / 2 5 columns: never fused, and the CFA phase of column 1 turns into that of column 2 at either scale
RAW_CROPS = ((1, 1), (3, 2), (8, 2))


def _raw_case(crop, scale, u16):
    cx, cy = crop
    iw, ih = RAW_W + RAW_MX, RAW_H + RAW_MY
    cfa = synth.bayer_mosaic(iw, ih, seed=3)
    piece = abi.Piece.make(RAW_W, RAW_H, filters=synth.FILTERS_RGGB, channels=1,
                           datatype=abi.DT_HIP_TYPE_UINT16 if u16 else abi.DT_HIP_TYPE_FLOAT,
                           roi_in=abi.Roi.make(0, 0, iw, ih, scale), roi_out=abi.Roi.make(0, 0, RAW_W, RAW_H, scale))
    d = abi.RawprepareData(cx, cy, RAW_MX - cx, RAW_MY - cy, abi.f4(512, 510, 514, 512),
                           abi.f4(*[synth.WHITE - 512, synth.WHITE - 510, synth.WHITE - 514, synth.WHITE - 512]))
    return piece, d, (cfa if u16 else cfa.astype(np.float32))


def _raw_shift(crop, scale):
    return tuple(int(math.floor(abs(v * scale) + 0.5)) for v in crop)  # roundf(): halves away from zero


@pytest.mark.parametrize("u16", (True, False), ids=("u16", "f32"))
@pytest.mark.parametrize("scale", (0.5, 1.5))
@pytest.mark.parametrize("crop", RAW_CROPS)
def test_rawprepare(crop, scale, u16):
    piece, d, cfa = _raw_case(crop, scale, u16)
    sx, sy = _raw_shift(crop, scale)
    assert sx <= RAW_MX and sy <= RAW_MY  # the shifted window stays inside the input
    got = hc.run_hip("dt_hip_iop_rawprepare_process", piece, d, cfa, (RAW_H, RAW_W))
    for which in hc.checkers_available():
        hc.assert_bit_exact(got, hc.run_cpu(which, "rawprepare", piece, d, cfa, (RAW_H, RAW_W)), "rawprepare vs " + which)
    one = abi.Piece.from_buffer_copy(piece)
    one.roi_in.scale = one.roi_out.scale = 1.0
    # (1, 1) at 0.5 rounds to (1, 1): the scale-1 window, and the one case whose words are the scale-1 words
    assert _same_words(got, hc.run_cpu("oracle", "rawprepare", one, d, cfa, (RAW_H, RAW_W))) == (_raw_shift(crop, scale) == crop)


def test_rawprepare_crops_change_the_cfa_phase():
    assert any((_raw_shift(c, s)[0] - c[0]) % 2 for c in RAW_CROPS for s in (0.5, 1.5))
    assert any((_raw_shift(c, s)[1] - c[1]) % 2 for c in RAW_CROPS for s in (0.5, 1.5))
    assert {_raw_shift(c, s)[0] % 4 == 0 for c in RAW_CROPS for s in (0.5, 1.5)} == {True, False}


@pytest.mark.parametrize("u16", (True, False), ids=("u16", "f32"))
@pytest.mark.parametrize("scale", (0.5, 1.5))
@pytest.mark.parametrize("crop", RAW_CROPS)
def test_rawprepare_inside_raw_chain(crop, scale, u16):
    """rawprepare + temperature + highlights through the executor: one launch (raw_chain) where round(x * scale), the two
    widths are multiples of 4, three otherwise -- and the oracle's words either way, fusion on and off"""
    hc.hip()
    piece, d, cfa = _raw_case(crop, scale, u16)
    one = abi.Piece.make(RAW_W, RAW_H, filters=synth.FILTERS_RGGB, channels=1, processed_maximum=synth.WB_COEFFS,
                         roi_in=abi.Roi.make(0, 0, RAW_W, RAW_H, scale), roi_out=abi.Roi.make(0, 0, RAW_W, RAW_H, scale))
    nodes = [pipe.Node("rawprepare", d, piece), pipe.Node("temperature", abi.TemperatureData(abi.f4(*synth.WB_COEFFS)), one),
             pipe.Node("highlights", abi.HighlightsData(abi.DT_HIP_HIGHLIGHTS_CLIP, 1.0), one)]
    want = pc.oracle_chain(nodes, cfa)
    fused_by_rule = _raw_shift(crop, scale)[0] % 4 == 0
    assert [g[0] for g in pc.plan_groups(nodes)] == (["raw"] if fused_by_rule else ["single"] * 3)
    base = pc.allocated()
    off, g0 = pc.device_pipe(nodes, cfa, fusion=False)
    on, g1 = pc.device_pipe(nodes, cfa, fusion=True)
    assert (g0, g1) == (3, 1 if fused_by_rule else 3)
    assert pc.allocated() == base
    assert pc.count_differing(off, want) == 0 and pc.count_differing(on, want) == 0
    tags = pc.launch_tags(nodes, cfa)
    assert ("raw_chain" in tags) == fused_by_rule, tags


# ---- degenerate frames at scale 0.5 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def few_oracle_threads():
    """the oracle's OpenMP loops over a handful of rows cost seconds per call on a host of many threads"""
    omp = C.CDLL("libgomp.so.1")
    omp.omp_get_max_threads.restype = C.c_int
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(4)
    yield
    omp.omp_set_num_threads(before)


@pytest.mark.parametrize("size", ec.SIZES, ids=["%dx%d" % s for s in ec.SIZES])
@pytest.mark.parametrize("module", ec.SCALE_READERS)
def test_tiny_frames(module, size, few_oracle_threads):
    w, h = size
    op, piece, data, inp, shape, pre = ec.case(module, w, h, scale=0.5)
    fn = "dt_hip_iop_%s_process" % op
    if ec.undefined_in_reference(module, w, h, scale=0.5):
        l = hc.hip()
        din, dout = lib.DeviceBuffer.from_numpy(0, inp), lib.DeviceBuffer.from_numpy(0, np.zeros(shape, np.float32))
        assert getattr(l, fn)(0, C.byref(piece), C.byref(data), din.ptr, dout.ptr) == abi.DT_HIP_INVALID_ARG
        assert l.dt_hip_finish(0) == 1
        din.release()
        dout.release()
        return
    want = np.zeros(shape, np.float32)
    assert ck.call(ck.oracle(), "oracle_" + op, piece, data, np.ascontiguousarray(inp), want) == 0
    got = hc.run_hip(fn, piece, data, inp, shape)
    d = ck.ulp_diff(got, want)
    assert int((d > 0).sum()) == 0, "%s %dx%d: %d differ, max %d ulp" % (module, w, h, int((d > 0).sum()), int(d.max()))


def test_the_scale_readers_are_stencil_modules_and_keep_their_refusals():
    assert set(ec.SCALE_READERS) <= set(ec.STENCIL_MODULES)
    # a size the reference is undefined on at scale 1 stays one at 0.5, for the wavelets' band count and for the grid
    for module in ("denoiseprofile", "bilat"):
        one = [s for s in ec.SIZES if ec.undefined_in_reference(module, *s)]
        half = [s for s in ec.SIZES if ec.undefined_in_reference(module, *s, scale=0.5)]
        assert one and set(one) <= set(half), (module, one, half)
