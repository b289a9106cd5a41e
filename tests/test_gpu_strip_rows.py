"""-m gpu: the strip kernels at the strip lengths real frames take.

hip_common.h strip_rows() gives the frames a test can afford 4 rows a strip and every real frame 32 (tests/test_strip_rule.py).
Here the length is forced -- dt_hip_test_dispatch("strip_rows", 8 | 16 | 32) -- on small frames, and every result is held
against the oracle on the same input, bit for bit: rings that turn over more than once, a few long strips a class with a
long partial last one, the grid's empty strip, and the state a lane carries from row to row (the wavelets' up1 / up2 /
up2_next, the PDE's fetch-ahead, the double buffer of the partial sums) over 8 to 32 rows instead of 3.

Which (dilation, class) strips each frame contributes: tests/strip_cases.py (print(strip_cases.report())).  The parameter
lists are those of the modules' own tests (test_gpu_denoiseprofile.py, test_gpu_diffuse.py, pipe_cases.py)."""
import functools

import numpy as np
import pytest

import checkers as ck
import edge_cases as ec
import hipcheck as hc
import pipe_cases as pc
import strip_cases as sc
import test_gpu_denoiseprofile as tdn
import test_gpu_diffuse as tdf
from ansel_amd import abi, params, pipe, synth

pytestmark = pytest.mark.gpu


@pytest.fixture
def dispatch():
    """dt_hip_test_dispatch(): the strip length of larger frames on a small one; cleared behind the test"""
    from ansel_amd import lib
    keys = []

    def force(key, value=1):
        lib.test_dispatch(key, value)
        keys.append(key)
    yield force
    for k in keys:
        lib.test_dispatch(k, 0)


def _differing(got, want):
    diff = ck.ulp_diff(got, want)
    return int((diff > 0).sum()), int(diff.max())


def _assert_same(got, want, what):
    n, worst = _differing(got, want)
    assert n == 0, "%s: %d values differ, max %d ulp" % (what, n, worst)


# ---- denoise (profiled), wavelets ------------------------------------------------------------------------------------
# name -> overrides of params.denoiseprofile(), taken from the module's own CASES (the comment: the kernel forms the case reaches)
WAVELETS = {
    "defaults": tdn.CASES[0][0],          # Y0U0V0: dn_decompose_strip<PRE, 1, ALPHA0, P3> at scale 0, <false, M, true, true> behind it
    "rgb": tdn.CASES[1][0],               # one four-channel sequence: <PRE, 1, false> and <false, M, false>
    "old-vst": tdn.CASES[2][0],           # the legacy transform (four channels), with the bias fix
    "old-vst-unfixed": tdn.CASES[3][0],   # ... and without
    "strength-shadows-bias": tdn.CASES[4][0],  # non-default strength / shadows / bias (RGB, no adaptive white balance)
}
assert WAVELETS["defaults"] == {} and WAVELETS["old-vst-unfixed"] == dict(use_new_vst=False, fix=False) and "bias" in WAVELETS["strength-shadows-bias"]
WAVELET_INPUTS = [(name, "noisy") for name in WAVELETS] + [("defaults", "adversarial"), ("defaults", "one-nan")]


@functools.lru_cache(maxsize=None)
def _wavelet_case(name, inp, frame):
    """(piece, data, input, the oracle's output, the reference's or None): computed once for the three strip lengths"""
    w, h, _ = sc.WAVELET_FRAMES[frame]
    d = params.denoiseprofile(**WAVELETS[name])
    piece = abi.Piece.make(w, h, processed_maximum=synth.WB_COEFFS)
    if inp == "adversarial":
        _, piece, d, img, _, _ = ec.adversarial("denoiseprofile", w, h)
    else:
        img = tdn._noisy(w, h, 70 + frame)
        if inp == "one-nan":
            img[0, w // 3, 1] = np.float32(np.nan)
            assert int((~np.isfinite(img)).sum()) == 1
    img = np.ascontiguousarray(img)
    want = np.zeros_like(img)
    assert ck.call(ck.oracle(), "oracle_denoiseprofile", piece, d, img, want) == 0
    r = None
    if ck.ref() is not None and inp == "noisy":
        r = np.zeros_like(img)
        assert ck.call(ck.ref(), "ref_denoiseprofile", piece, d, img, r) == 0
    for a in (img, want) + ((r,) if r is not None else ()):
        a.setflags(write=False)
    return piece, d, img, want, r


@pytest.mark.parametrize("strip", sc.FORCED)
@pytest.mark.parametrize("frame", range(len(sc.WAVELET_FRAMES)), ids=["%dx%d" % f[:2] for f in sc.WAVELET_FRAMES])
@pytest.mark.parametrize("name,inp", WAVELET_INPUTS, ids=["%s-%s" % c for c in WAVELET_INPUTS])
def test_wavelets_at_forced_strip_lengths(name, inp, frame, strip, dispatch):
    """dt_hip_iop_denoiseprofile_process == oracle, bit for bit, at 8, 16 and 32 rows a strip.

    defaults: the Y0U0V0 transform's two sequences -- the three-float launches (mode 1: <PRE, 1, ALPHA0, P3> at scale 0, which
    applies the transform as it fetches, then <false, 2 .. 32, true, true>), and the four-channel launches (mode 2), which leave
    at once.  rgb / old-vst / old-vst-unfixed / strength-shadows-bias: one sequence of four-channel launches (<PRE, 1, false>, <false, M, false>),
    16-byte ring entries.  adversarial: NaN, infinities, denormals and +-1e30 inside the supports, so that the three-float
    sequence raises the alpha flag and the four-channel one behind it redoes the module.  one-nan: the same through a single
    NaN word in row 0 -- the flag is raised by the strip that holds row 0 alone, and every strip of every later launch must
    see it"""
    piece, d, img, want, ref = _wavelet_case(name, inp, frame)
    dispatch("strip_rows", strip)
    got = hc.run_hip("dt_hip_iop_denoiseprofile_process", piece, d, img, img.shape)
    _assert_same(got, want, "%s, %s, %d rows a strip" % (name, inp, strip))
    if inp == "noisy":
        assert float(np.abs(got[..., :3] - img[..., :3]).max()) > 1e-4  # the module did something
    if ref is not None:
        # (the reference's band statistics are an OpenMP float reduction: bounded as in test_gpu_denoiseprofile.py)
        err = np.abs(got[..., :3] - ref[..., :3]) / np.maximum(np.abs(ref[..., :3]), 1e-3)
        assert float(err.max()) < 5e-5, float(err.max())


@pytest.mark.parametrize("strip", sc.FORCED)
def test_wavelets_in_two_row_bands_at_forced_strip_lengths(strip, dispatch):
    """the band job (denoiseprofile_band_step()): every scale as a four-channel launch <false, M, false> on the band's own
    rows, its input a buffer with the neighbour's halo rows above or below them (in_row0 / in_rows).  Two bands of 100 rows
    through the band engine == the unsplit executor run == the oracle"""
    w, h, _ = sc.WAVELET_BAND_FRAME
    piece = abi.Piece.make(w, h, channels=4, processed_maximum=synth.WB_COEFFS)
    nodes = [pipe.Node("denoiseprofile", params.denoiseprofile(), piece)]
    src = tdn._noisy(w, h, 77)
    oracle = pc.oracle_chain(nodes, src)
    hc.hip()
    base = pc.allocated()
    dispatch("strip_rows", strip)
    whole, _ = pc.device_pipe(nodes, src, fusion=True)
    banded = pc.device_bands(nodes, src, 2)
    assert pc.allocated() == base
    assert pc.count_differing(whole, oracle) == 0
    assert pc.count_differing(banded, whole) == 0
    assert pc.count_differing(banded, oracle) == 0


# ---- diffuse or sharpen ------------------------------------------------------------------------------------------------
# the parameters of test_diffuse_out_of_range_operands_take_the_long_forms(), from its own mark
_EXTREME = tdf.test_diffuse_out_of_range_operands_take_the_long_forms.pytestmark[0].args[1]
assert len(_EXTREME) == 3 and _EXTREME[0][0] == "lens_deblur_soft"


def _diffuse_image(w, h, imgname, seed=6):
    img = synth.rgba_image(w, h, seed=seed, lo=-0.02, hi=1.5)
    if "-" in imgname:
        img = tdf._with_alpha(img, imgname.split("-")[1])
    return img


@functools.lru_cache(maxsize=None)
def _diffuse_case(kind, k, imgname):
    """(piece, data, input, the oracle's output, the reference's or None) of case k of one of the lists below"""
    if kind == "cases":
        preset, over, (w, h) = tdf.CASES[k]
        img = _diffuse_image(w, h, imgname)
    elif kind == "frames":
        preset, over, (w, h), _ = sc.DIFFUSE_FRAMES[k]
        img = _diffuse_image(w, h, imgname)
    elif kind == "patterns":
        # as test_diffuse_kind_patterns() builds them
        w, h = 389, 251
        preset, over = "default", dict(iterations=2, radius=12, regularization=1.5, variance_threshold=0.3, sharpness=0.1, first=-0.25,
                                       second=0.125, third=-0.125, fourth=0.0625, **tdf.PATTERNS[k][1])
        img = tdf._with_alpha(synth.rgba_image(w, h, seed=16, lo=-0.02, hi=1.5), "patches")
    elif kind == "inpaint":
        preset, over, (w, h) = tdf.INPAINT_CASES[k]
        img = synth.rgba_image(w, h, seed=8, lo=-0.02, hi=1.8)
    else:
        assert kind == "extreme", kind
        preset, over = _EXTREME[k]
        w, h = 523, 331
        img = tdf._extreme_rgba(w, h)
    img = np.ascontiguousarray(img)
    piece = abi.Piece.make(w, h)
    d = params.diffuse(preset, **over)
    want = tdf._cpu("oracle", piece, d, img)
    assert want is not None
    ref = tdf._cpu("ref", piece, d, img) if kind != "patterns" else None  # (the patterns' own test compares with the oracle alone)
    for a in (img, want) + ((ref,) if ref is not None else ()):
        a.setflags(write=False)
    return piece, d, img, want, ref


def _run_diffuse(kind, k, imgname, strip, dispatch, nan_is_nan=False):
    piece, d, img, want, ref = _diffuse_case(kind, k, imgname)
    dispatch("strip_rows", strip)
    got = hc.run_hip("dt_hip_iop_diffuse_process", piece, d, img, img.shape)
    for name, other in (("oracle", want), ("reference", ref)):
        if other is None:
            continue
        if nan_is_nan:
            same = (got.view(np.uint32) == other.view(np.uint32)) | (np.isnan(got) & np.isnan(other))
            assert same.all(), "%s: %d values differ" % (name, int((~same).sum()))
        else:
            _assert_same(got, other, "%s %d %s against the %s, %d rows a strip" % (kind, k, imgname, name, strip))
    return got, img, d


@pytest.mark.parametrize("strip", sc.FORCED)
@pytest.mark.parametrize("imgname", ["scene", "scene-dense", "scene-sparse"])
@pytest.mark.parametrize("k", range(6), ids=["%s-%dx%d" % (c[0], c[2][0], c[2][1]) for c in tdf.CASES[:6]])
def test_diffuse_cases_at_forced_strip_lengths(k, imgname, strip, dispatch):
    """the first six of test_gpu_diffuse.CASES.
    Cases 0 and 2 (five scales, the isotropic and the deblur pattern): on `scene`, whose alpha is +0, the three-float sequence --
    bspline_decompose_strip3<M> and diffuse_pde_strip3<ISOTROPIC | DEBLUR, h0_4> at dilations 1 .. 16; on scene-dense the first
    launch raises the flag and the float4 chain redoes the module with four live channels, bspline_decompose_strip<R, T> without
    an HF plane and diffuse_pde_strip<true, MD, true> by LDS-DMA; on scene-sparse (-0, one sample and one NaN in a blank alpha)
    the same, with waves that may skip a blank alpha and waves that may not in one strip.
    Case 1 (six scales): dilation 32 has no three-float kernel: the float4 chain alone, its PDE by LDS-DMA up to dilation 16 and
    through registers (diffuse_pde_strip<true, MD>) at 32.  Case 3: a pattern of kinds no kernel spells at compile time (MD -1).
    Cases 4 and 5 (ten and nine scales, dilations up to 512): no chain above dilation 128, so the stored-HF form:
    bspline_decompose_strip<8, 32> with up to 64 column groups writing both planes, diffuse_pde_strip<false, MD> up to dilation 128
    and the per-row kernel above"""
    _run_diffuse("cases", k, imgname, strip, dispatch)


@pytest.mark.parametrize("strip", sc.FORCED)
@pytest.mark.parametrize("imgname", ["scene", "scene-dense"])
@pytest.mark.parametrize("k", range(len(sc.DIFFUSE_FRAMES)), ids=["%s-%dx%d" % (c[0], c[2][0], c[2][1]) for c in sc.DIFFUSE_FRAMES])
def test_diffuse_strip_frames_at_forced_strip_lengths(k, imgname, strip, dispatch):
    """the two frames of strip_cases.DIFFUSE_FRAMES, whose classes at the dilations 1 .. 16 hold what the frames above do not
    (the empty strip, a single short strip, a last strip of one row at 32).  lens_deblur_soft, two iterations: the three-float
    sequence (scene) or the float4 chain by LDS-DMA (scene-dense), with the ping-pong between iterations.  fast_local_contrast:
    ten scales -- the float4 chain is off above dilation 128, so the stored-HF form: bspline_decompose_strip<8, 32> with up to
    64 column groups, diffuse_pde_strip<false, MD> up to dilation 128"""
    _run_diffuse("frames", k, imgname, strip, dispatch)


@pytest.mark.parametrize("strip", sc.FORCED)
@pytest.mark.parametrize("k", range(len(tdf.PATTERNS)), ids=[p[0] for p in tdf.PATTERNS])
def test_diffuse_kind_patterns_at_forced_strip_lengths(k, strip, dispatch):
    """every entry of test_gpu_diffuse.PATTERNS on its 389 x 251 frame with alpha in patches: the float4 chain, one
    diffuse_pde_strip<true, MD, true> per compile-time pattern of kinds (MD) by LDS-DMA up to dilation 16 and <true, MD> through
    registers at 32, and the run-time kernel (MD -1) for the mixed one; two iterations, six scales"""
    _run_diffuse("patterns", k, "patches", strip, dispatch)


@pytest.mark.parametrize("strip", sc.FORCED)
def test_diffuse_masked_inpainting_at_forced_strip_lengths(strip, dispatch):
    """inpaint_highlights, four iterations, threshold 1.0 on 333 x 217: the masked form -- the PDE loads the mask's byte in its
    row step, so the LDS-DMA fetch does not overlap it -- and the noise seeded by position"""
    got, img, d = _run_diffuse("inpaint", 0, "scene", strip, dispatch)
    masked = (img[..., :3] > d.threshold).any(axis=2)
    assert 0 < masked.sum() and not np.array_equal(got[masked], img[masked])


@pytest.mark.parametrize("strip", sc.FORCED)
@pytest.mark.parametrize("k", range(len(_EXTREME)))
def test_diffuse_extreme_operands_at_forced_strip_lengths(k, strip, dispatch):
    """test_gpu_diffuse._extreme_rgba() on 523 x 331 (three column spans, 11 x 32 rows less 21): magnitudes beyond 2^64, infinities,
    NaN, subnormals -- the long forms of the PDE's divisions and square roots, in the deblur, isotropic and run-time kernels"""
    _run_diffuse("extreme", k, "extreme", strip, dispatch, nan_is_nan=True)


# ---- the fused tails ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    hc.hip()
    dev, host = pc.Tables(True), pc.Tables(False)
    yield dev, host
    dev.release()


@pytest.mark.parametrize("name", ["diffuse+rgb_to_lab", "wavelets+run-cm_none"])
def test_fused_tails_at_32_rows_a_strip(tables, name, dispatch):
    """the two strip kernels' results leave through another module's code when the frame walk fuses the pair: the PDE's last pass
    stores through post_lab (diffuse + rgb_to_lab), the wavelets' synthesis runs the pointwise run behind it (dn_finish_chain).
    At 32 rows a strip: fusion on == fusion off == the oracle, as test_gpu_fused_variants.py runs them at 4, and the pool is
    back at its baseline"""
    dev, host = tables
    names = [c[0] for c in pc.fused_pair_cases(host)]
    k = names.index(name)
    _, dev_nodes, kind, pairs, groups = pc.fused_pair_cases(dev)[k]
    host_nodes = pc.fused_pair_cases(host)[k][1]
    assert pairs  # the pair fuses by rule
    src = pc.pair_frame(kind)
    oracle = pc.oracle_chain(host_nodes, src)
    base = pc.allocated()
    dispatch("strip_rows", 32)
    fused, g1 = pc.device_pipe(dev_nodes, src, fusion=True)
    unfused, g0 = pc.device_pipe(dev_nodes, src, fusion=False)
    assert pc.allocated() == base, "%s: the pool is %d bytes off its baseline" % (name, pc.allocated() - base)
    assert g0 == len(pc.kept(dev_nodes)) and g1 == groups
    for what, got in (("fusion on", fused), ("fusion off", unfused)):
        bad = pc.count_differing(got, oracle)
        assert bad == 0, "%s, %s: %d of %d words differ from the oracle" % (name, what, bad, oracle.size)
