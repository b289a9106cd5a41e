"""TEST INFRASTRUCTURE (not a test): the frames of tests/test_gpu_strip_rows.py, and which strips they give.

The strip kernels (dn_decompose_strip, bspline_decompose_strip / _strip3, diffuse_pde_strip / _strip3) split the rows of a
frame into `mult` dilation classes -- class c holds the rows c, c + mult, c + 2 mult, ... -- and every class into strips of
`strip` rows, one workgroup per 256 columns and strip.  The launch sites size their grids for the class with the most rows,

    classes = min(h, mult)    per_class = ceil(h / mult)    strips_per_class = ceil(per_class / strip)

and the kernel computes the rows of ITS class, n_cls = (h - cls + mult - 1) // mult, from which the length of each strip
follows.  Everything below is arithmetic on h, the dilation and the strip length alone: no device, no library.

The lengths the rule of hip_common.h strip_rows() picks on these frames is 4; tests force 8, 16 and 32 (FORCED) with
dt_hip_test_dispatch("strip_rows").  tests/test_strip_rule.py asserts, on the CPU, that each family of frames below holds
every kind of strip of KINDS at every forced length -- print(report()) lists them frame by frame."""

DN_RING = 6    # denoiseprofile.hip: rows of the wavelets' LDS ring
PDE_RING = 4   # diffuse.hip: rows of the PDE's ring of squared ratios
FORCED = (8, 16, 32)

# kinds of (dilation, class) at a forced strip length
PARTIAL_LAST = "more than one strip, the last one partial"
LAST_OF_ONE = "a partial last strip of exactly one row"
EMPTY_STRIP = "n_cls a multiple of the strip while per_class is not: the grid's last strip of the class is empty (k0 >= n_cls)"
SHORT_SINGLE = "a single strip shorter than the forced length"
RING_TWICE = "a strip of at least 2 * DN_RING + 1 rows: the ring turns over twice"
RING_ONCE = "a full strip of 8 rows: the ring turns over once"
KINDS = (PARTIAL_LAST, LAST_OF_ONE, EMPTY_STRIP, SHORT_SINGLE, RING_TWICE, RING_ONCE)


def required_kinds(strip):
    """the kinds a family of frames must hold at this forced length.  A strip of 8 rows cannot have 2 * DN_RING + 1 = 13:
    at 8 the ring turns over once (s0 runs 0 .. 5, 0, 1), and the full strip that does it is asked for instead"""
    return (PARTIAL_LAST, LAST_OF_ONE, EMPTY_STRIP, SHORT_SINGLE, RING_TWICE if strip >= 2 * DN_RING + 1 else RING_ONCE)


def class_rows(h, mult):
    """[n_cls] for the classes 0 .. min(h, mult) - 1 of a frame of h rows at dilation mult"""
    return [(h - cls + mult - 1) // mult for cls in range(min(h, mult))]


def strip_lengths(n_cls, per_class, strip):
    """rows of each strip the grid launches for one class; 0: a workgroup that leaves at once"""
    return [max(min(strip, n_cls - k0), 0) for k0 in range(0, ((per_class + strip - 1) // strip) * strip, strip)]


def kinds_of(h, mult, cls, strip):
    n_cls, per_class = class_rows(h, mult)[cls], (h + mult - 1) // mult
    lengths = strip_lengths(n_cls, per_class, strip)
    found = set()
    if n_cls > strip and n_cls % strip:
        found.add(PARTIAL_LAST)
        if n_cls % strip == 1:
            found.add(LAST_OF_ONE)
    if n_cls % strip == 0 and per_class % strip:
        assert lengths[-1] == 0
        found.add(EMPTY_STRIP)
    if n_cls < strip:
        assert lengths == [n_cls]
        found.add(SHORT_SINGLE)
    if max(lengths) >= 2 * DN_RING + 1:
        found.add(RING_TWICE)
    if strip == 8 and max(lengths) == 8:
        found.add(RING_ONCE)
    return found


def strips_of(h, dilations, strip):
    """[(dilation, class, n_cls, [rows of each strip], kinds)] of a frame of h rows"""
    out = []
    for mult in dilations:
        per_class = (h + mult - 1) // mult
        for cls, n_cls in enumerate(class_rows(h, mult)):
            out.append((mult, cls, n_cls, strip_lengths(n_cls, per_class, strip), kinds_of(h, mult, cls, strip)))
    return out


def kinds_in(heights_and_dilations, strip):
    """the kinds a family of (h, dilations) holds at a forced length"""
    found = set()
    for h, dilations in heights_and_dilations:
        for _, _, _, _, kinds in strips_of(h, dilations, strip):
            found |= kinds
    return found


# ---- denoise (profiled), wavelets ------------------------------------------------------------------------------------
# (width, height, wavelet bands): the bands follow from the frame's longer side (denoiseprofile.c:1306-1322; at region scale 1
# dt_hip_iop_denoiseprofile_tiling() reports 1 << bands as its overlap, which tests/test_strip_rule.py holds these against),
# band k runs at dilation 1 << k.
#   520 x 131: three column segments, the last one 8 columns wide; dilation 1: four strips of 32 and one of 3; dilation 4:
#              classes of 33, 33, 33 and 32 rows -- a last strip of one row, and an empty one; dilation 32: classes of 5 and 4
#   300 x 200: two segments (44 columns in the second); two row bands of 100 rows each hold the coarsest halo (32 rows);
#              dilation 8: classes of 25 rows -- strips of 16 + 9 and 8 + 8 + 8 + 1
WAVELET_FRAMES = ((520, 131, 6), (300, 200, 5))
WAVELET_BAND_FRAME = (300, 200, 5)  # ... and the one the two-band test cuts


def wavelet_dilations(bands):
    return tuple(1 << k for k in range(bands))


def wavelet_family():
    return [(h, wavelet_dilations(bands)) for _, h, bands in WAVELET_FRAMES]


# ---- diffuse or sharpen ------------------------------------------------------------------------------------------------
# (preset, overrides, (width, height), scales): scale s runs the analysis at dilation 1 << s (any dilation) and the PDE on
# strips up to dilation 128 (PDE_SHARED_MULT); the scales follow from the radii alone (oracle_diffuse_scales(), held against
# in tests/test_strip_rule.py).  At the dilations 1 .. 16, which the three-float sequence and the LDS-DMA form of the PDE run,
# the frames of test_gpu_diffuse.CASES[:6] (217, 401, 300, 283, 500 and 160 rows) hold no class shorter than 8 rows, no class
# of a multiple of 16 or 32 rows beside a longer one, and no last strip of one row at 32: these two do.
#   259 x 131, lens_deblur_soft (dilations 1 .. 16): dilation 4: 33 / 32 rows; dilation 16: 9 / 8 rows
#   300 x 97,  fast_local_contrast (dilations 1 .. 512): dilation 2: 49 / 48; dilation 16: 7 / 6; above 64 one row a class
DIFFUSE_FRAMES = (
    ("lens_deblur_soft", dict(iterations=2), (259, 131), 5),
    ("fast_local_contrast", dict(), (300, 97), 10),
)
PDE_SHARED_MULT = 128


def diffuse_dilations(scales, pde=False):
    return tuple(1 << s for s in range(scales) if not pde or (1 << s) <= PDE_SHARED_MULT)


def diffuse_family(pde=False, low_only=False):
    """low_only: the dilations 1 .. 16 alone (what the three-float analysis and the LDS-DMA form of the PDE take)"""
    return [(size[1], tuple(m for m in diffuse_dilations(scales, pde) if not low_only or m <= 16))
            for _, _, size, scales in DIFFUSE_FRAMES]


def report():
    lines = []
    for name, frames in (("wavelets", [(w, h, wavelet_dilations(b)) for w, h, b in WAVELET_FRAMES]),
                         ("diffuse", [(s[0], s[1], diffuse_dilations(n)) for _, _, s, n in DIFFUSE_FRAMES])):
        for w, h, dilations in frames:
            for strip in FORCED:
                lines.append("%s %d x %d, strips of %d:" % (name, w, h, strip))
                for mult, cls, n_cls, lengths, kinds in strips_of(h, dilations, strip):
                    if kinds:
                        lines.append("  dilation %d class %d: %d rows in strips of %s -- %s"
                                     % (mult, cls, n_cls, lengths, "; ".join(k.split(":")[0] for k in sorted(kinds))))
    return "\n".join(lines)
