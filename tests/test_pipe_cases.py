"""not gpu: the generator and the CPU reference of tests/pipe_cases.py, checked before a GPU sees them.

  * the conditions on the fixed seed list of tests/test_gpu_pipe_generated.py -- half of the lists eligible for row bands,
    every kind of launch group and each of the four fused pairs somewhere -- counted from the restated rules
  * a list that is band-eligible by rule is one dt_hip_plan_bands() and the halo rows of its stencil modules take
  * every reference output has a spread: a pipe that saturates to black proves nothing
  * the oracle's nodes equal the reference's own code (oracle/_ref) wherever that is a function of its input, for every
    seed and every fixed case of tests/test_gpu_fused_variants.py; runs where oracle/_ref was built
  * the pairwise set over the switches of rgb_chain covers what it says"""
import ctypes as C
import functools

import numpy as np
import pytest

import checkers as ck
import pipe_cases as pc
from ansel_amd import abi, lib, params, pipe, synth, tiled


@functools.lru_cache(maxsize=None)
def _oracle(seed):
    """(nodes, src, tags, result, the frame in front of an encoder or the result) of one seed over host memory"""
    nodes, src, tags = pc.generate(seed)
    frames = {}
    out = pc.oracle_chain(nodes, src, tap=lambda k, n, i, o, before: frames.__setitem__(k, o))
    frame = frames[len(nodes) - 2] if nodes[-1].op in pc.ENCODERS else out
    return nodes, src, tags, out, frame


def test_the_seed_list_is_fixed_and_long_enough():
    assert len(pc.SEEDS) >= 60 and len(set(pc.SEEDS)) == len(pc.SEEDS)


def test_a_seed_gives_the_same_list_over_host_and_any_other_tables():
    for seed in pc.SEEDS[:12]:
        a, sa, ta = pc.generate(seed)
        b, sb, tb = pc.generate(seed, pc.Tables(False))
        assert [n.op for n in a] == [n.op for n in b] and np.array_equal(sa.view(np.uint8), sb.view(np.uint8))
        assert ta["bands"] == tb["bands"]
        for x, y in zip(a, b):
            assert bytes(x.piece) == bytes(y.piece)
            if x.op in ("exposure", "channelmixerrgb", "filmicrgb", "diffuse", "denoiseprofile", "nlmeans", "bilat", "flip"):
                assert bytes(x.data) == bytes(y.data), x.op  # (the other data carries pointers)


def test_frames_are_awkward():
    for w, h in pc.RAW_FRAMES + pc.RGBA_FRAMES + (pc.VARIANT_FRAME,):
        assert (w * h) % 256 and w * h <= 120000, (w, h)
    assert any(w % 4 for w, _ in pc.RAW_FRAMES) and any(w % 4 for w, _ in pc.RGBA_FRAMES)
    assert any(w % 4 == 0 for w, _ in pc.RAW_FRAMES)  # the fused CFA group wants whole float4s


def test_coverage_of_the_seed_list():
    """at least half of the lists run on row bands and all in a batch; every kind of launch group, each fused pair of the
    frame walk, every start, every ending and every node of the grammar occur"""
    kinds, pairs, starts, ends, ops = set(), set(), set(), set(), set()
    bands = batch = 0
    for seed in pc.SEEDS:
        nodes, _, tags = pc.generate(seed)
        bands += bool(tags["bands"])
        batch += bool(tags["batch"])
        kinds |= {k for k, _, _ in pc.plan_groups(nodes)}
        pairs |= pc.fused_pairs(nodes)
        starts.add(tags["start"])
        ends.add(tags["end"])
        ops |= {n.op for n in nodes}
    assert 2 * bands >= len(pc.SEEDS) and 2 * batch >= len(pc.SEEDS), (bands, batch)
    assert kinds == {"single", "raw", "rgb"}, kinds
    assert pairs == {"denoiseprofile+run", "bilat+run", "diffuse+rgb_to_lab", "nlmeans>bilat"}, pairs
    assert starts == {"raw_u16", "raw_f32", "rgba_scene", "rgba_adversarial"} and ends == set(pc.ENDINGS)
    assert ops >= set(pc.CFA_OPS + pc.RUN_OPS + pc.ENCODERS) | {"demosaic", "denoiseprofile", "diffuse", "rgb_to_lab", "nlmeans",
                                                              "bilat", "lab_to_rgb", "blend", "detailmask", "flip", "finalscale",
                                                              "export_u16", "export_u8", "export_rows"}


def test_the_placement_rules_hold_in_every_list():
    for seed in pc.SEEDS:
        nodes, _, _ = pc.generate(seed)
        ops = [n.op for n in nodes]
        for k, n in enumerate(nodes):
            if n.op == "blend":
                assert k > 0 and ops[k - 1] in pc.BLENDABLE, (seed, ops)
            if n.op == "flip" and k + 1 < len(nodes):
                assert nodes[k + 1].piece.channels == n.piece.channels and ops[k + 1] != "blend", (seed, ops)
            if n.op == "export_jpeg":
                assert k + 1 == len(nodes) and ops[k - 1] == "export_u8", (seed, ops)
            if n.op == "export_png":
                assert k + 1 == len(nodes) and ops[k - 1] == ("export_u16" if n.data.bit_depth == 16 else "export_u8"), (seed, ops)
            if k + 1 < len(nodes) and n.op not in ("blend", "flip", "finalscale") and ops[k + 1] not in ("blend",):
                nxt = nodes[k + 1].piece
                assert (nxt.roi_in.width, nxt.roi_in.height) == (n.piece.roi_out.width, n.piece.roi_out.height), (seed, ops)


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_band_eligibility_by_rule_is_what_the_library_plans(seed):
    """dt_hip_plan_bands() and dt_hip_band_halo_rows() are host functions: an eligible list is planned for 2 and 3 bands and
    no band is shorter than the halo a stencil module asks of it; a demosaic or a frame without a band mode is refused"""
    nodes, _, tags = pc.generate(seed)
    w, h = nodes[0].piece.roi_out.width, nodes[0].piece.roi_out.height
    method = tiled.pipe_demosaic_method(nodes)
    l = lib.load()
    for n_bands in (2, 3):
        tile_rows = pc.band_tile_rows(w, h, method)
        if tile_rows < n_bands:
            with pytest.raises(lib.AnselHipError):
                tiled.plan_bands(w, h, n_bands, method)
            continue
        bands = tiled.plan_bands(w, h, n_bands, method)
        assert [(b.row0, b.rows) for b in bands] == pc.band_rows(w, h, method, n_bands)
        for n in nodes:
            if n.data is None or n.op == "blend" or (n.piece.roi_out.width, n.piece.roi_out.height) != (w, h):
                continue
            halo = l.dt_hip_band_halo_rows(n.op.encode(), C.byref(n.piece), C.cast(C.byref(n.data), C.c_void_p), C.sizeof(n.data))
            assert halo <= pc.stencil_halo_bound(n), (n.op, halo)
            if tags["bands"]:
                for k, b in enumerate(bands):
                    assert k == 0 or min(halo, b.row0) <= bands[k - 1].rows, (n.op, halo, k)
                    assert k + 1 == n_bands or min(halo, h - b.row0 - b.rows) <= bands[k + 1].rows, (n.op, halo, k)


def _spread(a):
    v = a.astype(np.float64)
    return float(v[np.isfinite(v)].std())


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_every_generated_pipe_gives_a_picture(seed):
    """as test_gpu_tiled.py asks of its frames (std > 100 of 65535), in the units of the frame's sample type; a file is
    judged by the frame it encodes, and must decode to it"""
    nodes, src, tags, out, frame = _oracle(seed)
    shape, dtype = pc.out_format(nodes)
    if nodes[-1].op in pc.ENCODERS:
        assert out.dtype == np.uint8 and 0 < out.size <= shape[0] - 8
    else:
        assert out.shape == shape and out.dtype == dtype
    scale = {np.dtype(np.uint16): 1.0, np.dtype(np.uint8): 255.0 / 65535.0, np.dtype(np.float32): 1.0 / 65535.0}[frame.dtype]
    assert _spread(frame) > 100.0 * scale, _spread(frame)
    if nodes[-1].op == "export_png":
        import png_ref as pr
        h, w = frame.shape[:2]
        rows = pr.unfilter(pr.inflate(out.tobytes()), w, h, 8 * frame.itemsize)
        assert np.array_equal(np.asarray(rows).reshape(h, w, 3), frame[..., :3])


def _stale_mask(n):
    """the pixels where the reference is not a function of its input: the RCD scratch columns and the
    AMaZE tile buffer; the exclusions tests/test_oracle_vs_ref.py makes, no others"""
    w, h = n.piece.roi_out.width, n.piece.roi_out.height
    m = np.zeros((h, w), np.uint8)
    method = int(n.data.demosaicing_method)
    if method == abi.DT_HIP_DEMOSAIC_RCD:
        full = np.zeros((h, w), np.uint8)
        ck.oracle().oracle_rcd_stale_mask(ck.ptr(full), w, h, C.c_uint32(synth.FILTERS_RGGB))
        m[:, w - 9:w - 6] = full[:, w - 9:w - 6]
    elif method == abi.DT_HIP_DEMOSAIC_AMAZE:
        ck.oracle().oracle_amaze_stale_mask(ck.ptr(m), w, h)
    return m


def _differing(out, exp):
    return ck.ulp_diff(out, exp) if out.dtype == np.float32 else (out != exp).astype(np.int64)


def _nodes_equal_the_reference(nodes, src, what):
    """oracle_chain(.., "oracle") against the reference's own code, with the exclusions tests/test_oracle_vs_ref.py makes and
    no others: the reference on ONE thread and the oracle's wavelets summing in that order (the wavelets' sums, the
    bilateral splat and the AMaZE tile buffer follow the thread count), the RCD / AMaZE stale words masked.

      * node by node, each reference function on the oracle's own input of the node -- a blend on the copy of its module's
        output the blend found, a detailmask with its plane compared as well -- so that a masked word of a demosaic does
        not travel into the nodes behind it;
      * and the whole chain, oracle_chain(.., "ref") == oracle_chain(.., "oracle"), every word, for the lists whose
        reference is a function of its input from end to end: those without an RCD or AMaZE demosaic."""
    r, o = ck.ref(), ck.oracle()
    threads = r.ref_get_num_threads()
    r.ref_set_num_threads(1)
    o.oracle_denoiseprofile_sum_order(1)
    try:
        def tap(k, n, inp, out, before):
            name = "develop_blend" if n.op == "blend" else n.op
            if n.op in ("flip", "export_rows") + pc.ENCODERS or not hasattr(r, "ref_" + name):
                return
            fail = "%s, node %d (%s)" % (what, k, n.op)
            if n.op in ("export_u16", "export_u8"):
                exp = np.zeros_like(out)
                getattr(r, "ref_" + n.op.replace("export_", "export_convert_"))(out.shape[1], out.shape[0], ck.ptr(inp), ck.ptr(exp))
            elif n.op == "blend":
                exp = before.copy()  # in place in the module's output, as the oracle's blend found it
                assert ck.call(r, "ref_develop_blend", n.piece, n.data, np.ascontiguousarray(inp), exp) == 0, fail
            elif n.op == "detailmask":
                # the stage also writes the raw detail mask's plane, which a blend further down reads: the reference's plane
                # must be the oracle's, and the oracle's is what stays in place
                h, w = out.shape[:2]
                plane = np.ctypeslib.as_array(C.cast(n.data.mask, C.POINTER(C.c_float)), shape=(h, w))
                mine = plane.copy()
                exp = np.zeros_like(out)
                assert ck.call(r, "ref_detailmask", n.piece, n.data, np.ascontiguousarray(inp), exp) == 0, fail
                bad = int((ck.ulp_diff(plane, mine) > 0).sum())
                plane[...] = mine
                assert bad == 0, "%s: %d words of the raw detail mask differ from the reference" % (fail, bad)
            else:
                exp = np.zeros_like(out)
                assert ck.call(r, "ref_" + name, n.piece, n.data, np.ascontiguousarray(inp), exp) == 0, fail
            d = _differing(out, exp)
            if n.op == "demosaic":
                d = d * (_stale_mask(n) == 0)[..., None]
            assert int((d > 0).sum()) == 0, "%s: %d words differ from the reference" % (fail, int((d > 0).sum()))
        mine = pc.oracle_chain(nodes, src, tap=tap)
        stale = any(n.op == "demosaic" and int(n.data.demosaicing_method) in (abi.DT_HIP_DEMOSAIC_RCD, abi.DT_HIP_DEMOSAIC_AMAZE)
                    for n in nodes)
        if not stale:
            theirs = pc.oracle_chain(nodes, src, which="ref")
            assert mine.shape == theirs.shape and mine.dtype == theirs.dtype, what
            bad = int((_differing(mine, theirs) > 0).sum())
            assert bad == 0, "%s: %d words of the whole chain differ from the reference's" % (what, bad)
    finally:
        o.oracle_denoiseprofile_sum_order(0)
        r.ref_set_num_threads(threads)


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_generated_pipe_oracle_equals_the_reference(seed, ref_lib):
    nodes, src, _ = pc.generate(seed)
    _nodes_equal_the_reference(nodes, src, "seed %d" % seed)


def test_fixed_cases_oracle_equals_the_reference(ref_lib):
    tb = pc.Tables(False)
    frames = pc.variant_frames()
    for cm in pc.CM_KINDS:
        for fm in pc.FM_KINDS:
            for name, img in frames.items():
                _nodes_equal_the_reference(pc.run_nodes_of(tb, cm, fm), img, "cm %s fm %s %s" % (cm, fm, name))
    for case in pc.pairwise_cases()[0]:
        kw = pc.pairwise_kwargs(case)
        src = pc.variant_lab_frame() if kw["pre_lab"] else frames["scene"]
        _nodes_equal_the_reference(pc.run_nodes_of(tb, **kw), src, "pairwise %r" % (case,))
    for name, nodes, kind, _, _ in pc.fused_pair_cases(tb):
        _nodes_equal_the_reference(nodes, pc.pair_frame(kind), name)


def test_fixed_cases_have_a_reference_with_a_spread():
    tb = pc.Tables(False)
    frames = pc.variant_frames()
    for cm in pc.CM_KINDS:
        for fm in pc.FM_KINDS:
            nodes = pc.run_nodes_of(tb, cm, fm)
            assert pc.plan_groups(nodes) == [("rgb", 0, len(nodes))]
            for img in frames.values():
                assert _spread(pc.oracle_chain(nodes, img)) > 100.0
    for name, nodes, kind, pairs, groups in pc.fused_pair_cases(tb):
        assert pc.fused_pairs(nodes) == pairs, (name, pc.fused_pairs(nodes))
        assert len(pc.plan_groups(nodes)) == groups, (name, pc.plan_groups(nodes))
        out = pc.oracle_chain(nodes, pc.pair_frame(kind))
        assert _spread(out) > (100.0 if out.dtype == np.uint16 else 100.0 / 65535.0), name


def test_pairwise_set_covers_every_pair_of_switch_values():
    cases, want = pc.pairwise_cases()
    got = set()
    for c in cases:
        assert pc._valid(c)
        got |= pc._pairs_of(c)
    assert got == want
    # every value of every switch occurs with every value of every other, but "rgb_to_lab" behind an export conversion
    n = [len(v) for _, v in pc.SWITCHES]
    total = sum(n[i] * n[j] for i in range(len(n)) for j in range(i + 1, len(n)))
    assert len(want) == total - 2 and len(cases) <= 80, (len(want), total, len(cases))
    tb = pc.Tables(False)
    for c in cases:
        nodes = pc.run_nodes_of(tb, **pc.pairwise_kwargs(c))
        assert pc.plan_groups(nodes) == [("rgb", 0, len(nodes))], [x.op for x in nodes]


# ---- generate() is pinned; the lists at a region scale != 1 (generate_scaled()) ------------------------------------------------
_PLAIN_DATA = ("exposure", "diffuse", "denoiseprofile", "nlmeans", "bilat", "flip", "finalscale", "rawprepare", "temperature",
               "highlights", "demosaic", "export_rows")  # data that is literals, no pointer and no fitted curve


def test_generate_gives_the_lists_it_gave_before_there_was_a_scaled_generator():
    """the 72 lists of generate(), word for word: every op, every piece, the data that is plain numbers, the frame's format and
    the tags -- one digest, taken before generate_scaled() and _Builder.scale existed"""
    import hashlib
    h = hashlib.sha256()
    for seed in pc.SEEDS:
        nodes, src, tags = pc.generate(seed)
        h.update(("%d %s %s %s %s %s %s|" % (seed, src.shape, src.dtype, tags["bands"], tags["batch"], tags["start"], tags["end"])).encode())
        for n in nodes:
            h.update(n.op.encode())
            h.update(bytes(n.piece))
            if n.op in _PLAIN_DATA:
                h.update(bytes(n.data))
    assert len(pc.SEEDS) == 72
    assert h.hexdigest() == "d2e5f74ac9e5e0c04bb51fe92bd8564a6305e2b9e0a6c0398c65eebf0a803a68"


def _scale_of(n):
    return (n.piece.roi_in.scale, n.piece.roi_out.scale)


def _is_nlm(n):
    return n.op == "nlmeans" or (n.op == "denoiseprofile" and n.data.mode in (abi.DT_HIP_DENOISEPROFILE_NLMEANS, abi.DT_HIP_DENOISEPROFILE_NLMEANS_AUTO))


def test_coverage_of_the_scaled_seed_list():
    """24 lists; both shapes; every scale of either shape; every stencil module, both modes of denoise (profiled), at a scale
    != 1; at least four lists on row bands, one of them with non-local means or diffuse at scale 2; every piece behind the
    resampler (every piece of an RGBA list) carries the list's scale on both regions"""
    assert len(pc.SCALED_SEEDS) == 24
    shapes, scales, stencils, band_lists, heavy_on_bands = set(), set(), set(), 0, 0
    for seed in pc.SCALED_SEEDS:
        nodes, src, tags = pc.generate_scaled(seed)
        s = tags["scale"]
        shapes.add(tags["shape"])
        scales.add((tags["shape"], s))
        ops = [n.op for n in nodes]
        assert ("initialscale" in ops) == (tags["shape"] == "export") and "finalscale" not in ops and "flip" not in ops
        k0 = ops.index("initialscale") + 1 if tags["shape"] == "export" else 0
        assert all(_scale_of(n) == (1.0, 1.0) for n in nodes[:max(k0 - 1, 0)])
        if k0:
            assert _scale_of(nodes[k0 - 1]) == (1.0, s)
        assert all(_scale_of(n) == (s, s) for n in nodes[k0:] if n.data is not None or n.op in ("export_u16", "export_u8")), (seed, ops)
        for n in nodes[k0:]:
            if n.op in ("nlmeans", "diffuse", "bilat"):
                stencils.add(n.op)
            elif n.op == "denoiseprofile":
                stencils.add("denoiseprofile_nlm" if _is_nlm(n) else "denoiseprofile")
        band_lists += bool(tags["bands"])
        if tags["bands"] and s == 2.0 and any(n.op in ("nlmeans", "diffuse") for n in nodes):
            heavy_on_bands += 1
        if tags["shape"] == "rgba":
            assert src.dtype == np.float32 and src.shape[2] == 4
    assert shapes == {"export", "rgba"}
    assert scales == {("export", s) for s in pc.EXPORT_SCALES} | {("rgba", s) for s in pc.RGBA_SCALES}, scales
    assert stencils == {"nlmeans", "diffuse", "bilat", "denoiseprofile", "denoiseprofile_nlm"}, stencils
    assert band_lists >= 4 and heavy_on_bands >= 1, (band_lists, heavy_on_bands)


def _halo(n):
    return lib.load().dt_hip_band_halo_rows(n.op.encode(), C.byref(n.piece), C.cast(C.byref(n.data), C.c_void_p), C.sizeof(n.data))


def _restated_halo(n):
    """nlmeans_core_halo_rows(): P + 1 + the largest shift + the chunk height - 1 (nlmeans_core.c:264-295 gives the height);
    diffuse_halo_rows(): iterations * 3 * (2^scales - 1), the scale count by the oracle (pinned to diffuse.c:1005-1012)"""
    s = n.piece.roi_in.scale
    if _is_nlm(n):
        reach = pc.nlmeans_figures(n.data.radius, s)[2] if n.op == "nlmeans" else pc.dn_nlmeans_figures(n.data, s)[2]
        return reach + ck.oracle().oracle_nlmeans_slice_height(n.piece.roi_out.height) - 1
    assert n.op == "diffuse", n.op
    f = ck.oracle().oracle_diffuse_scales
    f.restype = C.c_int
    return max(int(n.data.iterations), 1) * 3 * ((1 << f(C.byref(n.piece), C.byref(n.data))) - 1)


@pytest.mark.parametrize("scale", sorted(set(pc.EXPORT_SCALES + pc.RGBA_SCALES + (1.0, 1.5, 2.6))))
def test_band_halo_rows_follow_the_scale(scale):
    """dt_hip_band_halo_rows() against the plain restatement, at every scale the scaled lists use (and 1, 1.5, 2.6): every
    parameter set of the generator's pools, on its RGBA frames"""
    seen = set()
    for w, h in pc.RGBA_FRAMES:
        piece = abi.Piece.make(w, h, roi_in=abi.Roi.make(0, 0, w, h, scale), roi_out=abi.Roi.make(0, 0, w, h, scale))
        cases = [("nlmeans", abi.NlmeansData(r, 50.0, 0.5, 1.0)) for r in (1.0, 2.0, 3.0)]
        cases += [("denoiseprofile", params.denoiseprofile(mode=abi.DT_HIP_DENOISEPROFILE_NLMEANS, **o))
                  for o in (dict(), dict(radius=2, nbhood=5, scattering=0.6, central_pixel_weight=0.5))]
        cases += [("diffuse", params.diffuse(name, iscale=i, **over)) for name, over in pc.DIFFUSE.items() for i in (1.0, 1.7)]
        for op, d in cases:
            n = pipe.Node(op, d, piece)
            assert _halo(n) == _restated_halo(n), (op, w, h, scale)
            seen.add(_halo(n))
    if scale == 2.0:
        assert max(seen) > 93  # beyond stencil_halo_bound(): a band that fetched the scale-1 halo would be short


@pytest.mark.parametrize("seed", pc.SCALED_SEEDS)
def test_scaled_lists_bands_and_halos(seed):
    """an eligible scaled list is planned for 2 and 3 bands and no band is shorter than the exact halo a stencil module asks of
    it; the halo of every non-local-means and diffuse node is the restated one; the planner's groups hold no surprise"""
    nodes, _, tags = pc.generate_scaled(seed)
    w, h = nodes[0].piece.roi_out.width, nodes[0].piece.roi_out.height
    for n in nodes:
        if n.data is not None and (_is_nlm(n) or n.op == "diffuse"):
            assert _halo(n) == _restated_halo(n) == pc.exact_halo(n), (seed, n.op)
    assert tags["bands"] == (tags["shape"] == "rgba" and all(pc.band_eligible(nodes, k, pc.exact_halo) for k in (2, 3)))
    if tags["bands"]:
        assert tiled.pipe_demosaic_method(nodes) == -1
        for n_bands in (2, 3):
            bands = tiled.plan_bands(w, h, n_bands, -1)
            assert [(b.row0, b.rows) for b in bands] == pc.band_rows(w, h, -1, n_bands)
            for n in nodes:
                halo = pc.exact_halo(n)
                for k, b in enumerate(bands):
                    assert k == 0 or min(halo, b.row0) <= bands[k - 1].rows, (n.op, halo, k)
                    assert k + 1 == n_bands or min(halo, h - b.row0 - b.rows) <= bands[k + 1].rows, (n.op, halo, k)
    kinds = {k for k, _, _ in pc.plan_groups(nodes)}
    assert kinds <= {"single", "raw", "rgb"}


@functools.lru_cache(maxsize=None)
def _scaled_oracle(seed):
    nodes, src, tags = pc.generate_scaled(seed)
    return nodes, src, tags, pc.oracle_chain(nodes, src)


@pytest.mark.parametrize("seed", pc.SCALED_SEEDS)
def test_every_scaled_pipe_gives_a_picture_that_is_not_the_scale_one_picture(seed):
    nodes, src, tags, out = _scaled_oracle(seed)
    shape, dtype = pc.out_format(nodes)
    assert out.shape == shape and out.dtype == dtype
    unit = {np.dtype(np.uint16): 1.0, np.dtype(np.uint8): 255.0 / 65535.0, np.dtype(np.float32): 1.0 / 65535.0}[out.dtype]
    assert _spread(out) > 100.0 * unit, _spread(out)
    if tags["shape"] == "rgba":
        # the same list with every region at scale 1: a stencil module that read no scale would give these words
        ones = [pipe.Node(n.op, n.data, abi.Piece.from_buffer_copy(n.piece)) for n in nodes]
        for n in ones:
            n.piece.roi_in.scale = n.piece.roi_out.scale = 1.0
        clamped = tags["scale"] > 1.0 and not any(n.op in ("nlmeans", "diffuse", "bilat") for n in nodes)  # denoise (profiled): min(scale, 1)
        assert (pc.count_differing(pc.oracle_chain(ones, src), out) == 0) == clamped, seed


@pytest.mark.parametrize("seed", pc.SCALED_SEEDS)
def test_a_scaled_pipe_ends_in_words_its_modules_wrote(seed):
    """the demosaic (and the local laplacian) leave the fourth channel of their output alone, as the reference does: a list
    that carried it to its end would be compared in words that are whatever the buffers held before.  With every module's
    output buffer full of NaN, or of a finite value, the list ends in the words it ends in over zeroed buffers"""
    nodes, src, _, out = _scaled_oracle(seed)
    assert pc.alpha_is_written(nodes), pc.describe(nodes)
    for fill in (np.nan, 123.25):
        assert pc.count_differing(pc.oracle_chain(nodes, src, fill=fill), out) == 0, (seed, fill)


@pytest.mark.parametrize("seed", pc.SCALED_SEEDS)
def test_scaled_pipe_oracle_equals_the_reference(seed, ref_lib):
    nodes, src, _ = pc.generate_scaled(seed)
    _nodes_equal_the_reference(nodes, src, "scaled seed %d" % seed)


def test_scaled_fused_pairs_fuse_by_rule_and_equal_the_reference_where_it_is_built():
    tb = pc.Tables(False)
    cases = dict((c[0], c) for c in pc.fused_pair_cases(tb, scale=0.5))
    ones = dict((c[0], c) for c in pc.fused_pair_cases(tb))
    found = set()
    for name in pc.SCALED_PAIRS:
        _, nodes, kind, pairs, groups = cases[name]
        assert all(_scale_of(n) == (0.5, 0.5) for n in nodes)
        assert pc.fused_pairs(nodes) == pairs and len(pc.plan_groups(nodes)) == groups, name
        found |= pairs
        out = pc.oracle_chain(nodes, pc.pair_frame(kind))
        assert _spread(out) > (100.0 if out.dtype == np.uint16 else 100.0 / 65535.0), name
        assert pc.count_differing(out, pc.oracle_chain(ones[name][1], pc.pair_frame(kind))) != 0, name
        if ck.ref() is not None:
            _nodes_equal_the_reference(nodes, pc.pair_frame(kind), name + " at 0.5")
    assert found == {"denoiseprofile+run", "bilat+run", "diffuse+rgb_to_lab", "nlmeans>bilat"}
