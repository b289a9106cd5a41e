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
from ansel_amd import abi, lib, synth, tiled


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
