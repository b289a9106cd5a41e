"""-m gpu: generated node lists (tests/pipe_cases.py generate()) through every walk of the executor.

The executor's other tests feed it sub-sequences of the one node order the two canonical pipes emit.  Here a fixed list
of seeds gives pipes in other orders -- pointwise modules out of pipe order and repeated, stencil and Lab modules
anywhere, blends, flips, the export resampler, every ending -- and each must give the CPU oracle's words through

  1. the per-module C-ABI, node by node                         4. the band walk driven from Python, 2 and 3 bands
  2. dt_hip_pipe_process() with fusion off                      5. dt_hip_pipe_process_bands(), the C driver, 3 bands
  3. dt_hip_pipe_process() with fusion on                       6. dt_hip_batch_*, depth 2, three copies of the frame

(4 and 5 for the lists the band walk takes by rule: pipe_cases.band_eligible()), with the launch groups the restated
planner expects and the runtime's pool back at its baseline.  A generated list the library refuses is a failure: of the
generator, or a bug.  tests/test_pipe_cases.py checks the seed list's coverage and the reference without a GPU.

generate_scaled() gives the same for lists whose RGBA part runs at a region scale != 1 (a reduced-size export behind
initialscale, or an RGBA frame at scale 0.5 / 2): the same walks, band eligibility from the exact halos; and the four fused
pairs of the frame walk run once each at scale 0.5, with the launches read back so that a pair that fell back fails."""
import ctypes as C

import pytest

import hipcheck as hc
import pipe_cases as pc
from ansel_amd import abi, lib

pytestmark = pytest.mark.gpu


def _every_walk(generate, seed):
    hc.hip()
    host_nodes, src, tags = generate(seed)
    what = "seed %d (%s)" % (seed, pc.describe(host_nodes))
    oracle = pc.oracle_chain(host_nodes, src)
    dev = pc.Tables(True)
    try:
        nodes, _, dtags = generate(seed, dev)
        assert [n.op for n in nodes] == [n.op for n in host_nodes] and dtags["bands"] == tags["bands"]
        base = pc.allocated()
        walks = [("module by module", pc.device_modulewise(nodes, src))]
        unfused, g0 = pc.device_pipe(nodes, src, fusion=False)
        fused, g1 = pc.device_pipe(nodes, src, fusion=True)
        assert g0 == len(pc.kept(nodes)) and g1 == len(pc.plan_groups(nodes)), (what, g0, g1, pc.plan_groups(nodes))
        walks += [("fusion off", unfused), ("fusion on", fused)]
        if tags["bands"]:
            walks += [("%d bands" % n, pc.device_bands(nodes, src, n)) for n in (2, 3)]
            walks.append(("3 bands, C driver", pc.device_bands_c(nodes, src, 3)))
        if tags["batch"]:
            walks += [("batch, frame %d" % k, f) for k, f in enumerate(pc.device_batch(nodes, src, depth=2, frames=3))]
        assert pc.allocated() == base, "%s: the pool is %d bytes off its baseline" % (what, pc.allocated() - base)
        for name, got in walks:
            bad = pc.count_differing(got, oracle)
            assert bad == 0, "%s, %s: %d of %d words differ from the oracle" % (what, name, bad, oracle.size)
    finally:
        dev.release()


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_generated_pipe(seed):
    _every_walk(pc.generate, seed)


@pytest.mark.parametrize("seed", pc.SCALED_SEEDS)
def test_generated_pipe_at_a_region_scale(seed):
    _every_walk(pc.generate_scaled, seed)


@pytest.mark.parametrize("name", pc.SCALED_PAIRS)
def test_fused_pairs_at_scale_one_half(name):
    """denoise (profiled) + run, local contrast + run, diffuse + rgb_to_lab and non-local means -> local contrast with every
    region at scale 0.5: the oracle's words with fusion on and off, and -- from the launch profile, as
    tests/test_gpu_fused_variants.py reads it -- the pair in one launch, not its fallback"""
    hc.hip()
    host = dict((c[0], c) for c in pc.fused_pair_cases(pc.Tables(False), scale=0.5))[name]
    _, host_nodes, kind, pairs, groups = host
    assert pairs and all(n.piece.roi_in.scale == 0.5 and n.piece.roi_out.scale == 0.5 for n in host_nodes)
    src = pc.pair_frame(kind)
    oracle = pc.oracle_chain(host_nodes, src)
    dev = pc.Tables(True)
    try:
        nodes = dict((c[0], c) for c in pc.fused_pair_cases(dev, scale=0.5))[name][1]
        base = pc.allocated()
        unfused, g0 = pc.device_pipe(nodes, src, fusion=False)
        fused, g1 = pc.device_pipe(nodes, src, fusion=True)
        assert (g0, g1) == (len(nodes), groups)
        tags = pc.launch_tags(nodes, src)
        assert pc.allocated() == base
        assert pc.count_differing(unfused, oracle) == 0 and pc.count_differing(fused, oracle) == 0
        chain = [t for t in tags if t.startswith("rgb_chain")]
        if "denoiseprofile+run" in pairs:
            assert "dn_finish_chain" in tags and not chain, tags
        if "bilat+run" in pairs:
            assert "bilat_splat" in tags and "bilat_slice" not in tags and chain, tags
        if "diffuse+rgb_to_lab" in pairs:
            assert "rgb_to_lab" not in tags, tags
        if "nlmeans>bilat" in pairs:
            assert "nlm_chunks" in tags and "bilat_splat" in tags, tags
    finally:
        dev.release()


_INVALID = [c[0] for c in pc.invalid_cases(pc.Tables(False))]


@pytest.mark.parametrize("name", _INVALID)
def test_invalid_lists_are_refused_with_the_pool_at_its_baseline(name):
    """an encoder that is not last behind its export node, a flip whose consumer reads another channel count, a blend
    without its module, a blend behind flip: DT_HIP_INVALID_ARG with a reason, nothing launched, nothing kept"""
    l = hc.hip()
    tb = pc.Tables(False)
    _, nodes, words = pc.invalid_cases(tb)[_INVALID.index(name)]
    base = pc.allocated()
    din, dout = lib.DeviceBuffer(0, 64 * 48 * 16), lib.DeviceBuffer(0, 1 << 20)
    h = l.dt_hip_pipe_new(0)
    try:
        rc = abi.DT_HIP_SUCCESS
        for n in nodes:
            data = C.cast(C.byref(n.data), C.c_void_p) if n.data is not None else None
            rc = l.dt_hip_pipe_add_node(h, n.op.encode(), C.byref(n.piece), data, C.sizeof(n.data) if n.data is not None else 0)
            if rc != abi.DT_HIP_SUCCESS:
                break
        if rc == abi.DT_HIP_SUCCESS:
            rc = l.dt_hip_pipe_process(h, din.ptr, dout.ptr)
        assert rc == abi.DT_HIP_INVALID_ARG, (name, rc)
        assert words in l.dt_hip_last_error().decode(), l.dt_hip_last_error()
    finally:
        l.dt_hip_pipe_free(h)
        din.release()
        dout.release()
    assert pc.allocated() == base
