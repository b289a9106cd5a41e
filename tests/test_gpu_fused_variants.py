"""-m gpu: every instantiation of the fused RGBA kernel, its run-time switches and the frame walk's four fused pairs.

rgb_chain<CM, FM> (rgb_chain_kernel.h) exists for 6 colour-calibration kinds x 5 filmic modes, in five translation units
whose copies of px_channelmixerrgb / px_filmicrgb are not the ones test_gpu_color.py and test_gpu_filmic.py launch.  Each
case here runs one node list four ways -- the executor with fusion on, with fusion off, module by module through the
C-ABI, and the CPU oracle -- and every word must agree (floats by bit pattern).  The number of launch groups is asserted
with it: a planner that quietly stopped fusing would otherwise pass."""
import numpy as np
import pytest

import hipcheck as hc
import pipe_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables():
    hc.hip()
    dev, host = pc.Tables(True), pc.Tables(False)
    yield dev, host
    dev.release()


def _four_ways(dev_nodes, host_nodes, src, groups, what):
    base = pc.allocated()
    fused, g1 = pc.device_pipe(dev_nodes, src, fusion=True)
    unfused, g0 = pc.device_pipe(dev_nodes, src, fusion=False)
    modulewise = pc.device_modulewise(dev_nodes, src)
    assert pc.allocated() == base, "%s: the pool is %d bytes off its baseline" % (what, pc.allocated() - base)
    oracle = pc.oracle_chain(host_nodes, src)
    assert g0 == len(pc.kept(dev_nodes)) and g1 == groups, "%s: %d groups without fusion, %d with (expected %d)" % (what, g0, g1, groups)
    for name, got in (("fusion on", fused), ("fusion off", unfused), ("module by module", modulewise)):
        bad = pc.count_differing(got, oracle)
        assert bad == 0, "%s, %s: %d of %d words differ from the oracle" % (what, name, bad, oracle.size)
    return oracle


@pytest.mark.parametrize("end", ["u16", "float"])
@pytest.mark.parametrize("imgname", ["scene", "adversarial"])
@pytest.mark.parametrize("fm", pc.FM_KINDS, ids=["fm_none"] + [pc.FILMIC_MODE[f] for f in pc.FM_KINDS[1:]])
@pytest.mark.parametrize("cm", pc.CM_KINDS, ids=["cm_none"] + ["cm_%d" % a for a in pc.ADAPTATIONS])
def test_every_instantiation_of_rgb_chain(tables, cm, fm, imgname, end):
    """exposure -> colorin -> [color calibration] -> [filmic] -> colorout -> export_u16 in ONE launch: all 30 kernels.  And
    the same run ending in float, where no 16-bit rounding stands between a kernel's last bit and the comparison"""
    dev, host = tables
    img = pc.variant_frames()[imgname]
    out = _four_ways(pc.run_nodes_of(dev, cm, fm, end=end), pc.run_nodes_of(host, cm, fm, end=end), img, 1,
                     "cm %s, fm %s, %s, %s" % (cm, fm, imgname, end))
    if end == "u16":
        assert out.dtype == np.uint16 and out.std() > 100
    else:
        assert out.dtype == np.float32 and out[np.isfinite(out)].std() > 100.0 / 65535.0


_PAIRWISE = pc.pairwise_cases()[0]


@pytest.mark.parametrize("case", _PAIRWISE, ids=["-".join(str(v) for v in c) for c in _PAIRWISE])
def test_switches_of_rgb_chain_pairwise(tables, case):
    """has_exposure / has_colorin / has_colorout in every subset, the three endings, the Lab glue on either side, cm_clip,
    filmic_export and the flavours of px_conversion_rt: every pair of values in some case (tests/test_pipe_cases.py checks
    the covering), one launch each"""
    dev, host = tables
    kw = pc.pairwise_kwargs(case)
    src = pc.variant_lab_frame() if kw["pre_lab"] else pc.variant_frames()["scene"]
    _four_ways(pc.run_nodes_of(dev, **kw), pc.run_nodes_of(host, **kw), src, 1, repr(kw))


_PAIR_NAMES = [c[0] for c in pc.fused_pair_cases(pc.Tables(False))]


@pytest.mark.parametrize("name", _PAIR_NAMES)
def test_fused_pairs_and_their_fallbacks(tables, name):
    """denoise (profiled) + run, local contrast + run, diffuse + rgb_to_lab, non-local means -> local contrast through the
    cells plane: the combinations that run in one launch and the ones that must run apart give the oracle's words, and
    every intermediate goes back to the pool.

    The pairs are made inside the walk, where the number of groups does not see them, so the launches are read from the
    runtime's profile: a pair that fused did not launch its second half on its own -- no rgb_chain behind dn_finish_chain,
    no bilat_slice, no rgb_to_lab -- and a fallback did.  (The cells plane between non-local means and local contrast has
    no launch of its own on either path -- bilat_zcells runs under the tag of the splat -- so for it only the words are
    pinned.)"""
    dev, host = tables
    k = _PAIR_NAMES.index(name)
    _, dev_nodes, kind, pairs, groups = pc.fused_pair_cases(dev)[k]
    host_nodes = pc.fused_pair_cases(host)[k][1]
    src = pc.pair_frame(kind)
    _four_ways(dev_nodes, host_nodes, src, groups, name)
    tags = pc.launch_tags(dev_nodes, src)
    ops = [n.op for n in dev_nodes]
    chain = [t for t in tags if t.startswith("rgb_chain")]
    if ops[0] == "denoiseprofile":
        if "denoiseprofile+run" in pairs:
            assert "dn_finish_chain" in tags and not chain, tags
        else:
            assert "dn_finish_chain" not in tags and chain, tags
    if "bilat" in ops and dev_nodes[ops.index("bilat")].data.mode == 0:
        assert "bilat_splat" in tags and ("bilat_slice" not in tags) == ("bilat+run" in pairs), tags
        assert chain, tags  # the fused pair is the run's own launch, the slice its first stage
    if ops[0] == "diffuse":
        assert ("rgb_to_lab" not in tags) == ("diffuse+rgb_to_lab" in pairs), tags
