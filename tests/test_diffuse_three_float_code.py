"""What the compiler made of the three-float kernels of diffuse or sharpen (tools/kernel_resources.py and the disassembly of
diffuse.o): no scratch, at most 128 VGPRs, the PDE's support rows by global_load_lds_dwordx3 with no register-destination
global load, and the float4 DMA kernel still there for every mode (the second sequence and the configurations the first does
not cover)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

OBJ = os.path.join(ROOT, "ansel_amd", "csrc", "_obj")
NEW = [r"^void diffuse_pde_strip3<", r"^void bspline_decompose_strip3<"]


@pytest.fixture(scope="module")
def kernels():
    if not os.path.isdir(OBJ) or not any(f.endswith(".o") for f in os.listdir(OBJ)):
        pytest.skip("no objects under ansel_amd/csrc/_obj (run __graft_entry__.build())")
    return kr.table(OBJ)


def test_three_float_kernels_use_no_scratch_and_at_most_128_vgprs(kernels):
    found = [k for k in kernels if any(re.search(p, k["demangled"]) for p in NEW)]
    for p in NEW:
        assert any(re.search(p, k["demangled"]) for k in found), p
    assert len(found) >= 10, len(found)  # 4 PDE (two modes x float4 / three-float first plane) + 6 analyses
    bad = ["%s: %d B scratch, %d VGPR" % (k["demangled"][:80], k["scratch"], k["vgpr"]) for k in found
           if k["scratch"] != 0 or k["vgpr_spills"] != 0 or k["vgpr"] > 128]
    assert not bad, "\n".join(bad)


def test_the_float4_dma_pde_exists_for_every_mode(kernels):
    names = {re.sub(r"\(.*", "", k["demangled"]) for k in kernels}
    modes = {m.group(1) for m in (re.match(r"void diffuse_pde_strip<true, (-?\d+), true>$", n) for n in names) if m}
    assert len(modes) == 9, modes


def _disassembly(obj):
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat"), os.path.join(td, "co")
        subprocess.run([kr.LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
        subprocess.run([kr.LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        return subprocess.run([kr.LLVM + "/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout


def test_the_three_float_pde_fetches_its_rows_by_dwordx3_dma():
    """the bench's instantiation (PDE_MODE_DEBLUR = 253; three-float first plane): 36 global_load_lds_dwordx3 (three planes x main +
    halo piece x three unrolled row steps + the prologue's three rows) and no register-destination global load at all (it has no
    luminance mask); the launch at scale 0 of the first iteration takes its first plane by global_load_lds_dwordx4"""
    obj = os.path.join(OBJ, "diffuse.o")
    if not os.path.exists(obj):
        pytest.skip("no diffuse.o")
    text = _disassembly(obj)
    bodies = {}
    for h0_4 in (0, 1):
        m = re.search(r"<_ZN\S*diffuse_pde_strip3ILi253ELb%dE\S*>:\n(.*?)\n\n" % h0_4, text, re.S)
        assert m, "diffuse_pde_strip3<253, %d> not found in diffuse.o" % h0_4
        bodies[h0_4] = m.group(1)
    for h0_4, body in bodies.items():
        assert body.count("global_load_lds_dwordx3") == (24 if h0_4 else 36), body.count("global_load_lds_dwordx3")
        assert body.count("global_load_lds_dwordx4") == (12 if h0_4 else 0)
        assert not re.search(r"global_load_(dword|ubyte|ushort|sbyte|short)", body.replace("global_load_lds_", "")), h0_4
        assert "global_store_dwordx3" in body and "global_store_dwordx4" in body  # three-float planes; the float4 output
