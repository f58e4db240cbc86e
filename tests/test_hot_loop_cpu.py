"""What the tile loop of the headline kernel issues besides arithmetic, pinned on a fresh compile (no GPU).

swe_rhs_tiled_kernel<3, 0, true, false, false, true> is the one launch per step of the flagship workload.  At four workgroups
per CU its waves queue for the VALU, so every VALU-issued instruction of the tile loop counts -- also the ones that compute
nothing: restores of SGPRs that hipcc spilled to VGPR lanes (v_readlane_b32, one per register), moves, selects and 64-bit
address arithmetic.  tools/isa_hot_loop.py counts them per basic block of a `hipcc -S` dump; this test compiles that one
instantiation alone (two seconds; its code is the same as in the library's translation unit, where the other 87 RHS kernels
take a minute) and holds two figures of profiles/RESULTS_LOG.md section 16:

                                                         parent    this kernel
  v_readlane_b32 + v_writelane_b32, whole kernel          244          8
  VALU-issued instructions of the tile loop, static       1000        826     (fp64 523 + other VALU 301 + lane ops 2)

"static": every basic block between the loop head and the back edge once, cold arms included (the tool's totals).  The bounds
leave a few instructions of slack for a compiler update; a change that moves them is looked at, then the table is updated."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "swe_rhs_tiled_kernelILi3ELi0ELb1ELb0ELb0ELb1E"
MAX_LANE_OPS = 12        # measured 8; the parent commit: 244
MAX_LOOP_VALU = 840      # measured 826; the parent commit: 1000
PARENT_LANE_OPS, PARENT_LOOP_VALU = 244, 1000


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def headline_blocks(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hot_loop
    d = tmp_path_factory.mktemp("hot_loop")
    src, asm = str(d / "headline.hip"), str(d / "headline.s")
    with open(src, "w") as fh:
        fh.write('#include "swe_kernels.h"\n'
                 "template __global__ void rdyhip::swe_rhs_tiled_kernel<3, 0, true, false, false, true>"
                 "(const rdyhip::KernelArgs, const double, const double *, double *);\n")
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           f"-I{ROOT}/include", f"-I{ROOT}/rdycore_amd/csrc", "-o", asm, src], stderr=subprocess.DEVNULL)
    lines = open(asm).read().split("\n")
    return isa_hot_loop, isa_hot_loop.blocks(lines, HEADLINE), lines


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_tile_loop_is_found_and_holds_both_barriers(headline_blocks):
    tool, bl, _ = headline_blocks
    head, back = tool.hot_loop(bl)
    assert sum(b.barriers for b in bl[head:back + 1]) == 2            # phase 0 | phase 1 | phase 2
    assert any(t == bl[head].label for _, t in bl[back].branches)     # the back edge jumps to the head
    tot = tool.totals(bl, head, back)
    assert tot["fp64"] >= 400 and tot["vmem"] >= 20 and tot["lds"] >= 30, tot       # it is the loop with the work in it


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_headline_kernel_restores_no_pointers_through_lanes(headline_blocks):
    tool, bl, lines = headline_blocks
    lane = sum(b.counts["lane"] for b in bl)
    assert lane == tool.static_ops(lines, HEADLINE)
    print(f"lane ops, whole kernel: {lane}")
    assert lane <= MAX_LANE_OPS < PARENT_LANE_OPS, lane


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_headline_tile_loop_valu_total(headline_blocks):
    tool, bl, _ = headline_blocks
    head, back = tool.hot_loop(bl)
    tot = tool.totals(bl, head, back)
    valu = tot["fp64"] + tot["valu"] + tot["lane"]
    print(f"tile loop, static: {dict(tot)}; VALU-issued {valu}")
    assert valu <= MAX_LOOP_VALU < PARENT_LOOP_VALU, tot
    assert tot["lane"] <= 4, tot
