"""How the tile loop of the headline kernel addresses its unit-stride data, pinned on a fresh compile (no GPU).

swe_rhs_tiled_kernel<3, 0, true, false, false, true>: every per-cell stream, edge record, halo id and [cell][3] row of a tile lies
at (array + a wave-uniform index) + the lane's 4 tid / 8 tid / row offset.  Written as array[uniform + tid], hipcc builds that
address per lane and per tile in a 64-bit VGPR pair (scalar halves moved into VGPRs, a sign extension, a 64-bit shift-and-add);
lane_ptr (swe_kernels.h) makes the base with scalar adds and the access becomes `global_load v, v_off, s[base:base+1]`.  With it
went the per-tile zeroing of the rows a lane without a cell carries into the store phase (rows_unset) and the two Courant tie
bounds that were fetched a tile ahead (now scalar loads inside the cold tie branch).  Same tool and same "static" count as
tests/test_hot_loop_cpu.py (tools/isa_hot_loop.py: every block of the loop once, cold arms included):

                                                              parent    this kernel
  VALU-issued instructions of the tile loop, static            839         797     (fp64 523 + other VALU 271 + lane ops 3)
  hinted global_load with a scalar base, whole kernel          0 of 27     24 of 26  (the two left: s1 / s2 of a momentum source)
  hinted global_load with a scalar base, tile loop             0           12 of 13
  hinted global_store with a scalar base, whole kernel         0 of 9      9 of 9
  unhinted 4-byte loads (halo ids) with a scalar base          0           4 (1 in the loop)
  VGPRs / scratch                                              126 / 0     127 / 0

(27 -> 26 hinted loads: the water source's two forms are one load with a scalar-selected base and stride, in prologue and loop.)
The bounds leave the few instructions of slack test_hot_loop_cpu.py leaves; a change that moves them is looked at, then the table
is updated."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "swe_rhs_tiled_kernelILi3ELi0ELb1ELb0ELb0ELb1E"
PARENT_LOOP_VALU = 839
MAX_LOOP_VALU = 811           # measured 797; test_hot_loop_cpu.py leaves 14 over its own measurement
MIN_SBASE_LOADS = 24          # measured 24 of the kernel's 26 hinted loads
MIN_SBASE_LOADS_LOOP = 12     # measured 12 of the loop's 13
MIN_SBASE_STORES = 9          # measured 9 of 9
MIN_SBASE_ID_LOADS = 4        # halo ids, unhinted: measured 4 in the kernel, 1 of them in the loop
SBASE = re.compile(r"\bv\d+, (v\[\d+:\d+\], )?s\[\d+:\d+\]")   # "v_off, [data,] s[base:base+1]": a 32-bit lane offset against a scalar base


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def headline(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hot_loop
    d = tmp_path_factory.mktemp("tile_loop_addr")
    src, asm = str(d / "headline.hip"), str(d / "headline.s")
    with open(src, "w") as fh:
        fh.write('#include "swe_kernels.h"\n'
                 "template __global__ void rdyhip::swe_rhs_tiled_kernel<3, 0, true, false, false, true>"
                 "(const rdyhip::KernelArgs, const double, const double *, double *);\n")
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           f"-I{ROOT}/include", f"-I{ROOT}/rdycore_amd/csrc", "-o", asm, src], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    lines = text.split("\n")
    return isa_hot_loop, lines, text


def _hinted(lines, op):
    code = [ln.split(";")[0].strip() for ln in lines]
    return [ln for ln in code if ln.startswith(op) and re.search(r"\bnt\b", ln)]


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_tile_loop_valu_total_is_below_the_parents(headline):
    tool, lines, _ = headline
    bl = tool.blocks(lines, HEADLINE)
    head, back = tool.hot_loop(bl)
    tot = tool.totals(bl, head, back)
    valu = tot["fp64"] + tot["valu"] + tot["lane"]
    print(f"tile loop, static: {dict(tot)}; VALU-issued {valu} (parent {PARENT_LOOP_VALU})")
    assert valu <= MAX_LOOP_VALU < PARENT_LOOP_VALU, tot
    assert tot["fp64"] == 523, tot                      # the arithmetic is what it was


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_hinted_loads_and_stores_take_a_scalar_base(headline):
    tool, lines, _ = headline
    body = tool.kernel_body(lines, HEADLINE)
    loads, stores = _hinted(body, "global_load"), _hinted(body, "global_store")
    n_ld, n_st = sum(1 for ln in loads if SBASE.search(ln)), sum(1 for ln in stores if SBASE.search(ln))
    # the loop's own: the lines between the loop head's label and the back edge
    bl = tool.blocks(lines, HEADLINE)
    head, back = tool.hot_loop(bl)
    first = next(i for i, ln in enumerate(body) if ln.startswith(bl[head].label + ":"))
    after = bl[back + 1].label if back + 1 < len(bl) and bl[back + 1].label.startswith(".LBB") else None
    last = next((i for i, ln in enumerate(body) if after and ln.startswith(after + ":")), len(body))
    loop_loads = _hinted(body[first:last], "global_load")
    n_loop = sum(1 for ln in loop_loads if SBASE.search(ln))
    print(f"hinted loads with a scalar base: {n_ld} of {len(loads)} (tile loop: {n_loop} of {len(loop_loads)}); stores: {n_st} of {len(stores)}")
    assert len(loads) >= 26 and len(stores) >= 9                      # the counts tests/test_isa_cpu.py wants of the built library
    assert n_ld >= MIN_SBASE_LOADS and n_st >= MIN_SBASE_STORES, (n_ld, n_st)
    assert n_loop >= MIN_SBASE_LOADS_LOOP, (n_loop, len(loop_loads))
    assert not [ln for ln in body if ln.split(";")[0].strip().startswith(("flat_load", "flat_store", "buffer_load", "buffer_store"))]
    # the halo ids (hcells) are 4-byte loads WITHOUT the hint: prologue, the next tile's, the loop's batch
    code = [ln.split(";")[0].strip() for ln in body]
    ids = [ln for ln in code if ln.startswith("global_load_dword ") and not re.search(r"\bnt\b", ln) and SBASE.search(ln)]
    ids_loop = [ln for ln in code[first:last] if ln.startswith("global_load_dword ") and not re.search(r"\bnt\b", ln) and SBASE.search(ln)]
    print(f"unhinted 4-byte loads with a scalar base: {len(ids)} (tile loop: {len(ids_loop)})")
    assert len(ids) >= MIN_SBASE_ID_LOADS and len(ids_loop) >= 1, (len(ids), len(ids_loop))


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_headline_kernel_has_no_scratch_and_fits_four_workgroups_per_cu(headline):
    tool, lines, text = headline
    tail = text[text.index("_ZN6rdyhip20" + HEADLINE):]
    tail = tail[tail.index(".Lfunc_end"):]
    scratch = int(re.search(r"; ScratchSize:\s+(\d+)", tail).group(1))
    vgprs = int(re.search(r"; NumVgprs:\s+(\d+)", tail).group(1))
    print(f"scratch {scratch} B, {vgprs} VGPRs")
    assert scratch == 0 and vgprs <= 128, (scratch, vgprs)
    assert not [ln for ln in tool.kernel_body(lines, HEADLINE) if ln.split(";")[0].strip().startswith("scratch_")]
