"""The machine code of the table family (swe_rhs_ntab_kernel: edge normals from an LDS table of the operator's distinct ones)
beside the streamed family (swe_rhs_tiled_kernel: one double per edge record, the other component rebuilt by edge_normal),
without a GPU.  Both include the same body (swe_tiled_body.h); the streamed kernels are byte for byte what they were.

A fresh compile of <3, 0, true, false, false, true> of both, same tool and same "static" count as
tests/test_tile_loop_addressing_cpu.py (tools/isa_hot_loop.py: every block of the tile loop once, cold arms included):

                                                              streamed    table
  fp64 instructions of the tile loop                            523         513    (edge_normal: rsq, Goldschmidt step, fma)
  VALU-issued instructions of the tile loop                     797         772    (fp64 + 256 other + 3 lane ops; streamed 271)
  hinted global_load, whole kernel                              26          22     (e_cs of two rounds, prologue and loop)
  hinted global_load, tile loop                                 13          11
  LDS instructions of the tile loop                             62          63     (one ds_read_b128 per edge: cn, sn)
  hinted global_store with a scalar base                        9 of 9      9 of 9
  VGPRs / scratch                                               127 / 0     118 / 0

The bounds leave the 14 instructions of slack the project's other pins leave over a measurement.

On the built library: 48 table kernels with distinct code beside the 84 + 4 kernels of before, and the selection of
rdyhip_api.hip restated as test_gpu_kernel_matrix.row_kernel restates the streamed one."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from rdycore_amd import build, codeobj

from test_gpu_kernel_matrix import ROWS, row_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = "ILi3ELi0ELb1ELb0ELb0ELb1E"
STREAMED, TABLE = "swe_rhs_tiled_kernel" + ARGS, "swe_rhs_ntab_kernel" + ARGS
STREAMED_FP64, STREAMED_VALU = 523, 797       # pinned by tests/test_tile_loop_addressing_cpu.py
MAX_TABLE_FP64 = 513 + 5                      # measured 513
MAX_TABLE_VALU = 772 + 14                     # measured 772
SBASE = re.compile(r"\bv\d+, (v\[\d+:\d+\], )?s\[\d+:\d+\]")

_demangler = pytest.mark.skipif(shutil.which("c++filt") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-cxxfilt"),
                                reason="no C++ demangler")


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hot_loop
    d = tmp_path_factory.mktemp("normal_table_isa")
    src, asm = str(d / "both.hip"), str(d / "both.s")
    sig = "(const rdyhip::KernelArgs, const double, const double *, double *);\n"
    with open(src, "w") as fh:
        fh.write('#include "swe_kernels.h"\n'
                 "template __global__ void rdyhip::swe_rhs_tiled_kernel<3, 0, true, false, false, true>" + sig +
                 "template __global__ void rdyhip::swe_rhs_ntab_kernel<3, 0, true, false, false, true>" + sig)
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           f"-I{ROOT}/include", f"-I{ROOT}/rdycore_amd/csrc", "-o", asm, src], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    return isa_hot_loop, text.split("\n"), text


def _hinted(lines, op):
    code = [ln.split(";")[0].strip() for ln in lines]
    return [ln for ln in code if ln.startswith(op) and re.search(r"\bnt\b", ln)]


def _loop_lines(tool, lines, pat):
    body = tool.kernel_body(lines, pat)
    bl = tool.blocks(lines, pat)
    head, back = tool.hot_loop(bl)
    first = next(i for i, ln in enumerate(body) if ln.startswith(bl[head].label + ":"))
    after = bl[back + 1].label if back + 1 < len(bl) and bl[back + 1].label.startswith(".LBB") else None
    last = next((i for i, ln in enumerate(body) if after and ln.startswith(after + ":")), len(body))
    return body, body[first:last], tool.totals(bl, head, back)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_the_table_kernels_loop_has_less_arithmetic_and_two_loads_fewer(both):
    tool, lines, _ = both
    body_s, loop_s, tot_s = _loop_lines(tool, lines, STREAMED)
    body_t, loop_t, tot_t = _loop_lines(tool, lines, TABLE)
    valu = lambda t: t["fp64"] + t["valu"] + t["lane"]
    print(f"streamed: {dict(tot_s)} VALU-issued {valu(tot_s)}; hinted loads {len(_hinted(body_s, 'global_load'))} (loop {len(_hinted(loop_s, 'global_load'))})")
    print(f"table:    {dict(tot_t)} VALU-issued {valu(tot_t)}; hinted loads {len(_hinted(body_t, 'global_load'))} (loop {len(_hinted(loop_t, 'global_load'))})")
    assert tot_s["fp64"] == STREAMED_FP64                                      # the streamed kernel compiled beside it is the pinned one
    assert tot_t["fp64"] <= MAX_TABLE_FP64 < STREAMED_FP64, tot_t
    assert valu(tot_t) <= MAX_TABLE_VALU < STREAMED_VALU, tot_t
    assert len(_hinted(loop_t, "global_load")) == len(_hinted(loop_s, "global_load")) - 2       # e_cs of the two rounds
    assert len(_hinted(body_t, "global_load")) == len(_hinted(body_s, "global_load")) - 4       # ... and of the prologue's
    assert tot_t["vmem"] == tot_s["vmem"] - 2 and tot_t["lds"] <= tot_s["lds"] + 2, (tot_t, tot_s)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_the_table_kernel_keeps_the_streamed_kernels_addressing_and_resources(both):
    tool, lines, text = both
    body = tool.kernel_body(lines, TABLE)
    stores = _hinted(body, "global_store")
    assert len(stores) == 9 and all(SBASE.search(ln) for ln in stores), stores
    loads = _hinted(body, "global_load")
    assert sum(1 for ln in loads if SBASE.search(ln)) >= len(loads) - 2           # the two left: s1 / s2 of a momentum source
    code = [ln.split(";")[0].strip() for ln in body]
    assert not [ln for ln in code if ln.startswith(("flat_", "buffer_", "scratch_"))]
    assert [ln for ln in code if ln.startswith("ds_read_b128")], "the (cn, sn) pair is one 16-byte LDS read"
    tail = text[text.index("_ZN6rdyhip19" + TABLE):]
    tail = tail[tail.index(".Lfunc_end"):]
    scratch = int(re.search(r"; ScratchSize:\s+(\d+)", tail).group(1))
    vgprs = int(re.search(r"; NumVgprs:\s+(\d+)", tail).group(1))
    print(f"table kernel: scratch {scratch} B, {vgprs} VGPRs")
    assert scratch == 0 and vgprs <= 128, (scratch, vgprs)


# ---- the built library ------------------------------------------------------------------------------------------------------
_ARG = {"true": True, "false": False}


def _ntab_tuple(name):
    m = re.search(r"rdyhip::swe_rhs_ntab_kernel<([^>]*)>", name)
    return None if m is None else tuple(_ARG[a.strip()] if a.strip() in _ARG else int(a) for a in m.group(1).split(","))


@_demangler
def test_the_library_has_48_table_kernels_beside_the_kernels_of_before():
    lib = build.lib_path()
    h = codeobj.kernel_hashes(lib)
    ntab = [k for k in h if "swe_rhs_ntab_kernel<" in k]
    assert len(ntab) == 48 and len({h[k] for k in ntab}) == 48
    assert not [k for k in ntab if "swe_rhs_tiled_kernel" in k]
    old = [k for k in h if "swe_rhs_tiled_kernel<" in k or "swe_rhs_muscl_fused_kernel<" in k]
    assert len(old) == 84 and len([k for k in h if "rdyhip::swe_rhs_kernel<" in k]) == 4
    assert not {h[k] for k in ntab} & {h[k] for k in old}
    # one table kernel per streamed first-order / HR instantiation, with six template arguments
    streamed = {tuple(r.kernel[1:]) for r in ROWS if r.kernel[0] == "tiled"}
    assert {_ntab_tuple(k) for k in ntab} == streamed and all(len(t) == 6 for t in streamed)
    # resources: four workgroups per CU need <= 128 VGPRs, nothing in scratch
    res = codeobj.kernel_resources(lib)
    for k in ntab:
        assert res[k]["vgpr"] <= 128 and res[k]["scratch"] == 0 and res[k]["agpr"] == 0, (k, res[k])
    # the Euler-step instantiations of both names are told apart from the RHS ones by the fifth argument
    assert sum(codeobj.is_euler_step_kernel(k) for k in ntab) == 16
    assert all(codeobj.is_euler_step_kernel(k) == _ntab_tuple(k)[4] for k in ntab)
    assert sum(codeobj.is_euler_step_kernel(k) for k in old if "tiled" in k) == 16


def table_row_kernel(row, num_keys, streamed_normals=False, kernel_env=None):
    """the kernel rdyhip_create / launch_rhs pick for a row of test_gpu_kernel_matrix.ROWS on a mesh whose edge records have
    num_keys distinct normals: the selection restated.  ("ntab" | "tiled", S, SRC, OVW, HR, EULER, FNT), or the row's own
    kernel where the table does not apply"""
    k = row_kernel(row)
    table = k[0] == "tiled" and kernel_env != "cell" and not streamed_normals and 1 <= num_keys <= 64
    return ("ntab",) + tuple(k[1:]) if table else k


def test_the_selection_follows_the_key_count_the_config_bit_and_the_operator_kind():
    for r in ROWS:
        k = row_kernel(r)
        for keys in (0, 1, 6, 64, 65, 10684):
            got = table_row_kernel(r, keys)
            if k[0] == "tiled" and 1 <= keys <= 64:
                assert got == ("ntab",) + tuple(k[1:]), (r.id, keys)
            else:
                assert got == k, (r.id, keys)
            assert table_row_kernel(r, keys, streamed_normals=True) == k
    # what the sources say: the flag of tiled_kernel_fn comes from the operator's entry count at both call sites, and the
    # count is set only for tiled first-order / HR operators without the config bit
    api = open(os.path.join(ROOT, "rdycore_amd", "csrc", "rdyhip_api.hip")).read()
    assert len(re.findall(r"tiled_kernel_fn\([^;]*\bn(?:t|tab)\);", api)) == 2
    assert "op->use_tiled && !op->muscl && !(config->flags & RDYHIP_CONFIG_STREAMED_NORMALS)" in api
    assert api.count("op->ntab_lds_bytes : op->lds_bytes") == 2
