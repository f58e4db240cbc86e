"""The oracle table of test_gpu_kernel_matrix.py against the built library, without a GPU: its rows name exactly the
instantiations of the RHS kernels in the code object (a new template axis or instantiation fails here until it has an oracle
row), every row reaches the instantiation it names by the selection of rdyhip_api.hip, and the meshes of the tile-walk tier
have the tile counts they claim (rdyhip_probe_layout, the host-side layout pass of rdyhip_create)."""
import os
import re
import shutil

import pytest

from rdycore_amd import build, codeobj
from rdycore_amd.operator import RDyFlowConfig, probe_layout

from test_gpu_kernel_matrix import ROWS, WALK_CASES, row_kernel, walk_mesh

_demangler = pytest.mark.skipif(shutil.which("c++filt") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-cxxfilt"),
                                reason="no C++ demangler")
_ARG = {"true": True, "false": False}
T, F = True, False


def kernel_tuple(name):
    """('tiled', S, SRC, OVERWRITE, HR, EULER, FNT) / ('muscl', S, SRC, OVERWRITE, LIM, EULER) / ('cell', S, SRC) of a demangled
    RHS kernel name, None for any other kernel"""
    m = re.search(r"rdyhip::(swe_rhs_tiled_kernel|swe_rhs_muscl_fused_kernel|swe_rhs_kernel)<([^>]*)>", name)
    if m is None:
        return None
    kind = {"swe_rhs_tiled_kernel": "tiled", "swe_rhs_muscl_fused_kernel": "muscl", "swe_rhs_kernel": "cell"}[m.group(1)]
    args = [a.strip() for a in m.group(2).split(",")]
    return (kind,) + tuple(_ARG[a] if a in _ARG else int(a) for a in args)


def library_tuples():
    return {t for t in map(kernel_tuple, codeobj.kernel_hashes(build.lib_path())) if t is not None}


@_demangler
def test_the_table_names_every_instantiation_of_the_library():
    lib = library_tuples()
    assert sum(t[0] in ("tiled", "muscl") for t in lib) == 84 and sum(t[0] == "cell" for t in lib) == 4
    table = [r.kernel for r in ROWS]
    assert len(table) == len(set(table)), "two rows name the same instantiation"
    missing = sorted(lib - set(table), key=str)
    extra = sorted(set(table) - lib, key=str)
    assert not missing, f"instantiations without an oracle row in test_gpu_kernel_matrix.ROWS: {missing}"
    assert not extra, f"rows naming no instantiation of the library: {extra}"


def test_every_row_reaches_the_instantiation_it_names():
    for r in ROWS:
        assert row_kernel(r) == r.kernel, r.id
        assert (r.kernel[0] == "cell") or r.kernel[1] == (3 if r.mesh == "tri" else 4), r.id
        assert r.call in ("rhs", "apply", "euler") and r.layout in ("prefix", "o2l"), r.id
        assert not r.phased or r.layout == "o2l", r.id          # the phases split work only where there are ghosts
    # both numberings and both store forms of u_out in each Euler-step kernel family, phased and unphased
    euler = [r for r in ROWS if r.call == "euler" and r.kernel[0] == "tiled"]
    assert {(r.kernel[1], r.kernel[6], r.layout) for r in euler} == {(s, fnt, lay) for s in (3, 4) for fnt in (T, F) for lay in ("prefix", "o2l")}
    assert {r.phased for r in euler if r.layout == "o2l"} == {True, False}
    assert {r.phased for r in ROWS if r.kernel[0] == "muscl" and r.layout == "o2l"} == {True, False}



@pytest.mark.parametrize("wc", WALK_CASES, ids=[w.name for w in WALK_CASES])
def test_walk_meshes_have_the_tile_counts_they_claim(wc, monkeypatch):
    monkeypatch.setenv("RDYHIP_TILE_CELLS", str(wc.tile_cells))
    for cfg, project_2d, want in ((RDyFlowConfig(), False, wc.num_tiles[0]), (RDyFlowConfig(well_balancing=2), True, wc.num_tiles[0]),
                                  (RDyFlowConfig(second_order=True), False, wc.num_tiles[1])):
        mesh = walk_mesh(wc.name, project_2d)
        assert 15_000 <= mesh.num_cells <= 120_000
        info = probe_layout(cfg, mesh, [0] * len(mesh.boundaries))
        assert info["num_tiles"] == want, (wc.name, cfg)
        assert (info["num_halo_tiles"] > 0) == wc.partition and (info["owned_is_prefix"] == 0) == wc.partition
    # what each case stands for in the walk (first order: rdyhip_api.hip starts XCD chunks at 64 tiles)
    n = wc.num_tiles[0]
    assert {"tri_lt64": n < 64, "quad_64": n == 64, "mixed_mod1": n > 64 and n % 8 == 1, "quad_mult8": n > 64 and n % 8 == 0,
            "tri_part_mod7": n > 64 and n % 8 == 7}[wc.name]


def test_walk_tier_covers_the_knobs():
    from test_gpu_kernel_matrix import KNOBS
    used = [KNOBS[k] for w in WALK_CASES for k in w.knobs]
    assert {k["RDYHIP_PGRID"] for k in used} == {"8", "24"}
    assert {k.get("RDYHIP_XCD_SWIZZLE", "1") for k in used} == {"0", "1"}
    assert {k.get("RDYHIP_BALANCE_ROUNDS", "0") for k in used} == {"0", "1"}
    assert {w.tile_cells for w in WALK_CASES} == {64, 256}
    assert {k.get("RDYHIP_INTERIOR_SHRINK") for w in WALK_CASES if w.partition for k in (KNOBS[n] for n in w.knobs)} >= {None, "2"}
    assert {w.kind for w in WALK_CASES} == {"tri", "quad", "mixed"}
