"""CPU: the tables of the host-side layout pass (rdycore_amd/csrc/host_layout.h), byte for byte, from a stand-alone host
program built under the address and undefined-behaviour sanitizers (tests/host/layout_dump.cpp; never loaded into Python,
never run on a device).  For every case the program must end without a sanitizer report, give the layout numbers
rdyhip_probe_layout gives through the library, and give the FNV-1a hash of every table recorded in
tests/golden/layout_tables.json -- recorded from the program at the revision that moved the layout pass, unchanged, out of
rdyhip_api.hip, so that any later edit of the pass that changes a table shows here.

Regenerate (only when a table is meant to change; the `device_bytes` section of the file is kept as it is):

    python tests/test_layout_tables_cpu.py --regenerate
"""
import copy
import ctypes as C
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig, RDyHipError, _abi_arguments, probe_layout

GOLDEN = os.path.join(ROOT, "tests", "golden", "layout_tables.json")
SOURCE = os.path.join(ROOT, "tests", "host", "layout_dump.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _random_tri():
    rng = np.random.default_rng(0)
    xyz, conn, _, _ = M.structured_tri_connectivity(64, 48)
    return M.build_mesh(xyz, conn[rng.permutation(conn.shape[0])], boundary_classifier=M.single_boundary())


def _interleaved():
    xyz, conn, cx = M.structured_tri_connectivity(24, 10)[:3]
    return M.extract_local_mesh(xyz, conn, cx < 12, ghosts="interleaved")


# name -> (mesh, the configurations it runs with).  The smallest meshes that still reach every capacity a tile is cut to:
# tri6x4       48 owned cells, 1 tile
# random64x48  6144 cells numbered at random, 192 tiles: hmax = 96 of 104 (one more 16-cell granule no longer fits); second order
#              hmax2 = 256, the ring capacity itself
# quads64x32   1801 cells, 8 tiles, S = 4: emax = 511, the cut at 512 edge records; second order hmax2 = 166 of 168
# strip40x48   one rank of a strip partition: 96 ghost cells, 9 halo tiles; second order: extra Courant edges, edge_is_owned
# interleaved  ghosts numbered between the owned cells: owned_is_prefix = 0
# hr32x16      hydrostatic reconstruction: the HR LDS size (second order with HR is an argument error, so first order only)
MESHES = {
    "tri6x4": lambda: M.structured_tri_mesh(6, 4, project_2d=True),
    "random64x48": _random_tri,
    "quads64x32": lambda: CS.dam_break_quads_mesh(64, 32, 0, 1, order="tiled"),
    "strip40x48": lambda: M.strip_partition_tri_mesh(40, 48, 1, 3, order="tiled", tile=8),
    "interleaved": _interleaved,
    "hr32x16": lambda: M.structured_tri_mesh(32, 16, order="tiled"),
}
FIRST, SECOND, HR = RDyFlowConfig(), RDyFlowConfig(second_order=True), RDyFlowConfig(well_balancing=2)
CASES = [("tri6x4", "first", FIRST)]
CASES += [(m, o, c) for m in ("random64x48", "quads64x32", "strip40x48", "interleaved") for o, c in (("first", FIRST), ("second", SECOND))]
CASES += [("hr32x16", "hr", HR)]

_mesh_cache = {}


def case_mesh(name):
    if name not in _mesh_cache:
        _mesh_cache[name] = MESHES[name]()
    return _mesh_cache[name]


def write_case(path, config, mesh):
    """the arguments rdyhip_probe_layout gets for (config, mesh), as the flat file layout_dump.cpp reads"""
    cfg, m, nb, barr, _, _keep = _abi_arguments(config, mesh, None)
    nc, ne, ni, nv = m.num_cells, m.num_edges, m.num_internal_edges, m.num_vertices
    arrays = [("cell_is_owned", np.int32, nc), ("cell_local_to_owned", np.int32, nc), ("cell_global_ids", np.int64, nc),
              ("cell_areas", np.float64, nc), ("cell_dz_dx", np.float64, nc), ("cell_dz_dy", np.float64, nc),
              ("edge_cell_ids", np.int32, 2 * ne), ("edge_internal_ids", np.int32, ni), ("edge_global_ids", np.int64, ne),
              ("edge_lengths", np.float64, ne), ("edge_cn", np.float64, ne), ("edge_sn", np.float64, ne), ("cell_zc", np.float64, nc),
              ("cell_centroids", np.float64, 3 * nc), ("edge_vertex_ids", np.int32, 2 * ne), ("vertex_points", np.float64, 3 * nv),
              ("edge_is_owned", np.int32, ne)]

    def block(ptr, dtype, n):
        if not ptr:
            return struct.pack("<q", -1)
        data = C.string_at(ptr, n * np.dtype(dtype).itemsize) if n else b""
        return struct.pack("<q", n) + data

    with open(path, "wb") as fh:
        fh.write(b"RDYLAY01" + bytes(cfg) + struct.pack("<6i", nc, m.num_owned_cells, ne, ni, nv, nb))
        for name, dtype, n in arrays:
            fh.write(block(getattr(m, name), dtype, n))
        for i in range(nb):
            fh.write(struct.pack("<i", barr[i].condition_type) + block(barr[i].edge_ids, np.int32, barr[i].num_edges))


def build_program(out_dir):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(out_dir), "layout_dump")
    # the sanitizer runtimes linked into the program (clang++ does so by itself): it runs whatever else the environment preloads
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx] + FLAGS + static + [f"-I{ROOT}/include", f"-I{ROOT}/rdycore_amd/csrc", "-o", exe, SOURCE])
    return exe


def run_program(exe, path):
    env = {k: v for k, v in os.environ.items() if k != "RDYHIP_TILE_CELLS"}   # (the layout pass's one knob)
    return subprocess.run([exe, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("layout_dump"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name,order,config", CASES, ids=[f"{m}-{o}" for m, o, _ in CASES])
def test_tables_of_the_layout_pass_are_the_recorded_ones_and_clean_under_sanitizers(program, golden, tmp_path, name, order, config):
    mesh = case_mesh(name)
    path = str(tmp_path / "case.bin")
    write_case(path, config, mesh)
    r = run_program(program, path)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    out = json.loads(r.stdout)
    assert out["rc"] == 0
    assert out["info"] == probe_layout(config, mesh)
    assert out["tables"] == golden["tables"][f"{name}-{order}"]


def _broken_meshes():
    base = M.structured_tri_mesh(6, 4, project_2d=True)

    def broken(**kw):
        m = copy.copy(base)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    # the same three as test_layout_cpu.test_argument_errors_of_create_without_a_device
    l2o = base.cell_local_to_owned.copy()
    l2o[1] = l2o[0]
    yield "local_to_owned_not_bijective", broken(cell_local_to_owned=l2o)
    ec = base.edge_cell_ids.copy()
    ec[2 * int(base.edge_internal_ids[0]) + 1] = base.num_cells + 5
    yield "edge_cell_out_of_range", broken(edge_cell_ids=ec)
    ec = base.edge_cell_ids.copy()
    e3 = base.edge_internal_ids[:3]
    ec[2 * e3.astype(int)] = 0
    ec[2 * e3.astype(int) + 1] = np.arange(1, 4)
    for e in base.edge_internal_ids[3:6]:
        ec[2 * int(e)] = 0
    yield "cell_with_five_edges", broken(edge_cell_ids=ec)


@pytest.mark.parametrize("name,mesh", list(_broken_meshes()), ids=[n for n, _ in _broken_meshes()])
def test_broken_meshes_end_with_the_librarys_code_and_message_and_no_report(program, tmp_path, name, mesh):
    with pytest.raises(RDyHipError) as e:
        probe_layout(FIRST, mesh)
    path = str(tmp_path / "case.bin")
    write_case(path, FIRST, mesh)
    r = run_program(program, path)
    assert r.stderr == "", r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert r.returncode == out["rc"] == e.value.code and out["error"] == e.value.message


if __name__ == "__main__":
    import tempfile
    assert sys.argv[1:] == ["--regenerate"], __doc__
    with tempfile.TemporaryDirectory() as d:
        exe = build_program(d)
        tables = {}
        for name, order, config in CASES:
            write_case(os.path.join(d, "case.bin"), config, case_mesh(name))
            r = run_program(exe, os.path.join(d, "case.bin"))
            assert r.returncode == 0 and r.stderr == "", (name, order, r.returncode, r.stderr[-4000:])
            tables[f"{name}-{order}"] = json.loads(r.stdout)["tables"]
    doc = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    doc["tables"] = tables
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
