"""The first-order tiled kernel with ONE generation of per-cell streams, and the persistent grid of each family.

The kernel reloads a tile's slot references, flux coefficients, bed slopes, Manning's n and water source into the registers
phase 2 has just read -- at the end of the previous tile instead of a whole tile ahead into a second set -- which is what lets
the plain first-order triangle family run four workgroups per CU.  What can go wrong with it shows only where a workgroup walks
several tiles: a reload placed before the last read of the old values (the cold Courant tie path reads the coefficients and
slot references again), a reload on the last tile, a first tile without its prologue load.  So: tiny meshes under
RDYHIP_PGRID=8 (prologue, steady state and last tile all run; or fewer tiles than workgroups), every call form, in one call and
in INTERIOR + HALO phases, against the oracle (rel L-inf <= 1e-10) and bit for bit between the default grid, the grid of
RDYHIP_BLOCKS_PER_CU=3 and the eight-workgroup walk; a lake at rest, where every tile takes the tie path; and the default
grid of every family on a create without knobs."""
import functools

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig

from helpers import rel_linf
from test_gpu_kernel_matrix import _KNOB_VARS, _torch, run_device, run_oracle
from test_gpu_parity import check_all
from test_occupancy_cpu import FOUR, THREE

pytestmark = pytest.mark.gpu
TOL = 1e-10
K = 2 * np.pi / 50
GRIDS = {"default": {}, "three_per_cu": {"RDYHIP_BLOCKS_PER_CU": "3"}, "walk8": {"RDYHIP_PGRID": "8"}}


@functools.lru_cache(maxsize=None)
def _case(name):
    """bed slopes, a Manning field, a water source, a dry disc and one boundary of each type: every per-cell stream carries
    values that differ from cell to cell"""
    if name == "tri_many_tiles":        # 7 000 cells: at least three tiles per workgroup of the eight, last tile partial
        mesh, lx, ly = M.structured_tri_mesh(70, 50, 1.0, zfunc=CS.mms_bathymetry(K=K)), 70.0, 50.0
    elif name == "tri_two_tiles":       # 400 cells: fewer tiles than workgroups, most workgroups have none
        mesh, lx, ly = M.structured_tri_mesh(20, 10, 1.0, zfunc=CS.mms_bathymetry(K=K)), 20.0, 10.0
    else:                               # 7 020 quads
        mesh, lx, ly = M.structured_quad_mesh(90, 78, 1.0, 1.0, zfunc=CS.mms_bathymetry(K=K)), 90.0, 78.0
    case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2, K=K)
    rng = np.random.default_rng(len(name))
    f0 = rng.normal(size=(mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0])
    return case, f0


@functools.lru_cache(maxsize=None)
def _reference(name, call):
    case, f0 = _case(name)
    return run_oracle(case, f0 if call == "apply" else None)


def _set(monkeypatch, env):
    for k in _KNOB_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _courant(op):
    op.update_diagnostics()
    d = op.get_diagnostics()
    return (d.max_courant_num, d.global_edge_id, d.global_cell_id)


@pytest.mark.parametrize("call", ["rhs", "apply", "euler"])
@pytest.mark.parametrize("name", ["tri_many_tiles", "tri_two_tiles", "quad_many_tiles"])
def test_grids_agree_bit_for_bit_and_with_the_oracle(name, call, rdyhip_kernel, monkeypatch):
    if rdyhip_kernel == "cell":
        pytest.skip("tiled kernels only")
    case, f0 = _case(name)
    fr, orc = _reference(name, call)
    own = case.mesh.cell_owned_to_local
    cref = orc.diagnostics()
    for phased in (False, True):
        first = None
        for grid, env in GRIDS.items():
            _set(monkeypatch, env)
            op, f, out = run_device(case, call, phased, f0=f0 if call == "apply" else None)
            info = op.layout_info()
            if grid == "walk8":
                assert info["persistent_grid"] == 8
                if name == "tri_two_tiles":
                    assert info["num_tiles"] < 8
                else:
                    assert info["num_tiles"] >= 3 * 8 and case.mesh.num_owned_cells % 256 != 0
            got = out[own] if call == "euler" else f
            ref = case.u_local[own] + case.dt * fr if call == "euler" else fr
            err = rel_linf(got, ref)
            print(f"{name} {call} phased={phased} {grid}: grid {info['persistent_grid']}, rel L-inf vs oracle {err:.3e}")
            assert err <= TOL, (grid, phased, err)
            if call == "euler":
                assert rel_linf(f, fr) <= TOL
            c = _courant(op)
            assert abs(c[0] - cref[0]) <= 1e-12 * max(1.0, cref[0]) and c[1:] == tuple(cref[1:]), (grid, phased, c, cref)
            if first is None:
                first = (got, f, c)
            else:
                assert np.array_equal(got, first[0]) and np.array_equal(f, first[1]), f"{grid}, phased={phased}: differs from the default grid's"
                assert c == first[2], (grid, phased, c, first[2])
            op.destroy()


@pytest.mark.parametrize("shape", ["tri", "quad"])
def test_every_tile_on_the_tie_path(shape, rdyhip_kernel, monkeypatch):
    """a lake at rest over a flat bed: every edge of a kind has the same Courant number to the last bit, so every tile of every
    workgroup runs the cold tie path, which reads the cell's coefficients and slot references after the sums -- a reload issued
    too early would hand it the next tile's.  The ids must be the oracle's (no near-tie allowance)."""
    if rdyhip_kernel == "cell":
        pytest.skip("tiled kernels only")
    m = M.structured_tri_mesh(70, 50, 1.0) if shape == "tri" else M.structured_quad_mesh(90, 78, 1.0, 1.0)
    m = M.dmplex_like_numbering(m, seed=33)          # slot order and coefficients change from cell to cell
    case = CS.dam_break_case(m, 1e9, perturb=0.0)    # h = 10 everywhere, at rest
    fr, orc = run_oracle(case)
    seen = []
    for grid, env in GRIDS.items():
        _set(monkeypatch, env)
        op, f, _ = run_device(case, "rhs", False)
        if grid == "walk8":
            assert op.layout_info()["num_tiles"] >= 3 * 8
        check_all(case, f, fr, op, orc)
        seen.append((f, _courant(op)))
        op.destroy()
    assert all(np.array_equal(f, seen[0][0]) and c == seen[0][1] for f, c in seen[1:])


@pytest.mark.parametrize("family", FOUR + THREE, ids=str)
def test_default_grid_of_every_family(family, rdyhip_kernel, monkeypatch):
    if rdyhip_kernel == "cell":
        pytest.skip("tiled kernels only")
    S, src, hr = family
    _set(monkeypatch, {})
    cus = _torch().cuda.get_device_properties(0).multi_processor_count
    mesh = M.structured_tri_mesh(24, 20, 1.0, project_2d=hr) if S == 3 else M.structured_quad_mesh(40, 30, 1.0, 1.0, project_2d=hr)
    case = CS.dam_break_case(mesh, 24.0 if S == 3 else 40.0, source_method=src)
    case.config = RDyFlowConfig(source_method=src, well_balancing=2 if hr else 0)
    op = CS.create_operator(case)
    info = op.layout_info()
    op.destroy()
    assert info["slots_per_cell"] == S and info["tiled_kernel"] == 1
    assert info["persistent_grid"] == (4 if family in FOUR else 3) * cus, (family, info["persistent_grid"], cus)
