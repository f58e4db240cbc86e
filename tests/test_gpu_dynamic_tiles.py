"""The dynamic tile walk of the first-order / HR tiled kernels (RDYHIP_TILE_WALK=dynamic) against the static one.

Under the dynamic walk a workgroup's first three tiles are fixed and every later one is drawn from its XCD's counter
(swe_kernels.h; the kernels that have no dynamic walk run the static one under either setting).  What can go wrong shows where workgroups take several tiles and race for them: a draw handed to the
wrong tile of the pipeline, a tile taken twice or never, a counter that is not back at zero for the next launch, a static
launch form that looks at the counters.  So: small meshes under RDYHIP_PGRID = 8 (one workgroup per XCD draws its whole range),
16 (two race for it), 24, and the default grid (one tile per workgroup: every draw comes back empty); 400 triangles (two
tiles: no XCD chunks, the static path under the dynamic setting).  Every call form; bit for bit between the walks and the
grids, and within 1e-10 of the oracle with the oracle's Courant ids."""
import functools

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import PHASE_HALO, PHASE_INTERIOR, WELL_BALANCING_HR

from helpers import rel_linf
from test_gpu_kernel_matrix import _KNOB_VARS, _torch, run_device, run_oracle
from test_gpu_parity import check_all

pytestmark = pytest.mark.gpu
TOL = 1e-10     # the bar of the existing parity tests (they measure 1e-16 .. 1e-15)
K = 2 * np.pi / 50
GRIDS = {"default": {}, "pgrid8": {"RDYHIP_PGRID": "8"}, "pgrid16": {"RDYHIP_PGRID": "16"}, "pgrid24": {"RDYHIP_PGRID": "24"}}
WALKS = ("static", "dynamic")
CALLS = ("rhs", "apply", "euler", "euler_no_f")
# mesh, (source method, hydrostatic reconstruction)
CASES = [("tri_40k", 0, False), ("tri_many_tiles", 0, False), ("quad_many_tiles", 0, False), ("tri_two_tiles", 0, False),
         ("tri_many_tiles", 0, True), ("tri_many_tiles", 1, False), ("quad_many_tiles", 1, False)]


@functools.lru_cache(maxsize=None)
def _case(name, src, hr):
    """the meshes of test_gpu_occupancy.py (bed slopes, a Manning field, a water source, a dry disc, all boundary types) and
    40 000 triangles: about 157 tiles, XCD chunks of 20"""
    nx, ny = {"tri_40k": (200, 100), "tri_many_tiles": (70, 50), "tri_two_tiles": (20, 10), "quad_many_tiles": (90, 78)}[name]
    if name.startswith("tri"):
        # (the 40 000 triangles numbered in blocks, as the benchmark's meshes are: full tiles, 157 of them)
        mesh = M.structured_tri_mesh(nx, ny, 1.0, zfunc=CS.mms_bathymetry(K=K), project_2d=hr, order="tiled" if name == "tri_40k" else "rowmajor")
    else:
        mesh = M.structured_quad_mesh(nx, ny, 1.0, 1.0, zfunc=CS.mms_bathymetry(K=K), project_2d=hr)
    case = CS.friction_slope_case(mesh, float(nx), float(ny), dt=1e-2, source_method=src, K=K)
    if hr:
        case.config.well_balancing = WELL_BALANCING_HR
    rng = np.random.default_rng(len(name) + 7 * src + (13 if hr else 0))
    f0 = rng.normal(size=(case.mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0])
    return case, f0


@functools.lru_cache(maxsize=None)
def _reference(name, src, hr, with_f0):
    case, f0 = _case(name, src, hr)
    return run_oracle(case, f0 if with_f0 else None)


def _set(monkeypatch, grid_env, walk):
    for k in _KNOB_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in grid_env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RDYHIP_TILE_WALK", walk)


def _courant(op):
    op.update_diagnostics()
    d = op.get_diagnostics()
    return (d.max_courant_num, d.global_edge_id, d.global_cell_id)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("name,src,hr", CASES, ids=[f"{n}-src{s}{'-hr' if h else ''}" for n, s, h in CASES])
def test_walks_and_grids_agree_bit_for_bit_and_with_the_oracle(name, src, hr, call, rdyhip_kernel, monkeypatch):
    if rdyhip_kernel == "cell":
        pytest.skip("tiled kernels only")
    case, f0 = _case(name, src, hr)
    fr, orc = _reference(name, src, hr, call == "apply")
    own = case.mesh.cell_owned_to_local
    cref = orc.diagnostics()
    kind = "euler" if call.startswith("euler") else call
    first = None
    for grid, env in GRIDS.items():
        for walk in WALKS:
            _set(monkeypatch, env, walk)
            op, f, out = run_device(case, kind, False, f0=f0 if call == "apply" else None, with_f=call != "euler_no_f")
            info = op.layout_info()
            if grid != "default":
                assert info["persistent_grid"] == int(env["RDYHIP_PGRID"])
            if name == "tri_two_tiles":
                assert info["num_tiles"] < 64          # no XCD chunks: the static path, whatever the setting
            elif name == "tri_40k":
                assert 150 <= info["num_tiles"] <= 170
            else:
                assert info["num_tiles"] >= 3 * 8
            got = out[own] if kind == "euler" else f
            ref = case.u_local[own] + case.dt * fr if kind == "euler" else fr
            err = rel_linf(got, ref)
            print(f"{name} src={src} hr={hr} {call} {grid} {walk}: grid {info['persistent_grid']}, tiles {info['num_tiles']}, rel L-inf vs oracle {err:.3e}")
            assert err <= TOL, (grid, walk, err)
            if call == "euler":
                assert rel_linf(f, fr) <= TOL
            c = _courant(op)
            assert abs(c[0] - cref[0]) <= 1e-12 * max(1.0, cref[0]) and c[1:] == tuple(cref[1:]), (grid, walk, c, cref)
            if first is None:
                first = (got, f, c)
            else:
                assert np.array_equal(got, first[0]), f"{grid} {walk}: differs from the default grid's static walk"
                assert (f is None and first[1] is None) or np.array_equal(f, first[1]), (grid, walk)
                assert c == first[2], (grid, walk, c, first[2])
            op.destroy()


def _five_launches(case, f0):
    """rhs_function / euler_step / apply / euler_step without F / rhs_function on ONE operator, nothing between them but
    the stream's order; then the same operator in INTERIOR + HALO phases.  Returns every result on the host."""
    torch = _torch()
    no = case.mesh.num_owned_cells
    op = CS.create_operator(case)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    fs = [torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda") for _ in range(4)]
    fs[2].copy_(torch.tensor(f0, dtype=torch.float64, device="cuda"))
    outs = [torch.full_like(u, -7.0) for _ in range(2)]
    f_ph = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    op.rhs_function(case.dt, u, fs[0])
    op.euler_step(case.dt, u, outs[0], fs[1])
    op.apply(case.dt, u, fs[2])
    op.euler_step(case.dt, u, outs[1], None)
    op.rhs_function(case.dt, u, fs[3])
    torch.cuda.synchronize()
    c = _courant(op)
    op.apply_phase(PHASE_INTERIOR, True, case.dt, u, f_ph, reset_diagnostics=True)
    op.apply_phase(PHASE_HALO, True, case.dt, u, f_ph)
    torch.cuda.synchronize()
    c_ph = _courant(op)
    res = [t.cpu().numpy() for t in fs + outs + [f_ph]]
    op.destroy()
    return res, c, c_ph


@pytest.mark.parametrize("name,grid", [("tri_40k", "pgrid16"), ("tri_many_tiles", "pgrid16"), ("quad_many_tiles", "pgrid24"), ("tri_40k", "default")])
def test_counters_are_back_at_zero_for_the_next_launch(name, grid, rdyhip_kernel, monkeypatch):
    if rdyhip_kernel == "cell":
        pytest.skip("tiled kernels only")
    case, f0 = _case(name, 0, False)
    _set(monkeypatch, GRIDS[grid], "static")
    ref, c_ref, _ = _five_launches(case, f0)
    _set(monkeypatch, GRIDS[grid], "dynamic")
    got, c, c_ph = _five_launches(case, f0)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), f"result {k} of the back-to-back launches differs from the static walk's"
    assert c == c_ref
    # the first and the last launch are the same call: a counter left over from launches 1-4 would show here
    assert np.array_equal(got[0], got[3])
    # the static launch forms did not see the counters: INTERIOR + HALO give the one-call result
    assert np.array_equal(got[6], got[0]) and c_ph == c


@pytest.mark.parametrize("shape", ["tri", "quad"])
def test_every_tile_on_the_tie_path_under_the_dynamic_walk(shape, rdyhip_kernel, monkeypatch):
    """a lake at rest under a DMPlex-like numbering: every tile of every workgroup runs the Courant tie path, and which
    workgroup meets which tile is up to the race.  The ids must be the oracle's (no near-tie allowance)."""
    if rdyhip_kernel == "cell":
        pytest.skip("tiled kernels only")
    m = M.structured_tri_mesh(70, 50, 1.0) if shape == "tri" else M.structured_quad_mesh(90, 78, 1.0, 1.0)
    m = M.dmplex_like_numbering(m, seed=33)
    case = CS.dam_break_case(m, 1e9, perturb=0.0)    # h = 10 everywhere, at rest
    fr, orc = run_oracle(case)
    seen = []
    for walk in WALKS:
        _set(monkeypatch, GRIDS["pgrid16"], walk)
        op, f, _ = run_device(case, "rhs", False)
        assert op.layout_info()["num_tiles"] >= 3 * 8 and op.layout_info()["persistent_grid"] == 16
        check_all(case, f, fr, op, orc)
        seen.append((f, _courant(op)))
        op.destroy()
    assert np.array_equal(seen[0][0], seen[1][0]) and seen[0][1] == seen[1][1]
