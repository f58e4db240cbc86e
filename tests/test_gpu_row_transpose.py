"""The [cell][3] stores of the first-order / HR tiled kernel, transposed through LDS that the storing wave owns.

F, the primitive variables, the flux divergence and the unit-stride u_out of an Euler step leave the kernel as whole lines:
lane l of a wave writes its row to elements 3 l .. 3 l + 2 of the wave's own 64 entries of three LDS planes, then reads elements
l, 64 + l, 128 + l and stores them at a unit stride (wave_store_rows3_lds, swe_kernels.h).  What can go wrong with that shows
in the rows themselves: a row in another cell's place, a component in another's, a wave that reads what its neighbour wrote, a
partly filled wave that stores past its cells, a tile whose phase 0 finds the planes not yet rewritten.  So every array that
goes through the transpose is checked, on every mesh, in every call form, with and without the two optional arrays:

  * against the CPU oracle at the project's bar, rel L-inf <= 1e-10 against max(1, |ref|);
  * the primitive variables bit for bit against the cell-centric kernel (RDYHIP_KERNEL=cell), which stores each row from the
    thread that owns the cell and derives (h, u, v) with the same riemann_side: pure data movement, so any misplaced value
    shows.  F, the flux divergence and u_out of that kernel are not the tiled kernel's to the last bit (it reads both
    components of an edge normal where the tiled kernels rebuild one from the other: F of the two differs by 2e-17 ...
    7e-16 on these five meshes), so those are held bit for bit
    against the same kernel on the grid of RDYHIP_BLOCKS_PER_CU=3 (other waves share a SIMD, tiles fall to other
    workgroups) and against each other across the requests: F must not change when pv or fdiv is also stored through the
    same LDS entries right after it.

Meshes, the smallest at which each thing can happen: 8 triangles (one tile, one partly filled wave); 400 triangles (256 + 144:
wave 2 of the second tile holds 16 cells, wave 3 none); 7 000 triangles in 71 tiles with a dry disc (several tiles per
workgroup under RDYHIP_PGRID=8: the next tile's phase 0 rewrites the entries the stores borrowed); 7 200 quads numbered in
16 x 15 blocks (240-cell tiles: wave 3 holds 48 cells, 112 halo slots shift every plane); one rank's part with interleaved
ghosts (o2l: u_out rows are scattered, F / pv / fdiv still go through the transpose)."""
import functools

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M

from helpers import rel_linf
from random_cases import random_case
from test_gpu_kernel_matrix import _KNOB_VARS, _torch, matrix_mesh, run_oracle
from rdycore_amd.operator import RDyFlowConfig

pytestmark = pytest.mark.gpu
TOL = 1e-10
K = 2 * np.pi / 50
MESHES = ["tri8", "tri400", "tri7000", "quad240", "part_o2l"]
CALLS = ["rhs", "apply", "euler_f", "euler"]
REQUESTS = ["none", "pv", "fdiv"]
# name -> (environment, what is compared bit for bit with the default run)
OTHERS = {"cell": ({"RDYHIP_KERNEL": "cell"}, ("pv",)), "three_per_cu": ({"RDYHIP_BLOCKS_PER_CU": "3"}, ("f", "out", "pv", "fdiv"))}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, f0, (number of tiles, owned cells), environment of every run)"""
    env = {}
    if name == "part_o2l":
        mesh = matrix_mesh("tri", "o2l", False)
        rng = np.random.default_rng(9100)
        case = random_case(rng, mesh, RDyFlowConfig(tiny_h=1e-5), region_block=64)
        case.dt = 1e-2
        shape = (27, 2759)
    else:
        if name == "tri8":
            mesh, lx, ly, shape = M.structured_tri_mesh(2, 2, 1.0, zfunc=CS.mms_bathymetry(K=K)), 2.0, 2.0, (1, 8)
        elif name == "tri400":
            mesh, lx, ly, shape = M.structured_tri_mesh(20, 10, 1.0, zfunc=CS.mms_bathymetry(K=K)), 20.0, 10.0, (2, 400)
        elif name == "tri7000":
            mesh, lx, ly, shape = M.structured_tri_mesh(70, 50, 1.0, zfunc=CS.mms_bathymetry(K=K)), 70.0, 50.0, (71, 7000)
            env = {"RDYHIP_PGRID": "8"}
        else:
            nx, ny = 96, 75                                   # 6 x 5 blocks of 16 x 15 squares, numbered block by block
            mesh = M.structured_quad_mesh(nx, ny, 1.0, 1.0, zfunc=CS.mms_bathymetry(K=K))
            i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
            key = ((j // 15) * (nx // 16) + i // 16) * 240 + (j % 15) * 16 + i % 16
            mesh = M.renumber_cells(mesh, np.argsort(key.ravel(), kind="stable"))
            lx, ly, shape = 96.0, 75.0, (30, 30 * 240)
            env = {"RDYHIP_PGRID": "8"}
        case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2, K=K)
    rng = np.random.default_rng(len(name))
    f0 = rng.normal(size=(case.mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0])
    return case, f0, shape, env


@functools.lru_cache(maxsize=None)
def _reference(name, accumulate):
    """(F, pv, flux divergence) of the oracle: computed once per mesh and form, shared, never written to"""
    case, f0, _, _ = _case(name)
    fr, orc = run_oracle(case, f0 if accumulate else None)
    out = (fr.copy(), orc.primitive_variables.copy(), np.array(orc.flux_divergence, copy=True))
    for a in out:
        a.setflags(write=False)
    return out


def _run(case, f0, call, request):
    """one evaluation on a new operator; (F, u_out, pv, fdiv) on the host, None where the call leaves none"""
    torch = _torch()
    no = case.mesh.num_owned_cells
    op = CS.create_operator(case)
    pv = op.primitive_variables if request == "pv" else None          # asked for before the evaluation: the kernel stores it
    if request == "fdiv":
        op.enable_flux_divergence(True)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f = out = None
    if call in ("euler", "euler_f"):
        out = torch.full_like(u, -7.0)
        f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda") if call == "euler_f" else None
        op.euler_step(case.dt, u, out, f)
    elif call == "rhs":
        f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
        op.rhs_function(case.dt, u, f)
    else:
        f = torch.tensor(f0, dtype=torch.float64, device="cuda")
        op.reset_diagnostics()
        op.apply(case.dt, u, f)
    torch.cuda.synchronize()
    info = op.layout_info()
    res = {"f": None if f is None else f.cpu().numpy(), "out": None if out is None else out.cpu().numpy(),
           "pv": None if pv is None else pv.cpu().numpy(), "fdiv": op.flux_divergence.cpu().numpy() if request == "fdiv" else None}
    op.destroy()
    return res, info


def _set(monkeypatch, env):
    for k in _KNOB_VARS + ("RDYHIP_KERNEL",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("name", MESHES)
def test_transposed_rows(name, call, monkeypatch):
    case, f0, (ntiles, ncells), env = _case(name)
    mesh = case.mesh
    own = mesh.cell_owned_to_local
    ghost = mesh.cell_is_owned == 0
    accumulate = call == "apply"
    fr, pvr, fdr = _reference(name, accumulate)
    outr = case.u_local[own] + case.dt * fr
    f_plain = None
    for request in REQUESTS:
        _set(monkeypatch, env)
        got, info = _run(case, f0, call, request)
        assert info["tiled_kernel"] == 1 and info["num_tiles"] == ntiles, info
        assert info["owned_is_prefix"] == (name != "part_o2l")
        assert mesh.num_owned_cells == ncells
        if env.get("RDYHIP_PGRID"):
            assert info["persistent_grid"] == 8 and ntiles >= 3 * 8
        refs = {"f": fr, "out": outr, "pv": pvr, "fdiv": fdr}
        for key, ref in refs.items():
            if got[key] is None:
                continue
            val = got[key][own] if key == "out" else got[key]
            err = rel_linf(val, ref)
            print(f"{name} {call} +{request}: {key} rel L-inf vs oracle {err:.3e}")
            assert err <= TOL, (name, call, request, key, err)
        if got["out"] is not None:
            assert np.all(got["out"][ghost] == -7.0), "ghost rows of u_out were written"
        # F (u_out) does not depend on what else is stored through the same LDS entries after it
        main = got["f"] if got["f"] is not None else got["out"]
        if f_plain is None:
            f_plain = main
        else:
            assert np.array_equal(main, f_plain), f"{name} {call}: F / u_out changes when {request} is stored as well"
        for other, (oenv, keys) in OTHERS.items():
            _set(monkeypatch, dict(env, **oenv))
            ogot, oinfo = _run(case, f0, call, request)
            assert oinfo["tiled_kernel"] == (other != "cell")
            for key in keys:
                if got[key] is None:
                    continue
                same = np.array_equal(got[key], ogot[key])
                if not same:
                    print(f"{name} {call} +{request}: {key} differs from {other}: rel L-inf {rel_linf(got[key], ogot[key]):.3e}")
                assert same, f"{name} {call} +{request}: {key} is not {other}'s bit for bit"
