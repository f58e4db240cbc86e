"""Primitive variables on demand: the RHS kernels store (h, u, v) only once somebody has asked for them
(KernelArgs::pv, include/rdyhip.h at rdyhip_field_ptr); the first request after evaluations that did not store fills the array
from the input state of the most recent one (primitive_variables_kernel), and rdyhip_field_release turns the stores off again.

Meshes of a few thousand cells (test_gpu_kernel_matrix.matrix_mesh) cut into 64-cell tiles on a persistent grid of 8
workgroups: every workgroup walks several tiles, the last tile is partial, and on the o2l mesh the owned index is not the local
one -- the smallest shapes at which a wrong row, a wrong phase subset or a missed tile shows.  random_case states hold dry cells
and cells around tiny_h (the HR kernels' h == tiny_h correction feeds the stored values).
Tolerance against the oracle: the bar of test_gpu_parity.py (rel L-inf <= 1e-10 against max(1, |ref|)); between an operator that
stores from the start and one that fills on request the bar is bit for bit."""
import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd.operator import RDyFlowConfig

from helpers import oracle_from_case, rel_linf
from random_cases import random_case
from test_gpu_kernel_matrix import matrix_mesh
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

MESHES = [("tri", "prefix"), ("quad", "prefix"), ("tri", "o2l")]
_WALK_ENV = {"RDYHIP_TILE_CELLS": "64", "RDYHIP_PGRID": "8"}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _walk_env(monkeypatch, kernel=None):
    for k in ("RDYHIP_PGRID", "RDYHIP_XCD_SWIZZLE", "RDYHIP_BALANCE_ROUNDS", "RDYHIP_INTERIOR_SHRINK", "RDYHIP_TILE_CELLS",
              "RDYHIP_UOUT_CACHED", "RDYHIP_BLOCKS_PER_CU", "RDYHIP_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in _WALK_ENV.items():
        monkeypatch.setenv(k, v)
    if kernel:
        monkeypatch.setenv("RDYHIP_KERNEL", kernel)


def _case(kind, layout, hr, seed, second_order=False):
    rng = np.random.default_rng(seed)
    mesh = matrix_mesh(kind, layout, hr)
    cfg = RDyFlowConfig(tiny_h=1e-5, source_method=int(rng.integers(0, 2)), well_balancing=2 if hr else 0, second_order=second_order)
    case = random_case(rng, mesh, cfg, region_block=64)
    case.dt = 1e-2
    # a few cells at h == tiny_h exactly, moving: where the HR kernels' staged velocities and the stored ones follow different rules
    ids = rng.permutation(mesh.num_cells)[:16]
    case.u_local[ids, 0] = cfg.tiny_h
    case.u_local[ids, 1:] = rng.normal(size=(16, 2)) * 1e-6
    return rng, case


def _dev(a):
    return _torch().tensor(a, dtype=_torch().float64, device="cuda")


def _oracle_pv(orc, case, u_local):
    orc.apply(case.dt, u_local)
    return orc.primitive_variables.copy()


def _three_calls(op, case, u, f0):
    """rhs_function, the accumulate form and euler_step: (F, F accumulated, u_out, F of the step, Courant number of the step)"""
    torch = _torch()
    no, dt = case.mesh.num_owned_cells, case.dt
    f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
    op.rhs_function(dt, u, f)
    fa = _dev(f0)
    op.reset_diagnostics()
    op.apply(dt, u, fa)
    out = torch.full_like(u, -7.0)
    fe = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
    op.euler_step(dt, u, out, fe)
    op.update_diagnostics()
    return f, fa, out, fe, op.get_diagnostics().max_courant_num


def _modes_agree(case, rng, what):
    """operator A takes the pointer before its first evaluation, operator B after its last"""
    torch = _torch()
    mesh, no = case.mesh, case.mesh.num_owned_cells
    f0 = rng.normal(size=(no, 3)) * np.array([0.1, 1.0, 1.0])
    u = _dev(case.u_local)
    a, b = CS.create_operator(case), CS.create_operator(case)
    assert not a.primitive_variables_stored() and not b.primitive_variables_stored()
    pv_a = a.primitive_variables
    assert a.primitive_variables_stored() and not b.primitive_variables_stored()
    res_a = _three_calls(a, case, u, f0)
    res_b = _three_calls(b, case, u, f0)
    assert a.primitive_variables_stored() and not b.primitive_variables_stored()
    pv_b = b.primitive_variables
    assert b.primitive_variables_stored()
    torch.cuda.synchronize()
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local).copy()
    pvr = orc.primitive_variables.copy()
    for name, got in (("stored", pv_a), ("filled on request", pv_b)):
        err = rel_linf(got.cpu().numpy(), pvr)
        print(f"{what}: pv, {name}: rel L-inf {err:.3e}")
        assert err <= TOL, f"{what}: pv, {name}: rel L-inf {err:.3e}"
    assert torch.equal(pv_a, pv_b), f"{what}: the stored and the filled primitive variables differ"
    err = rel_linf(res_b[0].cpu().numpy(), fr)
    print(f"{what}: F without the store: rel L-inf {err:.3e}")
    assert err <= TOL
    for name, x, y in zip(("F", "F accumulated", "u_out", "F of the Euler step"), res_a, res_b):
        assert torch.equal(x, y), f"{what}: {name} differs between the two modes"
    assert res_a[4] == res_b[4] > 0.0, f"{what}: Courant number {res_a[4]} / {res_b[4]}"
    assert torch.all(res_b[2][torch.as_tensor(mesh.cell_is_owned == 0, device="cuda")] == -7.0), "ghost rows of u_out were written"
    a.destroy()
    b.destroy()


@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
@pytest.mark.parametrize("kind,layout", MESHES, ids=[f"{k}-{l}" for k, l in MESHES])
def test_modes_agree(kind, layout, hr, monkeypatch):
    _torch()
    _walk_env(monkeypatch)
    rng, case = _case(kind, layout, hr, 8100 + 10 * MESHES.index((kind, layout)) + int(hr))
    op = CS.create_operator(case)
    info = op.layout_info()
    op.destroy()
    assert info["tiled_kernel"] and info["persistent_grid"] == 8 and info["num_tiles"] >= 24     # several tiles per workgroup
    assert info["owned_is_prefix"] == (layout == "prefix")
    _modes_agree(case, rng, f"{kind}-{layout}-{'hr' if hr else 'plain'}")


@pytest.mark.parametrize("which", ["second_order", "cell"])
def test_modes_agree_for_the_other_kernels(which, monkeypatch):
    _torch()
    _walk_env(monkeypatch, kernel="cell" if which == "cell" else None)
    rng, case = _case("tri", "prefix", False, 8200 + (which == "cell"), second_order=which == "second_order")
    op = CS.create_operator(case)
    info = op.layout_info()
    op.destroy()
    assert info["tiled_kernel"] == (which != "cell") and info["second_order_fused"] == (which == "second_order")
    _modes_agree(case, rng, which)


def test_first_request_before_any_evaluation_returns_zeros_and_turns_storing_on(monkeypatch):
    torch = _torch()
    _walk_env(monkeypatch)
    rng, case = _case("tri", "o2l", False, 8300)
    op = CS.create_operator(case)
    assert not op.primitive_variables_stored()
    pv = op.primitive_variables
    assert op.primitive_variables_stored()
    assert pv.shape == (case.mesh.num_owned_cells, 3) and torch.all(pv == 0.0)
    u = _dev(case.u_local)
    f = torch.empty((case.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.rhs_function(case.dt, u, f)
    torch.cuda.synchronize()
    assert rel_linf(pv.cpu().numpy(), _oracle_pv(oracle_from_case(case), case, case.u_local)) <= TOL
    op.destroy()


@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
def test_the_last_evaluation_wins(hr, monkeypatch):
    torch = _torch()
    _walk_env(monkeypatch)
    rng, case = _case("tri", "o2l", hr, 8400 + int(hr))
    mesh, no = case.mesh, case.mesh.num_owned_cells
    # three states: the case's, and the same rows dealt to other cells (dry cells and cells around tiny_h stay in the mix)
    states = [case.u_local, case.u_local[rng.permutation(mesh.num_cells)], case.u_local[rng.permutation(mesh.num_cells)]]
    orc = oracle_from_case(case)
    refs = [_oracle_pv(orc, case, np.ascontiguousarray(s)) for s in states]
    assert rel_linf(refs[0], refs[1]) > 1e-3 and rel_linf(refs[1], refs[2]) > 1e-3
    u1, u2, u3 = (_dev(np.ascontiguousarray(s)) for s in states)
    a, b = CS.create_operator(case), CS.create_operator(case)
    pv_a = a.primitive_variables
    f = torch.empty((no, 3), dtype=torch.float64, device="cuda")
    for op in (a, b):
        op.rhs_function(case.dt, u1, f)
        op.rhs_function(case.dt, u2, f)
    assert not b.primitive_variables_stored()
    pv_b = b.primitive_variables
    torch.cuda.synchronize()
    err = rel_linf(pv_b.cpu().numpy(), refs[1])
    print(f"pv of the second state: rel L-inf {err:.3e}")
    assert err <= TOL
    assert torch.equal(pv_a, pv_b)
    # from here on the tensor obtained above is written by every evaluation, with no new request
    b.rhs_function(case.dt, u3, f)
    torch.cuda.synchronize()
    err = rel_linf(pv_b.cpu().numpy(), refs[2])
    print(f"pv of the third state, through the tensor obtained earlier: rel L-inf {err:.3e}")
    assert err <= TOL
    a.rhs_function(case.dt, u3, f)
    torch.cuda.synchronize()
    assert torch.equal(pv_a, pv_b)
    a.destroy()
    b.destroy()


@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
def test_euler_step_in_two_phases_then_the_request_fills_every_owned_row_from_the_input_state(hr, monkeypatch):
    torch = _torch()
    _walk_env(monkeypatch)
    rng, case = _case("tri", "o2l", hr, 8500 + int(hr))
    mesh = case.mesh
    assert 0 < mesh.num_owned_cells < mesh.num_cells
    u = _dev(case.u_local)
    ghost = torch.as_tensor(mesh.cell_is_owned == 0, device="cuda")
    a, b = CS.create_operator(case), CS.create_operator(case)
    info = b.layout_info()
    assert 0 < info["num_halo_tiles"] < info["num_tiles"]                 # both phases have tiles
    pv_a = a.primitive_variables
    outs = []
    for op in (a, b):
        out = torch.full_like(u, -7.0)
        op.reset_boundary_fluxes_accum()
        op.euler_step(case.dt, u, out, None, phase=1)
        op.euler_step(case.dt, u, out, None, phase=2, reset_diagnostics=False)
        outs.append(out)
    assert not b.primitive_variables_stored()
    pv_b = b.primitive_variables
    torch.cuda.synchronize()
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local).copy()
    err = rel_linf(pv_b.cpu().numpy(), orc.primitive_variables)
    print(f"pv after a two-phase Euler step: rel L-inf {err:.3e}")
    assert err <= TOL                                                     # the INPUT state's, all owned rows
    assert torch.equal(pv_a, pv_b)
    assert torch.equal(outs[0], outs[1])
    assert torch.all(outs[1][ghost] == -7.0), "ghost rows of u_out were written"
    own = mesh.cell_owned_to_local
    assert rel_linf(outs[1].cpu().numpy()[own], case.u_local[own] + case.dt * fr) <= TOL
    a.destroy()
    b.destroy()


@pytest.mark.parametrize("kind,layout,hr", [("tri", "o2l", False), ("quad", "prefix", True)], ids=["tri-o2l-plain", "quad-prefix-hr"])
def test_release_stops_the_stores_and_the_next_request_fills(kind, layout, hr, monkeypatch):
    torch = _torch()
    _walk_env(monkeypatch)
    rng, case = _case(kind, layout, hr, 8600 + int(hr))
    mesh, no = case.mesh, case.mesh.num_owned_cells
    u2_host = np.ascontiguousarray(case.u_local[rng.permutation(mesh.num_cells)])
    orc = oracle_from_case(case)
    ref1, ref2 = _oracle_pv(orc, case, case.u_local), _oracle_pv(orc, case, u2_host)
    assert rel_linf(ref1, ref2) > 1e-3
    u1, u2 = _dev(case.u_local), _dev(u2_host)
    f = torch.empty((no, 3), dtype=torch.float64, device="cuda")
    op = CS.create_operator(case)
    pv = op.primitive_variables
    op.rhs_function(case.dt, u1, f)
    torch.cuda.synchronize()
    assert rel_linf(pv.cpu().numpy(), ref1) <= TOL
    op.release_primitive_variables()
    assert not op.primitive_variables_stored()
    pv.fill_(-7.0)
    f_stored = f.clone()
    op.rhs_function(case.dt, u2, f)
    out = torch.full_like(u2, -7.0)
    op.euler_step(case.dt, u2, out, None)
    torch.cuda.synchronize()
    assert torch.all(pv == -7.0), "a launch stored primitive variables after the release"
    assert not torch.equal(f, f_stored)                                   # (the evaluation itself did run)
    again = op.primitive_variables
    assert op.primitive_variables_stored() and again.data_ptr() == pv.data_ptr()
    torch.cuda.synchronize()
    err = rel_linf(pv.cpu().numpy(), ref2)
    print(f"pv after release and a new request: rel L-inf {err:.3e}")
    assert err <= TOL
    op.destroy()


def test_the_python_operator_keeps_the_state_of_the_last_evaluation_alive(monkeypatch):
    """a caller that drops its state tensor right after the call (tests/test_gpu_golden_and_scale.py's gpu_rhs does): the
    Operator holds it, so the allocator cannot hand the memory to the next tensor before the request has read it"""
    torch = _torch()
    _walk_env(monkeypatch)
    rng, case = _case("tri", "o2l", False, 8700)
    op = CS.create_operator(case)

    def evaluate():
        u = _dev(case.u_local)
        f = torch.empty((case.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
        op.rhs_function(case.dt, u, f)
        torch.cuda.synchronize()
        return u.data_ptr()

    ptr = evaluate()
    junk = [torch.full((case.mesh.num_cells, 3), 123.0, dtype=torch.float64, device="cuda") for _ in range(4)]
    assert all(j.data_ptr() != ptr for j in junk)
    pv = op.primitive_variables
    torch.cuda.synchronize()
    assert rel_linf(pv.cpu().numpy(), _oracle_pv(oracle_from_case(case), case, case.u_local)) <= TOL
    op.destroy()


def test_rank_that_owns_nothing():
    torch = _torch()
    from rdycore_amd import mesh as M
    from rdycore_amd.operator import Operator
    xyz, conn, _, _ = M.structured_tri_connectivity(3, 2)
    mesh = M.build_mesh(xyz, conn, is_owned=np.zeros(conn.shape[0], dtype=np.int32), boundary_classifier=M.box_side_boundaries(0, 3, 0, 2))
    assert mesh.num_owned_cells == 0
    op = Operator.create(RDyFlowConfig(), mesh)
    u = torch.ones((mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    f = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    op.rhs_function(0.1, u, f)
    assert not op.primitive_variables_stored()
    assert op.primitive_variables.shape == (0, 3)
    assert op.primitive_variables_stored()
    op.release_primitive_variables()
    assert not op.primitive_variables_stored()
    op.rhs_function(0.1, u, f)
    assert op.primitive_variables.shape == (0, 3)
    torch.cuda.synchronize()
    op.destroy()
