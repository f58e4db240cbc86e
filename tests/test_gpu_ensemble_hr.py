"""GPU: ensembles under hydrostatic reconstruction (rdyhip_ens_hr_enable, ensemble_hr_kernel in csrc/ensemble_kernels.h) against
the C oracle created with hydrostatic reconstruction, one oracle per member.

The members are those of tests/test_ensemble_hr_cpu.py, which checks without a device that each has a finite F and no near tie at
its largest Courant number: random states with dry cells, cells around tiny_h, films and deep water over the random triangle (126
cells) and mixed (80) meshes of test_gpu_tracers_hr.py, the 44 quads of planar_dam_10x5.msh over a bed of their own with
h_anuga = 1e-3, one rank's part of a random partition (972 owned cells of 1 043, ghosts interleaved), 8 192 triangles with a member
count that the group count does not divide, and 38 448 quads and triangles with 50 members, where a thread walks eight of them.
RDYHIP_KERNEL=cell cannot create an HR operator and the ensemble kernels do not depend on the variable: it is taken out for the
whole file (_operators_of_the_tiled_kind).

Bars, the ensemble suite's own: 1e-10 (helpers.rel_linf) for F, the boundary fluxes and trajectories, 1e-12 for the Courant number,
exact ids, bits for the Euler step, for a member among others, for the two halves of the diagnostics and for the undisturbed SWE
path; 1e-10 max(1, scale) for a lake at rest."""
import dataclasses

import numpy as np
import pytest

from helpers import oracle_from_case, rel_linf
from rdycore_amd import _lib
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import (Operator, RDyFlowConfig, RDyHipError, SOURCE_IMPLICIT_XQ2018, SOURCE_SEMI_IMPLICIT, WELL_BALANCING_HR,
                                  WELL_BALANCING_NONE)
from rdycore_amd.timestep import EnsembleEulerStepper
from test_ensemble_hr_cpu import LAKE_LEVELS, MESHES, SOURCES, hr_ensemble_mesh, lakes, members
from test_gpu_ensemble import _check_euler_sample, _groups, _set_member
from test_gpu_tracers import _bits, _dev, _empty_mesh, _torch
from test_gpu_tracers_hr import _levee

pytestmark = pytest.mark.gpu

TOL = 1e-10
SENT = -777.0


@pytest.fixture(autouse=True)
def _operators_of_the_tiled_kind(rdyhip_kernel, monkeypatch):
    """The suite's autouse fixture runs every GPU test once with RDYHIP_KERNEL=tiled and once with =cell, and an operator with
    hydrostatic reconstruction cannot be created under the latter.  The ensemble kernels do not depend on the variable: it is taken
    out (after that fixture has set it: hence the argument), as test_gpu_tracers_hr.py does."""
    monkeypatch.delenv("RDYHIP_KERNEL", raising=False)


def _full(shape, value):
    return _torch().full(shape, value, dtype=_torch().float64, device="cuda")


def _operator(mem):
    """an HR operator on the members' mesh with none of its own inputs set, the HR ensemble enabled and every member's inputs set"""
    case0 = mem[0][0]
    assert case0.config.well_balancing == WELL_BALANCING_HR
    op = Operator.create(case0.config, case0.mesh, case0.condition_types)
    assert op.ensemble_well_balancing() == WELL_BALANCING_NONE
    op.enable_ensemble(len(mem), well_balancing=WELL_BALANCING_HR)
    assert op.ensemble_info() == len(mem) and op.ensemble_well_balancing() == WELL_BALANCING_HR
    for m, (case, _, _, _) in enumerate(mem):
        assert case.condition_types == case0.condition_types
        _set_member(op, m, case)
    return op


def _evaluate(op, mem):
    """one evaluation of all members into a buffer pre-filled with NaN: (device state, F on the host)"""
    mesh = mem[0][0].mesh
    u = _dev(np.stack([c.u_local for c, _, _, _ in mem]))
    f = _full((len(mem), mesh.num_owned_cells, 3), float("nan"))           # every owned row of every member is written
    op.ensemble_rhs_function([c.dt for c, _, _, _ in mem], u, f)
    _torch().cuda.synchronize()
    return u, f.cpu().numpy()


def _diag_bits(d):
    return (int(_bits(np.array([d.max_courant_num]))[0]), int(d.global_edge_id), int(d.global_cell_id))


# ---- parity ------------------------------------------------------------------------------------------------------------------------
def _check_parity(name, src, B, euler=False):
    mem = members(name, src, B)
    mesh = mem[0][0].mesh
    op = _operator(mem)
    u, got = _evaluate(op, mem)
    assert np.isfinite(got).all()
    op.ensemble_update_diagnostics()
    diags = op.ensemble_get_diagnostics()
    assert len(diags) == B
    for m, (case, F, bf, (cmax, edge, cell)) in enumerate(mem):
        err = rel_linf(got[m], F)
        print(f"{name} src={src} B={B} member {m}: F {err:.3e}")
        assert err <= TOL, (m, err)
        if name == "part-o2l":          # F only: boundary fluxes behind ghosts and the ghost edges' Courant numbers are stated differences
            continue
        for b in range(len(mesh.boundaries)):
            have, want = op.ensemble_boundary_fluxes(m, b), bf[b]
            ok = np.isfinite(want).all(axis=1)          # an edge dry on both sides: 0 / 0 in the reference's flux, which it then discards
            assert rel_linf(have[ok], want[ok]) <= TOL, (m, b)
        d = diags[m]
        assert abs(d.max_courant_num - cmax) <= 1e-12 * max(1.0, cmax), (m, d.max_courant_num, cmax)
        assert (d.global_edge_id, d.global_cell_id) == (edge, cell), (m, d, edge, cell)
    if euler:
        _check_euler_sample(op, mem, u, got)
    op.destroy()


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("B", [1, 3, 7])
@pytest.mark.parametrize("name", MESHES)
def test_rhs_boundary_fluxes_and_courant_of_every_member(name, B, src):
    _check_parity(name, src, B)


@pytest.mark.parametrize("src", SOURCES)
def test_sixty_four_members_under_one_workgroup(src):
    assert hr_ensemble_mesh("tri-hr").num_owned_cells == 126
    _check_parity("tri-hr", src, 64)


def test_a_member_count_the_group_count_does_not_divide():
    """33 members on 32 workgroups of cells: the existing rule makes 17 groups of two, the last holding one; with the Euler step"""
    groups, per = _groups(33, 8192)
    assert (groups, per) == (17, 2) and 33 - (groups - 1) * per == 1
    _check_parity("tri-8192", SOURCE_SEMI_IMPLICIT, 33, euler=True)


def test_eight_members_per_thread_on_quads_and_triangles():
    """50 members on a mixed mesh of 38 448 cells (quads, and triangles with an empty fourth slot), XQ2018: six groups walk eight
    members and the seventh two"""
    groups, per = _groups(50, hr_ensemble_mesh("mixed-38k").num_owned_cells)
    assert (groups, per) == (7, 8) and 50 - (groups - 1) * per == 2
    _check_parity("mixed-38k", SOURCE_IMPLICIT_XQ2018, 50, euler=True)


# ---- the Euler step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,src", [("tri-hr", 3, SOURCE_SEMI_IMPLICIT), ("part-o2l", 3, SOURCE_IMPLICIT_XQ2018), ("mixed-hr", 7, SOURCE_SEMI_IMPLICIT)])
def test_euler_step_is_one_fused_multiply_add_of_the_rhs(name, B, src):
    from fractions import Fraction
    torch = _torch()
    mem = members(name, src, B)
    mesh = mem[0][0].mesh
    op = _operator(mem)
    u = np.stack([c.u_local for c, _, _, _ in mem])
    dts = [c.dt for c, _, _, _ in mem]
    ud, Fd = _evaluate(op, mem)
    assert np.isfinite(Fd).all()
    own = np.asarray(mesh.cell_owned_to_local)
    want = np.array([[[float(Fraction(dts[m]) * Fraction(float(Fd[m, o, k])) + Fraction(float(u[m, c, k]))) for k in range(3)]
                      for o, c in enumerate(own)] for m in range(B)])
    ghost = np.setdiff1d(np.arange(mesh.num_cells), own)
    assert (ghost.size > 0) == (name == "part-o2l")
    for with_f in (True, False):
        out = _full((B, mesh.num_cells, 3), SENT)
        f2 = _full((B, mesh.num_owned_cells, 3), float("nan")) if with_f else None
        op.ensemble_euler_step(dts, ud, out, f2)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(_bits(o[:, own]), _bits(want))
        assert (o[:, ghost] == SENT).all()                                      # ghost rows are left alone
        if with_f:
            assert np.array_equal(_bits(f2.cpu().numpy()), _bits(Fd))
    assert np.array_equal(_bits(ud.cpu().numpy()), _bits(u))                    # not in place
    op.destroy()


# ---- a member among others -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,src", [("tri-hr", SOURCE_SEMI_IMPLICIT), ("quad-44", SOURCE_IMPLICIT_XQ2018)])
def test_a_member_does_not_feel_the_others(name, src):
    """the same inputs as member 0 of B = 1 and as member 5 of B = 7: F, boundary fluxes and the Courant struct are the same bits"""
    seven = members(name, src, 7)
    mesh = seven[0][0].mesh
    res = []
    for mem, m in (([seven[5]], 0), (seven, 5)):
        op = _operator(mem)
        _, got = _evaluate(op, mem)
        op.ensemble_update_diagnostics()
        res.append((got[m], [op.ensemble_boundary_fluxes(m, b) for b in range(len(mesh.boundaries))], _diag_bits(op.ensemble_get_diagnostics()[m])))
        op.destroy()
    a, b = res
    assert np.isfinite(a[0]).all() and np.array_equal(_bits(a[0]), _bits(b[0]))
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(_bits(x), _bits(y))
    assert a[2] == b[2] and a[2][1] >= 0


# ---- lakes at rest -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("name", ["tri", "mixed"])
def test_every_members_lake_stays_at_rest(name, src):
    """four members at four water levels over one partly dry bed (50 / 19 / 4 / 0 dry cells of 60, 79 / 40 / 10 / 0 of 112), zero
    momentum, reflecting boundaries, no sources: every member's F vanishes to rounding.  test_ensemble_hr_cpu.py shows that the HR
    oracle is at rest there and the plain one is not.  No id check: such states tie by construction."""
    torch = _torch()
    mesh, u, scales = lakes(name)
    B = len(LAKE_LEVELS)
    op = Operator.create(RDyFlowConfig(source_method=src, well_balancing=WELL_BALANCING_HR), mesh, [M.CONDITION_REFLECTING] * len(mesh.boundaries))
    op.enable_ensemble(B, well_balancing=WELL_BALANCING_HR)
    f = _full((B, mesh.num_owned_cells, 3), float("nan"))
    op.ensemble_rhs_function([0.1] * B, _dev(u), f)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    assert np.isfinite(got).all()
    for m in range(B):
        err = np.abs(got[m]).max()
        print(f"{name} src={src} level {LAKE_LEVELS[m]}: max |F| on the device {err:.3e} (scale {scales[m]:.3g})")
        assert err <= 1e-10 * max(1.0, scales[m]), m
    op.destroy()


# ---- the levee deck in miniature -----------------------------------------------------------------------------------------------------------
def test_levee_trajectories_of_three_members():
    """the reference's HR deck (506 triangles), the water raised by 0.5 m in the wet cells left of the median wet x as in
    test_levee_trajectory_with_two_sediment_classes; three members with Manning's n 0.033 / 0.05 / 0.02 and uniform rain of
    0 / 1e-4 / 5e-4 m/s: 40 steps of 0.1 s through EnsembleEulerStepper against one Euler loop of the HR oracle per member"""
    torch = _torch()
    case, u5 = _levee()
    mesh = case.mesh
    no = mesh.num_owned_cells
    u0 = np.ascontiguousarray(u5[:, :3])
    wet = u0[:, 0] > 0.0
    x = mesh.cell_centroids[:, 0]
    u0[wet & (x < np.median(x[wet])), 0] += 0.5
    mann, rain, dt, nsteps = (0.033, 0.05, 0.02), (0.0, 1e-4, 5e-4), 0.1, 40
    want, cmax = [], 0.0
    for n, r in zip(mann, rain):
        src = np.zeros((no, 3))
        src[:, 0] = r
        orc = oracle_from_case(dataclasses.replace(case, mannings=np.full(no, n), ext_src=src))
        u = u0.copy()
        for _ in range(nsteps):
            u = u + dt * orc.apply(dt, u)
            cmax = max(cmax, orc.diagnostics()[0])
        orc.close()
        want.append(u)
    newly = int(((want[0][:, 0] > 0.0) & ~(u0[:, 0] > 0.0)).sum())
    assert np.isfinite(want).all() and 0.0 < cmax < 1.0 and newly > 0
    assert min(rel_linf(want[a], want[b]) for a, b in ((0, 1), (0, 2), (1, 2))) > 1e-6          # a kernel that mixes the members up cannot pass
    op = CS.create_operator(case)                        # member 0 keeps the operator's own inputs
    op.enable_ensemble(3, well_balancing=WELL_BALANCING_HR)
    for m in (1, 2):
        op.ensemble_set_mannings_n(m, np.full(no, mann[m]))
        op.ensemble_set_external_source(m, 0, np.full(no, rain[m]))
    st = EnsembleEulerStepper(op)
    got = st.advance(_dev(np.stack([u0] * 3)), [dt] * 3, nsteps)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert st.step == nsteps and np.isfinite(got).all()
    for m in range(3):
        err = rel_linf(got[m], want[m])
        print(f"levee member {m} (n = {mann[m]}, rain {rain[m]}): 40 steps, state vs oracle {err:.3e}; max Courant {cmax:.3f}, {newly} cells newly wet")
        assert err <= TOL, m
    op.destroy()


# ---- diagnostics in two halves ---------------------------------------------------------------------------------------------------------------
def test_diagnostics_begin_and_wait_give_the_structs_of_the_blocking_call():
    mem = members("mixed-hr", SOURCE_SEMI_IMPLICIT, 7)
    op = _operator(mem)
    _evaluate(op, mem)
    op.ensemble_diagnostics_begin()
    op.ensemble_diagnostics_wait()
    got = [_diag_bits(d) for d in op.ensemble_get_diagnostics()]
    op.ensemble_update_diagnostics()
    want = [_diag_bits(d) for d in op.ensemble_get_diagnostics()]
    assert got == want and len(want) == 7 and len(set(want)) == 7
    for (_, _, _, (cmax, edge, cell)), w, d in zip(mem, want, op.ensemble_get_diagnostics()):
        assert abs(d.max_courant_num - cmax) <= 1e-12 * max(1.0, cmax) and w[1:] == (edge, cell)
    op.destroy()


# ---- the SWE path ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed-hr", "part-o2l"])
def test_the_swe_path_is_undisturbed(name):
    """After enable_ensemble(..., well_balancing=HR) and an ensemble evaluation, rdyhip_rhs_function on the same HR operator gives
    the bits of a fresh HR operator: F, primitive variables, boundary fluxes and the Courant struct."""
    torch = _torch()
    mem = members(name, SOURCE_SEMI_IMPLICIT, 3)
    case = mem[0][0]
    mesh = case.mesh
    plain = CS.create_operator(case)
    op = CS.create_operator(case)
    op.enable_ensemble(3, well_balancing=WELL_BALANCING_HR)
    for m, (c, _, _, _) in enumerate(mem):
        _set_member(op, m, c)
    _evaluate(op, mem)
    u3 = _dev(case.u_local)
    res = []
    for o in (plain, op):
        pv = o.primitive_variables
        f = _full((mesh.num_owned_cells, 3), float("nan"))
        o.rhs_function(case.dt, u3, f)
        torch.cuda.synchronize()
        o.update_diagnostics()
        res.append(([_bits(f.cpu().numpy()), _bits(pv.cpu().numpy())] + [_bits(o.boundary_fluxes(b)) for b in range(len(mesh.boundaries))] +
                    [_bits(o.boundary_fluxes(b, accumulated=True)) for b in range(len(mesh.boundaries))], _diag_bits(o.get_diagnostics())))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    assert np.isfinite(res[0][0][0].view(np.float64)).all() and res[0][1] == res[1][1] and res[0][1][1] >= 0
    assert rel_linf(res[1][0][0].view(np.float64), mem[0][1]) <= TOL              # ... which is the oracle's F of member 0
    plain.destroy()
    op.destroy()


# ---- refusals, info, a rank that owns nothing --------------------------------------------------------------------------------------------------
def test_refusals_and_info():
    _torch()
    mesh = hr_ensemble_mesh("tri-hr")

    def refused(op, n, text, wb=WELL_BALANCING_HR, members_now=0, wb_now=WELL_BALANCING_NONE):
        before = op.layout_info()["device_bytes"]
        with pytest.raises(RDyHipError) as e:
            op.enable_ensemble(n, well_balancing=wb)
        assert e.value.code == 83 and text in e.value.message, e.value.message
        assert op.ensemble_info() == members_now and op.ensemble_well_balancing() == wb_now
        assert op.layout_info()["device_bytes"] == before                 # nothing was allocated
    # a plain operator and a second-order one
    for cfg, text in ((RDyFlowConfig(), "RDYHIP_WELL_BALANCING_HR"), (RDyFlowConfig(second_order=True), "second_order")):
        op = Operator.create(cfg, mesh)
        refused(op, 2, text)
        op.destroy()
    # a plain ensemble reports NONE, and the HR enable on it is a second enable
    op = Operator.create(RDyFlowConfig(), mesh)
    assert op.ensemble_well_balancing() == WELL_BALANCING_NONE
    op.enable_ensemble(2)
    assert op.ensemble_info() == 2 and op.ensemble_well_balancing() == WELL_BALANCING_NONE
    refused(op, 2, "already", members_now=2)
    op.destroy()
    # an HR operator: num_members outside 1..64, a value that is no well-balancing method, the plain enable
    op = Operator.create(RDyFlowConfig(well_balancing=WELL_BALANCING_HR), mesh)
    for n in (0, 65, -1):
        refused(op, n, "num_members")
    with pytest.raises(ValueError):
        op.enable_ensemble(2, well_balancing=7)
    assert op.ensemble_info() == 0
    refused(op, 2, "rdyhip_ens_hr_enable", wb=WELL_BALANCING_NONE)
    # the enable itself: the plain enable's allocations, counted the same way, then a second enable of either kind
    before = op.layout_info()["device_bytes"]
    op.enable_ensemble(3, well_balancing=WELL_BALANCING_HR)
    no, K = mesh.num_owned_cells, sum(b.num_edges for b in mesh.boundaries)
    W = 4 * ((no + 255) // 256)
    assert op.layout_info()["device_bytes"] == before + 3 * (32 * no + 48 * K + 12 * W + 16)
    assert op.ensemble_info() == 3 and op.ensemble_well_balancing() == WELL_BALANCING_HR
    for wb in (WELL_BALANCING_HR, WELL_BALANCING_NONE):
        refused(op, 3, "already", wb=wb, members_now=3, wb_now=WELL_BALANCING_HR)
    op.destroy()
    lib = _lib.load()
    assert lib.rdyhip_ens_hr_enable(None, 2) == 83 and b"null operator" in lib.rdyhip_last_error()


def test_a_rank_that_owns_nothing():
    torch = _torch()
    mesh = _empty_mesh()
    op = Operator.create(RDyFlowConfig(well_balancing=WELL_BALANCING_HR), mesh)
    op.enable_ensemble(3, well_balancing=WELL_BALANCING_HR)
    assert op.ensemble_well_balancing() == WELL_BALANCING_HR
    u = torch.zeros((3, mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    f = torch.empty((3, 0, 3), dtype=torch.float64, device="cuda")
    op.ensemble_rhs_function([0.1, 0.2, 0.3], u, f)
    out = torch.full_like(u, 5.0)
    op.ensemble_euler_step([0.1, 0.2, 0.3], u, out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5.0).all()
    op.ensemble_update_diagnostics()
    ds = op.ensemble_get_diagnostics()
    assert [(d.max_courant_num, d.global_edge_id, d.global_cell_id) for d in ds] == [(0.0, -1, -1)] * 3
    op.destroy()
