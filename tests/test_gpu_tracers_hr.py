"""GPU: tracers under hydrostatic reconstruction (rdyhip_tracer_hr_enable, tracer_hr_kernel in csrc/tracer_kernels.h) against
tests/tracer_hr_reference.py, the numpy restatement that tests/test_tracers_hr_cpu.py ties to the C oracle created with
hydrostatic reconstruction, to a lake at rest and to a hand-derived answer.

Shapes: the random triangle (126 cells) and mixed (8 x 8 squares) meshes of the CPU file with cells at h == tiny_h exactly -- where
the HR operator's wet test and the plain one part --, the 44 quads of planar_dam_10x5.msh over a bed of their own with
h_anuga = 1e-3 (the two rule sets differ in every cell), one rank's part of a random partition (about 1 000 owned cells, ghosts
interleaved), the two RCB parts of a 600-cell mesh, the reference's levee deck (506 triangles), and a rank that owns nothing.
RDYHIP_KERNEL=cell cannot create an HR operator, so no test here takes the rdyhip_kernel fixture or branches on it; the variable is
taken out for the whole file (_operators_of_the_tiled_kind).

Bars, the tracer suite's own: 1e-10 (helpers.rel_linf) for F, the primitive variables, the boundary fluxes and trajectories,
1e-12 for the Courant number, exact ids, bits for the Euler step, the phases and the undisturbed SWE path."""
import dataclasses
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

import houston
import random_cases as RC
import tracer_hr_reference as THR
import tracer_parts as TP
import tracer_reference as TR
from helpers import rel_linf
from rdycore_amd import _lib
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import (Operator, PHASE_ALL, PHASE_HALO, PHASE_INTERIOR, RDyFlowConfig, RDyHipError, SOURCE_IMPLICIT_XQ2018,
                                  TRACER_FORM_PRIMITIVE, TRACER_RIEMANN_ROE, TRACER_RIEMANN_UPWIND_ROE, WELL_BALANCING_HR, WELL_BALANCING_NONE)
from rdycore_amd.timestep import TracerEulerStepper
from test_gpu_tracers import _bathymetry, _bits, _dev, _empty_mesh, _mesh, _torch
from test_tracers_hr_cpu import hr_tracer_case, lake_at_rest, lake_mesh

pytestmark = pytest.mark.gpu

TOL = 1e-10
SENT = -777.0
MESHES = ["tri-hr", "mixed-hr", "quad-44", "part-o2l"]
COMBOS = [(1, TRACER_RIEMANN_ROE), (2, TRACER_RIEMANN_UPWIND_ROE), (7, TRACER_RIEMANN_ROE), (7, TRACER_RIEMANN_UPWIND_ROE)]


@pytest.fixture(autouse=True)
def _operators_of_the_tiled_kind(rdyhip_kernel, monkeypatch):
    """The suite's autouse fixture runs every GPU test once with RDYHIP_KERNEL=tiled and once with =cell, and an operator with
    hydrostatic reconstruction cannot be created under the latter.  The tracer kernels do not depend on the variable: it is taken
    out (after that fixture has set it: hence the argument), so both runs create the operators HR has, as
    test_gpu_diagnostics_async.py does for second order."""
    monkeypatch.delenv("RDYHIP_KERNEL", raising=False)


@functools.lru_cache(maxsize=None)
def _hr_mesh(name):
    if name == "tri-hr":
        return RC.random_mesh(np.random.default_rng(2033), "tri", 9, 7)
    if name == "mixed-hr":
        return RC.random_mesh(np.random.default_rng(2032), "mixed", 8, 8)
    if name == "quad-44":      # the file has a flat bed: elevations of its own at the centroids (the shared mesh is left as it is)
        mesh = _mesh("quad-44")
        c = mesh.cell_centroids
        return dataclasses.replace(mesh, cell_zc=np.ascontiguousarray(_bathymetry(c[:, 0], c[:, 1])))
    return _mesh(name)


@functools.lru_cache(maxsize=None)
def _case(name, nt, riemann):
    """(case, HR reference with its results of ONE apply, state, F): computed once, shared, left unchanged"""
    rng = np.random.default_rng(3000 + 10 * nt + riemann + len(name))
    mesh = _hr_mesh(name)
    assert np.ptp(mesh.cell_zc) > 0.0
    case, ref, u = hr_tracer_case(rng, mesh, nt, riemann, h_anuga=1e-3 if name == "quad-44" else 0.0, region_block=16 if name == "mixed-hr" else 0)
    h = u[:, 0]
    assert (h == 0.0).any() and (h >= case.config.tiny_h).any()
    if name != "quad-44":
        assert (h == case.config.tiny_h).sum() >= 3
    F = ref.apply(case.dt, u)
    assert np.isfinite(F).all() and np.abs(F[:, 3:]).max() > 0.0
    assert ref.edges_with_flux > 0 and ref.edges_correction_only + ref.edges_skipped > 0
    for a in (u, F, ref.primitive_variables):
        a.setflags(write=False)
    return case, ref, u, F


def _arm(op, ref):
    """the HR tracer path of an operator created with hydrostatic reconstruction, with every input of the reference set"""
    op.enable_tracers(ref.nt, ref.riemann, well_balancing=WELL_BALANCING_HR)
    assert op.tracers_info() == (ref.nt, ref.riemann) and op.tracers_well_balancing() == WELL_BALANCING_HR
    for j in range(ref.nt):
        op.tracers_set_source(j, ref.tracer_sources[:, j])
    for b, bnd in enumerate(ref.mesh.boundaries):
        if bnd.num_edges:
            op.tracers_set_boundary_values(b, ref.boundary_values[b])
    return op


def _operator(case, ref):
    assert case.config.well_balancing == WELL_BALANCING_HR
    return _arm(CS.create_operator(case), ref)


def _full(shape, value):
    return _torch().full(shape, value, dtype=_torch().float64, device="cuda")


def _courant(op):
    op.update_diagnostics()
    d = op.get_diagnostics()
    return (int(_bits(np.array([d.max_courant_num]))[0]), int(d.global_edge_id), int(d.global_cell_id))


# ---- parity ------------------------------------------------------------------------------------------------------------------------
def _check_rhs(name, nt, riemann):
    """one evaluation of a case: F, the primitive variables, the boundary fluxes and the Courant struct against the HR reference"""
    torch = _torch()
    case, ref, u, F = _case(name, nt, riemann)
    mesh = case.mesh
    op = _operator(case, ref)
    pv = op.tracers_primitive_variables()
    f = _full((mesh.num_owned_cells, 3 + nt), float("nan"))           # every owned row is written
    op.tracers_rhs_function(case.dt, _dev(u), f)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    assert np.isfinite(got).all()
    err, perr = rel_linf(got, F), rel_linf(pv.cpu().numpy(), ref.primitive_variables)
    print(f"{name} nt={nt} riemann={riemann}: F {err:.3e}, pv {perr:.3e}; edges with flux / correction only / skipped / one side dry "
          f"{ref.edges_with_flux} / {ref.edges_correction_only} / {ref.edges_skipped} / {ref.edges_one_side_dry}")
    assert err <= TOL and perr <= TOL
    if name == "part-o2l":          # F and pv only: boundary fluxes behind ghosts and the ghost edges' Courant numbers are stated differences
        op.destroy()
        return
    for b, bnd in enumerate(mesh.boundaries):
        bf, want = op.tracers_boundary_fluxes(b), ref.boundary_fluxes[b]
        ok = np.isfinite(want).all(axis=1)          # an edge dry on both sides: 0 / 0 in the reference's flux, which it then discards
        assert rel_linf(bf[ok], want[ok]) <= TOL
    op.update_diagnostics()
    d = op.get_diagnostics()
    cmax, edge, cell = ref.courant
    assert cmax > 0.0 and abs(d.max_courant_num - cmax) <= 1e-12 * max(1.0, cmax)
    ec = np.sort(ref.edge_courant[np.isfinite(ref.edge_courant)])
    assert ec[-1] - ec[-2] > 1e-9 * ec[-1], "the state has a near tie: choose another seed"
    assert (d.global_edge_id, d.global_cell_id) == (int(mesh.edge_global_ids[edge]), int(mesh.cell_global_ids[cell]))
    op.destroy()


@pytest.mark.parametrize("nt,riemann", COMBOS)
@pytest.mark.parametrize("name", MESHES)
def test_rhs_primitive_variables_boundary_fluxes_and_courant(name, nt, riemann):
    _check_rhs(name, nt, riemann)


@pytest.mark.parametrize("riemann", [TRACER_RIEMANN_ROE, TRACER_RIEMANN_UPWIND_ROE])
@pytest.mark.parametrize("nt", range(1, 8))
@pytest.mark.parametrize("name", ["tri-hr", "quad-44"])
def test_every_instantiation_runs_on_the_device(name, nt, riemann):
    """tracer_hr_kernel<S, NT, UPWIND> for S = 3 (tri-hr) and 4 (quad-44), NT = 1..7 and both tracer Riemann solvers: each of the 28
    instantiations evaluated once, on the smallest meshes of this file, under the bars of the test above"""
    _check_rhs(name, nt, riemann)


# ---- a lake at rest ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "tri"])
def test_a_lake_at_rest_stays_at_rest_on_the_device(name):
    torch = _torch()
    mesh = lake_mesh(name)
    ref, _, u, scale = lake_at_rest(mesh)
    F = ref.apply(0.1, u)
    op = Operator.create(RDyFlowConfig(well_balancing=WELL_BALANCING_HR), mesh, ref.types)
    op.enable_tracers(2, well_balancing=WELL_BALANCING_HR)
    f = _full((mesh.num_owned_cells, 5), float("nan"))
    op.tracers_rhs_function(0.1, _dev(u), f)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    err = np.abs(got[:, :3]).max()
    print(f"{name}: max |F_flow| on the device {err:.3e} (scale {scale:.3g}), tracers vs reference {rel_linf(got[:, 3:], F[:, 3:]):.3e}")
    assert np.isfinite(got).all() and err <= 1e-10 * max(1.0, scale)
    assert rel_linf(got[:, 3:], F[:, 3:]) <= TOL
    op.destroy()


# ---- the Euler step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nt,riemann", [("tri-hr", 2, TRACER_RIEMANN_UPWIND_ROE), ("part-o2l", 7, TRACER_RIEMANN_ROE), ("quad-44", 1, TRACER_RIEMANN_ROE)])
def test_euler_step_is_one_fused_multiply_add_of_the_rhs(name, nt, riemann):
    torch = _torch()
    case, ref, u, _ = _case(name, nt, riemann)
    mesh, dt, n = case.mesh, case.dt, 3 + nt
    op = _operator(case, ref)
    ud = _dev(u)
    f = torch.empty((mesh.num_owned_cells, n), dtype=torch.float64, device="cuda")
    op.tracers_rhs_function(dt, ud, f)
    Fd = f.cpu().numpy()
    own = np.asarray(mesh.cell_owned_to_local)
    want = np.array([[float(Fraction(dt) * Fraction(float(Fd[o, k])) + Fraction(float(u[c, k]))) for k in range(n)] for o, c in enumerate(own)])
    ghost = np.setdiff1d(np.arange(mesh.num_cells), own)
    for with_f in (True, False):
        out = _full((mesh.num_cells, n), SENT)
        f2 = _full((mesh.num_owned_cells, n), float("nan")) if with_f else None
        op.tracers_euler_step(dt, ud, out, f2)                                  # f_global=None is accepted
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(_bits(o[own]), _bits(want))
        assert (o[ghost] == SENT).all()                                         # ghost rows are left alone
        if with_f:
            assert np.array_equal(_bits(f2.cpu().numpy()), _bits(Fd))
    assert np.array_equal(_bits(ud.cpu().numpy()), _bits(u))                    # not in place
    op.destroy()


# ---- phases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,riemann", [(2, TRACER_RIEMANN_UPWIND_ROE), (7, TRACER_RIEMANN_ROE)])
def test_interior_then_halo_is_the_whole_evaluation(nt, riemann):
    torch = _torch()
    case, ref, u, _ = _case("part-o2l", nt, riemann)
    mesh, dt, n = case.mesh, case.dt, 3 + nt
    halo = TP.ghost_adjacent(mesh)
    assert halo.any() and (~halo).any()
    op = _operator(case, ref)
    pv = op.tracers_primitive_variables()
    ud = _dev(u)

    def collect(f, out):
        torch.cuda.synchronize()
        return {"F": _bits(f.cpu().numpy()), "pv": _bits(pv.cpu().numpy()), "u_out": _bits(out.cpu().numpy()), "courant": _courant(op)}
    f, out = _full((mesh.num_owned_cells, n), float("nan")), _full((mesh.num_cells, n), SENT)
    op.tracers_euler_step_phase(PHASE_ALL, dt, ud, out, f, reset_diagnostics=True)
    whole = collect(f, out)
    assert np.isfinite(whole["F"].view(np.float64)).all() and whole["courant"][1] >= 0
    f, out = _full((mesh.num_owned_cells, n), float("nan")), _full((mesh.num_cells, n), SENT)
    pv.fill_(SENT)
    op.tracers_euler_step_phase(PHASE_INTERIOR, dt, ud, out, f, reset_diagnostics=True)
    torch.cuda.synchronize()
    assert (pv.cpu().numpy()[halo] == SENT).all() and (pv.cpu().numpy()[~halo] != SENT).any()      # INTERIOR left the other phase's rows alone
    op.tracers_euler_step_phase(PHASE_HALO, dt, ud, out, f)
    phased = collect(f, out)
    for k in whole:
        assert np.array_equal(phased[k], whole[k]) if k != "courant" else phased[k] == whole[k], k
    # ... and the whole evaluation is the unphased call
    f2 = _full((mesh.num_owned_cells, n), float("nan"))
    op.tracers_rhs_function(dt, ud, f2)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(f2.cpu().numpy()), whole["F"]) and _courant(op) == whole["courant"]
    op.destroy()


# ---- halo steps ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_parts():
    """a 600-cell jittered triangle mesh with an HR tracer case (NT = 2, Roe), its reference results and its two RCB parts"""
    rng = np.random.default_rng(641)
    xyz, conn = RC.random_connectivity(rng, "tri", 20, 15)
    classifier = M.box_side_boundaries(0, 20, 0, 15)
    g = M.build_mesh(xyz, conn, boundary_classifier=classifier)
    assert g.num_cells == 600
    case, ref, u = hr_tracer_case(rng, g, 2, TRACER_RIEMANN_ROE)
    F = ref.apply(case.dt, u)
    assert np.isfinite(F).all()
    parts = TP.split(g, case, ref, u, 2, classifier)
    assert all(p.peers for p in parts)
    return g, case, ref, u, F, parts


@pytest.mark.parametrize("form", ["in_order", "two_streams"])
def test_halo_steps_of_two_parts_against_the_reference_on_the_undivided_mesh(form):
    """HaloExchange.tracers_step_overlapped on each of the two parts, the other rank played by the scripted transport of
    test_gpu_tracers_multirank.py: F and u_out of the owned rows against the HR reference on the undivided mesh"""
    from test_gpu_tracers_multirank import Scripted
    torch = _torch()
    g, case, ref, u, F, parts = _two_parts()
    got_f, got_u = np.full_like(F, np.nan), np.full_like(u, np.nan)
    best = 0.0
    for part in parts:
        mesh = part.mesh
        assert np.array_equal(mesh.cell_zc, g.cell_zc[np.asarray(mesh.cell_global_ids)])
        op = _arm(CS.create_operator(part.case), part.ref)
        h = Scripted(op, part)
        h.serve(part.u)
        hx = h.as_halo_exchange()
        hx.set_form("tracers_euler", form)
        assert hx.form_info("tracers_euler")["form"] == form
        start = np.array(part.u)
        start[mesh.cell_is_owned == 0] = np.nan
        ud, out, f = _dev(start), _full(part.u.shape, SENT), _full((mesh.num_owned_cells, 5), float("nan"))
        hx.tracers_step_overlapped(op, case.dt, ud, out, f)
        torch.cuda.synchronize()
        assert h.calls == 1 and np.array_equal(_bits(ud.cpu().numpy()), _bits(part.u))       # the ghost rows arrived
        own = np.asarray(mesh.cell_global_ids)[mesh.cell_owned_to_local]
        got_f[own] = f.cpu().numpy()
        got_u[own] = out.cpu().numpy()[mesh.cell_owned_to_local]
        assert (out.cpu().numpy()[mesh.cell_is_owned == 0] == SENT).all()
        op.update_diagnostics()
        best = max(best, op.get_diagnostics().max_courant_num)
        h.destroy()
        op.destroy()
    err, uerr = rel_linf(got_f, F), rel_linf(got_u, u + case.dt * F)
    print(f"{form}: F of the two parts vs the undivided HR reference {err:.3e}, u_out {uerr:.3e}")
    assert np.isfinite(got_f).all() and err <= TOL and uerr <= TOL
    assert abs(best - ref.courant[0]) <= 1e-12 * max(1.0, ref.courant[0])


# ---- the levee deck ----------------------------------------------------------------------------------------------------------------------
def _levee():
    case = CS.levee_hr_case(os.path.join(os.path.dirname(houston.DATA), "levee"))
    assert case.mesh.num_cells == 506
    u = np.zeros((506, 5))
    u[:, :3] = case.u_local
    return case, u


def _with_classes(u):
    u[:, 3], u[:, 4] = 0.3 * u[:, 0], 0.05 * u[:, 0]
    return u


def _levee_run(case, u0, nsteps=40, dt=0.1):
    """(device state, reference state, the reference's largest Courant number) after `nsteps` TracerEulerStepper steps"""
    torch = _torch()
    ref = THR.TracerHRReference(case.mesh, case.condition_types, 2)
    ref.mannings[:] = case.mannings
    want, cmax = u0.copy(), 0.0
    for _ in range(nsteps):
        want = want + dt * ref.apply(dt, want)
        cmax = max(cmax, ref.courant[0])
    op = CS.create_operator(case)
    op.enable_tracers(2, well_balancing=WELL_BALANCING_HR)
    stepper = TracerEulerStepper(op)
    got = stepper.advance(_dev(u0), dt, nsteps)
    torch.cuda.synchronize()
    assert stepper.step == nsteps
    got = got.cpu().numpy()
    op.destroy()
    return got, want, cmax


def test_levee_trajectory_with_two_sediment_classes():
    """the reference's HR deck with two classes at 0.3 and 0.05, the water raised by 0.5 m in the wet cells left of the median wet x:
    40 steps of 0.1 s wet new cells over the levee's foot; against the same loop in numpy"""
    case, u0 = _levee()
    wet = u0[:, 0] > 0.0
    x = case.mesh.cell_centroids[:, 0]
    u0[wet & (x < np.median(x[wet])), 0] += 0.5
    _with_classes(u0)
    got, want, cmax = _levee_run(case, u0)
    newly = int(((want[:, 0] > 0.0) & ~(u0[:, 0] > 0.0)).sum())
    err = rel_linf(got, want)
    print(f"levee, dam: 40 steps, state vs reference {err:.3e}; reference: max Courant {cmax:.3f}, {newly} cells newly wet, min h {want[:, 0].min():.3e}")
    assert np.isfinite(want).all() and 0.0 < cmax < 1.0 and newly > 0 and want[:, 0].min() >= 0.0
    assert np.isfinite(got).all() and err <= TOL


def test_levee_at_rest_keeps_the_bits_of_h():
    """the unmodified deck (a lake at rest on both sides of the levee): after 40 steps h has its bits in every cell, on the device
    as in the restatement; the classes settle"""
    case, u0 = _levee()
    _with_classes(u0)
    got, want, _ = _levee_run(case, u0)
    assert np.array_equal(_bits(want[:, 0]), _bits(u0[:, 0]))
    print(f"levee, at rest: 40 steps, max |momentum| on the device {np.abs(got[:, 1:3]).max():.3e}, state vs reference {rel_linf(got, want):.3e}")
    assert np.array_equal(_bits(got[:, 0]), _bits(u0[:, 0]))
    assert rel_linf(got, want) <= TOL and (got[u0[:, 0] > 0.0, 3] < u0[u0[:, 0] > 0.0, 3]).all()


# ---- tracer output -------------------------------------------------------------------------------------------------------------------------
def test_tracer_output_on_an_hr_operator():
    """one primitive read-out (the bits the evaluation stores, the reference's values) and one set of error sums (the host's
    math.fsum forms of test_gpu_tracer_output.py) through an operator enabled with rdyhip_tracer_hr_enable"""
    from test_gpu_tracer_output import _host_sums
    torch = _torch()
    nt = 2
    case, ref, u, _ = _case("tri-hr", nt, TRACER_RIEMANN_UPWIND_ROE)
    mesh, n = case.mesh, 3 + nt
    op = _operator(case, ref)
    ud = _dev(u)
    pv = op.tracers_primitive_variables()
    op.tracers_rhs_function(case.dt, ud, _full((mesh.num_owned_cells, n), 0.0))
    torch.cuda.synchronize()
    planes = op.tracers_state_planes(ud, (1 << n) - 1, TRACER_FORM_PRIMITIVE).cpu().numpy()
    assert np.array_equal(_bits(planes), _bits(pv.cpu().numpy().T))
    assert rel_linf(planes.T, ref.primitive_variables) <= TOL
    got, want = op.tracers_error_sums(ud), _host_sums(mesh, u, None)
    for k in ("l1", "l2_squared"):
        for c in range(n):
            assert abs(float(got[k][c]) - float(want[k][c])) <= 1e-13 * float(want[k][c]), (k, c)
    assert np.array_equal(_bits(got["linf"]), _bits(want["linf"])) and abs(got["area"] - want["area"]) <= 1e-13 * want["area"]
    op.destroy()


# ---- the SWE path ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed-hr", "part-o2l"])
def test_the_swe_path_is_undisturbed(name):
    """After enable_tracers(..., well_balancing=HR) and a tracer evaluation, rdyhip_rhs_function on the [num_cells, 3] state gives
    the bits of a fresh HR operator: F, primitive variables, boundary fluxes and the Courant struct."""
    torch = _torch()
    case, ref, u, _ = _case(name, 2, TRACER_RIEMANN_UPWIND_ROE)
    mesh = case.mesh
    plain = CS.create_operator(case)
    op = _operator(case, ref)
    op.tracers_primitive_variables()
    op.tracers_rhs_function(case.dt, _dev(u), _full((mesh.num_owned_cells, 5), 0.0))
    u3 = _dev(case.u_local)
    res = []
    for o in (plain, op):
        pv = o.primitive_variables
        f = _full((mesh.num_owned_cells, 3), float("nan"))
        o.rhs_function(case.dt, u3, f)
        torch.cuda.synchronize()
        res.append(([_bits(f.cpu().numpy()), _bits(pv.cpu().numpy())] + [_bits(o.boundary_fluxes(b)) for b in range(len(mesh.boundaries))] +
                    [_bits(o.boundary_fluxes(b, accumulated=True)) for b in range(len(mesh.boundaries))], _courant(o)))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    assert np.isfinite(res[0][0][0].view(np.float64)).all() and res[0][1] == res[1][1] and res[0][1][1] >= 0
    plain.destroy()
    op.destroy()


# ---- refusals, bookkeeping, a rank that owns nothing -----------------------------------------------------------------------------------------
def test_refusals_info_and_device_bytes():
    _torch()
    lib = _lib.load()
    hr_cfg = lambda **kw: RDyFlowConfig(well_balancing=WELL_BALANCING_HR, **kw)
    mesh = _hr_mesh("tri-hr")
    refl = [M.CONDITION_REFLECTING] * len(mesh.boundaries)

    def refused(op, n, riemann, text, wb=WELL_BALANCING_HR):
        before = op.layout_info()["device_bytes"]
        with pytest.raises(RDyHipError) as e:
            op.enable_tracers(n, riemann, well_balancing=wb)
        assert e.value.code == 83 and text in e.value.message, e.value.message
        assert op.tracers_info() == (0, 0) and op.tracers_well_balancing() == WELL_BALANCING_NONE
        assert op.layout_info()["device_bytes"] == before                 # nothing was allocated
    # a null operator, reported first
    assert lib.rdyhip_tracer_hr_enable(None, 0, 7) == 83 and b"null operator" in lib.rdyhip_last_error()
    assert lib.rdyhip_tracer_hr_info(None, None) == 83 and b"null operator" in lib.rdyhip_last_error()
    # an operator without HR: the message points to rdyhip_tracers_enable
    op = Operator.create(RDyFlowConfig(), mesh, refl)
    refused(op, 2, 0, "rdyhip_tracers_enable")
    op.enable_tracers(2)
    assert op.tracers_well_balancing() == WELL_BALANCING_NONE         # a plain tracer operator
    with pytest.raises(RDyHipError) as e:                              # ... on which the HR enable is a second enable
        op.enable_tracers(2, well_balancing=WELL_BALANCING_HR)
    assert e.value.code == 83 and "already enabled" in e.value.message and op.tracers_info() == (2, 0)
    op.destroy()
    # second_order (which cannot be created together with HR)
    op = Operator.create(RDyFlowConfig(second_order=True), mesh, refl)
    refused(op, 1, 0, "second_order")
    op.destroy()
    # a source method other than semi-implicit
    op = Operator.create(hr_cfg(source_method=SOURCE_IMPLICIT_XQ2018), mesh, refl)
    refused(op, 1, 0, "Only semi_implicit is supported for tracer HR")
    op.destroy()
    # a critical-outflow boundary
    op = Operator.create(hr_cfg(), mesh, [M.CONDITION_CRITICAL_OUTFLOW] + refl[1:])
    refused(op, 1, 0, "CRITICAL_OUTFLOW")
    op.destroy()
    # num_tracers outside 1..7, an unknown solver; the plain enable is still refused on this operator, with a message that names the new call
    op = Operator.create(hr_cfg(), mesh, refl)
    for n, r in ((0, 0), (8, 0), (-1, 0)):
        refused(op, n, r, "num_tracers")
    for n, r in ((2, 2), (2, -1)):
        refused(op, n, r, "Riemann")
    refused(op, 1, 0, "rdyhip_tracer_hr_enable", wb=WELL_BALANCING_NONE)
    with pytest.raises(RDyHipError) as e:
        op.enable_tracers(1)
    assert e.value.code == 83
    # the enable itself: the plain enable's allocations, counted the same way
    assert op.tracers_well_balancing() == WELL_BALANCING_NONE
    before = op.layout_info()["device_bytes"]
    op.enable_tracers(2, TRACER_RIEMANN_UPWIND_ROE, well_balancing=WELL_BALANCING_HR)
    K = sum(b.num_edges for b in mesh.boundaries)
    assert op.layout_info()["device_bytes"] == before + 8 * (2 * 5 * K + 2 * mesh.num_owned_cells)
    assert op.tracers_info() == (2, TRACER_RIEMANN_UPWIND_ROE) and op.tracers_well_balancing() == WELL_BALANCING_HR
    for b in range(len(mesh.boundaries)):
        assert (op.tracers_boundary_fluxes(b) == 0.0).all()
    # tracers already enabled: either call
    for wb in (WELL_BALANCING_HR, WELL_BALANCING_NONE):
        with pytest.raises(RDyHipError) as e:
            op.enable_tracers(2, TRACER_RIEMANN_UPWIND_ROE, well_balancing=wb)
        assert e.value.code == 83 and "already enabled" in e.value.message
    assert op.tracers_info() == (2, TRACER_RIEMANN_UPWIND_ROE) and op.tracers_well_balancing() == WELL_BALANCING_HR
    assert op.layout_info()["device_bytes"] == before + 8 * (2 * 5 * K + 2 * mesh.num_owned_cells)
    op.destroy()


def test_a_rank_that_owns_nothing():
    torch = _torch()
    mesh = _empty_mesh()
    assert mesh.cell_zc.shape == (mesh.num_cells,)
    op = Operator.create(RDyFlowConfig(well_balancing=WELL_BALANCING_HR), mesh)
    op.enable_tracers(3, well_balancing=WELL_BALANCING_HR)
    assert op.tracers_well_balancing() == WELL_BALANCING_HR
    u = torch.zeros((mesh.num_cells, 6), dtype=torch.float64, device="cuda")
    f = torch.empty((0, 6), dtype=torch.float64, device="cuda")
    op.tracers_rhs_function(0.1, u, f)
    out = torch.full_like(u, 5.0)
    op.tracers_euler_step(0.1, u, out)
    for phase in (PHASE_ALL, PHASE_INTERIOR, PHASE_HALO):
        op.tracers_rhs_phase(phase, 0.1, u, f, reset_diagnostics=True)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5.0).all()
    assert op.tracers_primitive_variables().shape == (0, 6)
    op.update_diagnostics()
    assert op.get_diagnostics().max_courant_num == 0.0
    op.destroy()
