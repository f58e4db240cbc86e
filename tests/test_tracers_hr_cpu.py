"""CPU: tracers under hydrostatic reconstruction (rdyhip_tracer_hr_enable, tracer_hr_kernel in csrc/tracer_kernels.h) as far as it
goes without a device -- the numpy restatement the GPU tests compare against (tests/tracer_hr_reference.py) is tied to the C oracle
created with hydrostatic reconstruction, to a lake at rest and to a hand-derived answer; the two new entry points are in the ctypes
table as the header declares them and report a null operator; every instantiation of the kernel keeps its rows in registers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import random_cases as RC
import tracer_hr_reference as THR
import tracer_reference as TR
from helpers import oracle_from_case, rel_linf
from rdycore_amd import _lib, build, codeobj
from rdycore_amd import mesh as M
from rdycore_amd.operator import WELL_BALANCING_HR
from test_tracers_cpu import tracer_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hr_reference_like(ref, mesh):
    """the HR reference with every input of a plain one"""
    hr = THR.TracerHRReference(mesh, ref.types, ref.nt, ref.riemann, ref.tiny_h, ref.h_anuga)
    hr.mannings[:] = ref.mannings
    hr.external_sources[:] = ref.external_sources
    hr.tracer_sources[:] = ref.tracer_sources
    for b in range(len(mesh.boundaries)):
        hr.boundary_values[b][:] = ref.boundary_values[b]
    return hr


def hr_tracer_case(rng, mesh, nt, riemann, h_anuga=0.0, region_block=0, exact_tiny=6):
    """test_tracers_cpu.tracer_case for an operator with hydrostatic reconstruction: (case, HR reference, state).  Up to
    `exact_tiny` of the KIND_TINY cells get h == tiny_h exactly with their momentum kept (metres per second), which is where the
    HR operator's wet test (h > tiny_h) and the plain one (h < tiny_h => 0) part.  Also used by the GPU tests."""
    case, ref, u = tracer_case(rng, mesh, nt, riemann, h_anuga=h_anuga, region_block=region_block)
    case.config.well_balancing = WELL_BALANCING_HR
    tiny = np.flatnonzero(case.cell_kind == RC.KIND_TINY)
    pick = tiny[:: max(1, tiny.size // exact_tiny)][:exact_tiny] if exact_tiny else tiny[:0]
    u[pick, 0] = case.config.tiny_h
    case.u_local[pick, 0] = case.config.tiny_h
    case.exact_tiny_cells = pick
    return case, hr_reference_like(ref, mesh), u


# ---- (a) the flow components are the C oracle's HR right-hand side ---------------------------------------------------------------
@pytest.mark.parametrize("riemann", [TR.RIEMANN_ROE, TR.RIEMANN_UPWIND_ROE])
@pytest.mark.parametrize("region_block", [0, 16])
@pytest.mark.parametrize("kind,nx,ny", [("tri", 9, 7), ("quad", 8, 6), ("mixed", 8, 8)])
def test_flow_components_are_the_oracles_hr_rhs(kind, nx, ny, region_block, riemann):
    """F[:, :3], the Courant number and its edge and cell against the pinned C oracle with well_balancing = HR at 1e-12 relative
    (the bar of test_flow_components_are_the_oracles_first_order_rhs), on states with cells at h == tiny_h exactly that move at
    metres per second: taking the plain wet rule for them changes F far beyond the bar (measured: 4e-2 relative on the first triangle
case).  Every case has interior edges of all four
    kinds: with a flux, with the pressure correction only, skipped, and with exactly one reconstructed depth equal to 0."""
    rng = np.random.default_rng(2024 + nx + region_block)
    mesh = RC.random_mesh(rng, kind, nx, ny)
    assert np.ptp(mesh.cell_zc) > 0.0
    for nt in (1, 3):
        case, ref, u = hr_tracer_case(rng, mesh, nt, riemann, region_block=region_block)
        assert case.exact_tiny_cells.size >= 3 and (np.abs(u[case.exact_tiny_cells, 1:3]).max(axis=1) > 0.0).any()
        assert {M.CONDITION_DIRICHLET, M.CONDITION_REFLECTING} == set(case.condition_types)
        orc = oracle_from_case(case)
        F = ref.apply(case.dt, u)
        Fo = orc.apply(case.dt, case.u_local)
        assert np.isfinite(F).all()
        err = rel_linf(F[:, :3], Fo)
        counts = (ref.edges_with_flux, ref.edges_correction_only, ref.edges_skipped, ref.edges_one_side_dry)
        print(f"{kind} block={region_block} nt={nt} riemann={riemann}: flow components vs HR oracle {err:.3e}, edges {counts}")
        assert err <= 1e-12
        assert min(counts) > 0, counts
        assert rel_linf(ref.primitive_variables[:, :3], orc.primitive_variables) <= 1e-12
        cmax, edge_gid, cell_gid = orc.diagnostics()
        assert cmax > 0.0 and abs(ref.courant[0] - cmax) <= 1e-12 * max(1.0, cmax)
        assert (int(mesh.edge_global_ids[ref.courant[1]]), int(mesh.cell_global_ids[ref.courant[2]])) == (edge_gid, cell_gid)


# ---- (b) a lake at rest ---------------------------------------------------------------------------------------------------------
def lake_at_rest(mesh):
    """(HR reference, plain reference, state, scale): eta = zmin + 0.6 (zmax - zmin), h = max(0, eta - zc), zero momentum, two
    tracers at uniform 0.3 and 0.05, every boundary reflecting, n = 0, no sources.  scale = 0.5 g hmax^2 max len / min area: the size
    of one edge's pressure term in F.  Also used by the GPU tests."""
    zc = np.asarray(mesh.cell_zc)
    eta = zc.min() + 0.6 * (zc.max() - zc.min())
    u = np.zeros((mesh.num_cells, 5))
    u[:, 0] = np.maximum(0.0, eta - zc)
    u[:, 3] = 0.3 * u[:, 0]
    u[:, 4] = 0.05 * u[:, 0]
    types = [M.CONDITION_REFLECTING] * len(mesh.boundaries)
    scale = 0.5 * TR.G * u[:, 0].max() ** 2 * mesh.edge_lengths.max() / mesh.cell_areas.min()
    return THR.TracerHRReference(mesh, types, 2), TR.TracerReference(mesh, types, 2), u, scale


LAKES = {"mixed": ("mixed", 8, 8, 31), "tri": ("tri", 6, 5, 32)}


def lake_mesh(name):
    kind, nx, ny, seed = LAKES[name]
    return RC.random_mesh(np.random.default_rng(seed), kind, nx, ny, project_2d=True)


@pytest.mark.parametrize("name", sorted(LAKES))
def test_a_lake_at_rest_stays_at_rest(name):
    """With x-y projected lengths and areas (without them a cell's edge vectors do not sum to zero and no scheme is at rest) the
    flow components vanish to rounding over a bed that is partly dry, and the tracers see only their deposition:
    F[3 + j] = -0.001 - 0.01 c_j in wet cells.  The plain tracer reference accelerates the same lake."""
    mesh = lake_mesh(name)
    hr, plain, u, scale = lake_at_rest(mesh)
    dry = int((u[:, 0] == 0.0).sum())
    assert 0 < dry < mesh.num_cells // 2
    F = hr.apply(0.1, u)
    bar = 1e-12 * max(1.0, scale)
    err = np.abs(F[:, :3]).max()
    wet = u[mesh.cell_owned_to_local, 0] >= hr.tiny_h
    terr = max(np.abs(F[wet, 3 + j] - (-0.001 - 0.01 * c)).max() for j, c in enumerate((0.3, 0.05)))
    F0 = plain.apply(0.1, u)
    print(f"{name}: {dry} of {mesh.num_cells} cells dry, max |F_flow| = {err:.3e} (scale {scale:.3g}), tracers {terr:.3e}; "
          f"without HR {np.abs(F0[:, :3]).max():.3g}")
    assert err <= bar and terr <= bar
    assert (F[~wet, 3:] == 0.0).all()
    assert np.abs(F0[:, :3]).max() > 0.1


# ---- (c) uniform concentration is carried by the mass flux ------------------------------------------------------------------------
@pytest.mark.parametrize("riemann,dry", [(TR.RIEMANN_ROE, True), (TR.RIEMANN_UPWIND_ROE, False)])
def test_uniform_concentration_is_carried_by_the_mass_flux_under_hr(riemann, dry):
    """The HR twin of test_uniform_concentration_is_carried_by_the_mass_flux, same construction and bar: with uniform c the Roe wave
    strength dW_j = (c hr_rec - c hl_rec) - c (hr_rec - hl_rec) vanishes on the reconstructed depths as it does on the original
    ones, the pressure correction has no tracer component, so F[3 + j] = c F[0] - 0.001 - 0.01 c in every wet cell.  A side that
    the reconstruction dries (h_rec = 0 with c kept) is the dry side of the plain test's argument."""
    rng = np.random.default_rng(77)
    mesh = RC.random_mesh(rng, "mixed", 8, 8)
    conc = np.array([0.3, 0.05])
    case, ref, u = tracer_case(rng, mesh, 2, riemann, tiny=False)
    ref = hr_reference_like(ref, mesh)
    if not dry:
        u[:, :3] = np.where(u[:, :1] < 0.2, np.array([[1.0, 0.3, -0.2]]), u[:, :3])
    else:
        assert (u[:, 0] == 0.0).any()
    ref.mannings[:] = 0.0
    ref.external_sources[:] = 0.0
    ref.tracer_sources[:] = 0.0
    u[:, 3:] = u[:, :1] * conc
    for b in range(len(mesh.boundaries)):
        bv = ref.boundary_values[b]
        bv[:, 0] = np.where(bv[:, 0] < 0.1, 0.0 if dry else 0.5, bv[:, 0])
        bv[:, 3:] = bv[:, :1] * conc
    F = ref.apply(case.dt, u)
    own = mesh.cell_owned_to_local
    wet = u[own, 0] >= case.config.tiny_h
    assert wet.sum() > 50 and ref.edges_with_flux > 0
    speed = np.sqrt(TR.G * u[:, 0].max()) + 12.0
    e = mesh.edge_internal_ids
    scale = (mesh.edge_lengths[e] / np.minimum(mesh.cell_areas[mesh.edge_cell_ids[2 * e]], mesh.cell_areas[mesh.edge_cell_ids[2 * e + 1]])).max()
    T = scale * u[:, 0].max() * speed
    for j in range(2):
        want = conc[j] * F[wet, 0] - 0.001 - 0.01 * conc[j]
        err = np.abs(F[wet, 3 + j] - want).max()
        print(f"riemann={riemann} tracer {j}: max |F - (c F0 - 0.001 - 0.01 c)| = {err:.3e}, bar {1e-12 * max(1.0, T * conc[j]):.3e}")
        assert err <= 1e-12 * max(1.0, T * conc[j])


# ---- (d) the C ABI without a device ---------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_bound_and_report_a_null_operator():
    with open(os.path.join(ROOT, "include", "rdyhip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    ctype = {"RDyHipOperator": C.c_void_p, "int32_t": C.c_int32, "int32_t *": _lib.c_int32_p}
    for name in ("rdyhip_tracer_hr_enable", "rdyhip_tracer_hr_info"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/rdyhip.h"
        params = [re.sub(r"\s*\w+$", "", p.strip()).strip() for p in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and [ctype[p] for p in params] == list(argtypes), (name, params, argtypes)
    lib = _lib.load()
    wb = C.c_int32(-1)
    for name, args in (("rdyhip_tracer_hr_enable", (None, 2, 0)), ("rdyhip_tracer_hr_info", (None, C.byref(wb)))):
        assert getattr(lib, name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())
    # the null operator is reported first, whatever else is wrong with the arguments
    assert lib.rdyhip_tracer_hr_enable(None, 0, 5) == 83 and b"null operator" in lib.rdyhip_last_error()


# ---- (e) the built code object ----------------------------------------------------------------------------------------------------
def test_every_hr_tracer_kernel_keeps_its_rows_in_registers():
    """2 slot counts x 7 tracer counts x 2 flux variants of tracer_hr_kernel, none with scratch or a spilled register, each within
    256 VGPR + AGPR (two waves per SIMD: the bar the plain family is held to); the plain family is still 28 kernels of its own"""
    all_res = codeobj.kernel_resources(build.lib_path())
    res = {k: v for k, v in all_res.items() if "tracer_hr_kernel<" in k}
    forms = {k.split("tracer_hr_kernel<")[1].split(">")[0] for k in res}
    assert forms == {f"{s}, {nt}, {up}" for s in (3, 4) for nt in range(1, 8) for up in ("false", "true")} and len(res) == 28
    assert not any("tracer_rhs_kernel<" in k for k in res)
    bad = {k: v for k, v in res.items() if v["scratch"] != 0 or v["vgpr_spills"] != 0}
    assert not bad, bad
    worst = max(res, key=lambda k: res[k]["vgpr"] + res[k]["agpr"])
    print(f"most registers: {worst}: {res[worst]}")
    assert res[worst]["vgpr"] + res[worst]["agpr"] <= 256
