"""CPU: ensembles under hydrostatic reconstruction (rdyhip_ens_hr_*, ensemble_hr_kernel in csrc/ensemble_kernels.h) as far as they
go without a device -- the two symbols against the header and their null-operator refusal, the eight instantiations of the kernel
in the built library and their registers, and the precondition of tests/test_gpu_ensemble_hr.py: every member that file evaluates
has, from the C oracle created with hydrostatic reconstruction, a finite F and a largest Courant number that is no near tie.

The meshes, configurations, seeds and members of the GPU file are defined here and imported by it, so both files look at the same
cases: member k of (mesh, source) is random_case(default_rng(9000 + 100 len(name) + 10 source + k), mesh, config)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from helpers import interior_courant_numbers, oracle_from_case
from random_cases import random_case, random_mixed_mesh
from rdycore_amd import _lib, build, codeobj
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig, SOURCE_IMPLICIT_XQ2018, SOURCE_SEMI_IMPLICIT, WELL_BALANCING_HR
from test_gpu_ensemble import boundary_courant_numbers
from test_gpu_tracers import _bathymetry
from test_gpu_tracers_hr import _hr_mesh
from test_tracers_hr_cpu import lake_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rdyhip_ens_hr_enable", "rdyhip_ens_hr_info"]
MESHES = ["tri-hr", "mixed-hr", "quad-44", "part-o2l"]
SOURCES = [SOURCE_SEMI_IMPLICIT, SOURCE_IMPLICIT_XQ2018]
GRAVITY = 9.806
# (mesh, source, members): the largest member count the GPU file asks of each (mesh, source); smaller counts are prefixes
CONFIGURATIONS = ([("tri-hr", src, 64) for src in SOURCES] + [(name, src, 7) for name in MESHES[1:] for src in SOURCES] +
                  [("tri-8192", SOURCE_SEMI_IMPLICIT, 33), ("mixed-38k", SOURCE_IMPLICIT_XQ2018, 50)])
# seeds whose state has two edges at the largest Courant number to 5e-12 (quad-44, semi-implicit): `member` refuses them, the
# member lists skip them, as test_gpu_ensemble.py does with 7705
TIED_SEEDS = {9700}


@functools.lru_cache(maxsize=None)
def hr_ensemble_mesh(name):
    """tri-hr (126 cells), mixed-hr (80) and quad-44 with centroid elevations: the meshes of test_gpu_tracers_hr.py; part-o2l: 972
    owned cells of 1043, ghosts interleaved; tri-8192: 32 workgroups; mixed-38k: 38 448 quads and triangles"""
    if name == "tri-8192":
        mesh = M.structured_tri_mesh(64, 64, 1.0, zfunc=_bathymetry)
        assert mesh.num_owned_cells == 8192
    elif name == "mixed-38k":
        mesh = random_mixed_mesh(np.random.default_rng(3), 160, 160)
        assert mesh.num_owned_cells == 38448 and (mesh.cell_nverts == 3).any() and (mesh.cell_nverts == 4).any()
    else:
        mesh = _hr_mesh(name)
    assert np.ptp(mesh.cell_zc) > 0.0
    return mesh


def hr_config(name, src):
    return RDyFlowConfig(source_method=src, well_balancing=WELL_BALANCING_HR, h_anuga_regular=1e-3 if name == "quad-44" else 0.0)


def seeds(name, src, B, first=0):
    base = 9000 + 100 * len(name) + 10 * src + first
    return [s for s in range(base, base + B + len(TIED_SEEDS)) if s not in TIED_SEEDS][:B]


@functools.lru_cache(maxsize=None)
def member(name, src, seed):
    """(case, F, boundary fluxes, (Courant number, edge, cell)) of one member from the C oracle with hydrostatic reconstruction:
    computed once, shared, left unchanged.  Refuses a state without a finite F or a positive Courant number and, on a mesh without
    ghosts, one whose largest Courant number the numpy restatement does not reproduce or that has a near tie."""
    mesh = hr_ensemble_mesh(name)
    case = random_case(np.random.default_rng(seed), mesh, hr_config(name, src))
    orc = oracle_from_case(case)
    F = orc.apply(case.dt, case.u_local)
    assert np.isfinite(F).all(), (name, src, seed)
    bf = [np.array(b) for b in orc.boundary_fluxes]
    diag = orc.diagnostics()
    orc.close()
    assert diag[0] > 0.0, (name, src, seed)
    if mesh.num_cells == mesh.num_owned_cells:
        c = np.concatenate([interior_courant_numbers(case), boundary_courant_numbers(case)])
        c = np.sort(c[np.isfinite(c)])
        assert abs(c[-1] - diag[0]) <= 1e-12 * max(1.0, diag[0]), (name, src, seed, c[-1], diag[0])
        assert c[-1] - c[-2] > 1e-9 * c[-1], f"{name} source {src} seed {seed}: the state has a near tie (gap {(c[-1] - c[-2]) / c[-1]:.1e})"
    for a in [case.u_local, case.mannings, case.ext_src, F] + bf:
        a.setflags(write=False)
    return case, F, bf, diag


def members(name, src, B, first=0):
    return [member(name, src, s) for s in seeds(name, src, B, first)]


# ---- lakes at rest, one per member ----------------------------------------------------------------------------------------------
LAKE_LEVELS = (0.3, 0.6, 0.9, 1.5)
LAKE_DRY = {"tri": (60, (50, 19, 4, 0)), "mixed": (112, (79, 40, 10, 0))}


def lakes(name):
    """(mesh, states [4, num_cells, 3], scales [4]): eta = zmin + f (zmax - zmin) for f in LAKE_LEVELS over lake_mesh(name) of
    test_tracers_hr_cpu.py (x-y projected), h = max(0, eta - zc), zero momentum; scale = 0.5 g hmax^2 max len / min area, the size
    of one edge's pressure term in that member's F"""
    mesh = lake_mesh(name)
    zc = np.asarray(mesh.cell_zc)
    u = np.zeros((len(LAKE_LEVELS), mesh.num_cells, 3))
    for m, f in enumerate(LAKE_LEVELS):
        u[m, :, 0] = np.maximum(0.0, zc.min() + f * (zc.max() - zc.min()) - zc)
    cells, dry = LAKE_DRY[name]
    assert mesh.num_cells == cells and tuple(int((u[m, :, 0] == 0.0).sum()) for m in range(len(LAKE_LEVELS))) == dry
    scales = 0.5 * GRAVITY * u[:, :, 0].max(axis=1) ** 2 * mesh.edge_lengths.max() / mesh.cell_areas.min()
    return mesh, u, scales


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_bound_and_report_a_null_operator():
    with open(os.path.join(ROOT, "include", "rdyhip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    ctype = {"RDyHipOperator": C.c_void_p, "int32_t": C.c_int32, "int32_t *": _lib.c_int32_p}
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("rdyhip_ens_hr_")) == sorted(SYMBOLS)
    lib = _lib.load()
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/rdyhip.h"
        params = [re.sub(r"\s*\w+$", "", p.strip()).strip() for p in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and [ctype[p] for p in params] == list(argtypes), (name, params, argtypes)
        assert getattr(lib, name).argtypes == argtypes, name
    wb = C.c_int32(-1)
    for name, args in (("rdyhip_ens_hr_enable", (None, 2)), ("rdyhip_ens_hr_info", (None, C.byref(wb)))):
        assert getattr(lib, name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())
    # the null operator is reported first, whatever else is wrong with the arguments
    assert lib.rdyhip_ens_hr_enable(None, 0) == 83 and b"null operator" in lib.rdyhip_last_error()
    assert lib.rdyhip_ens_hr_info(None, None) == 83 and b"null operator" in lib.rdyhip_last_error()
    assert lib.rdyhip_version() == 110


# ---- the built code object ------------------------------------------------------------------------------------------------------
def test_every_hr_ensemble_kernel_keeps_its_geometry_on_chip():
    """2 slot counts x 2 source methods x with / without the fused Euler update of ensemble_hr_kernel; a per-thread array that went
    to scratch, or a spilled register, shows in the code object's metadata.  The plain family is still eight kernels of its own."""
    all_res = codeobj.kernel_resources(build.lib_path())
    res = {k: v for k, v in all_res.items() if "ensemble_hr_kernel<" in k}
    forms = {k.split("ensemble_hr_kernel<")[1].split(">")[0] for k in res}
    assert forms == {f"{s}, {src}, {eu}" for s in (3, 4) for src in (0, 1) for eu in ("false", "true")} and len(res) == 8
    for k in sorted(res):
        print(k.split("(")[0], res[k])
    bad = {k: v for k, v in res.items() if v["scratch"] != 0 or v["vgpr_spills"] != 0 or v["sgpr_spills"] != 0}
    assert not bad, bad
    assert max(v["vgpr"] + v["agpr"] for v in res.values()) <= 256          # at least two waves per SIMD
    assert not any("ensemble_rhs_kernel<" in k for k in res)
    assert sum("ensemble_rhs_kernel<" in k for k in all_res) == 8


# ---- the precondition of the GPU file -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,src,B", CONFIGURATIONS)
def test_every_member_of_the_gpu_file_has_a_finite_rhs_and_no_near_tie(name, src, B):
    """`member` asserts it for each seed; here every (mesh, source, seed) the GPU file uses is built once"""
    got = members(name, src, B)
    assert len(got) == B and len({id(m[0]) for m in got}) == B
    mesh = hr_ensemble_mesh(name)
    assert all(m[0].config.well_balancing == WELL_BALANCING_HR and m[0].condition_types == got[0][0].condition_types for m in got)
    if name == "part-o2l":
        assert (mesh.num_owned_cells, mesh.num_cells) == (972, 1043)
    h = np.stack([m[0].u_local[:, 0] for m in got])
    assert (h == 0.0).any() and (h > got[0][0].config.tiny_h).any()          # wet / dry fronts: what HR is for
    print(f"{name} source {src}: {B} members, Courant numbers {min(m[3][0] for m in got):.3g} .. {max(m[3][0] for m in got):.3g}")


def test_the_tied_seed_is_a_near_tie():
    """9700 is left out for the reason given: `member` refuses it"""
    assert 9700 not in seeds("quad-44", SOURCE_SEMI_IMPLICIT, 7) and 9700 == 9000 + 100 * len("quad-44") + 10 * SOURCE_SEMI_IMPLICIT
    with pytest.raises(AssertionError, match="near tie"):
        member("quad-44", SOURCE_SEMI_IMPLICIT, 9700)


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("name", sorted(LAKE_DRY))
def test_the_lakes_of_the_gpu_file_are_at_rest_under_the_hr_oracle_only(name, src):
    """the bar the GPU file holds the device to, 1e-10 max(1, scale), separates the two oracles: with HR every cancellation is exact
    up to a few roundings of terms of the size of `scale`; without it a partly dry lake accelerates with a sizeable share of one
    edge's pressure term (0.06 to 0.36 of it here), held to a thousandth of it: seven orders above the bar"""
    from rdycore_amd import cases as CS
    mesh, u, scales = lakes(name)
    types = [M.CONDITION_REFLECTING] * len(mesh.boundaries)
    no = mesh.num_owned_cells
    for m in range(u.shape[0]):
        res = []
        for wb in (WELL_BALANCING_HR, 0):
            case = CS.Case("lake", mesh, RDyFlowConfig(source_method=src, well_balancing=wb), types, u[m], np.zeros(no), np.zeros((no, 3)), {}, 0.1)
            orc = oracle_from_case(case)
            res.append(float(np.abs(orc.apply(0.1, u[m])).max()))
            orc.close()
        print(f"{name} source {src} level {LAKE_LEVELS[m]}: max |F| with HR {res[0]:.3e}, without {res[1]:.3e}, scale {scales[m]:.3g}")
        assert res[0] <= 1e-10 * max(1.0, scales[m]) and res[1] > 1e-3 * max(1.0, scales[m])
