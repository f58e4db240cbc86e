"""Uniform fields: where every owned cell holds the same water source, the same Manning's n or a flat bed, the first-order / HR
tiled kernels read element 0 of the array in every lane instead of streaming the plane (KernelArgs::src_mom bits 1-3,
include/rdyhip.h "Uniform fields", rdycore_amd/csrc/uniform_fields.h).

The results must be the SAME BITS with the modes on and with RDYHIP_UNIFORM_FIELDS=0 -- F, u_out and the Courant struct -- and
both within the project's bar (rel L-inf <= 1e-10 against max(1, |ref|), test_gpu_parity.py) of the oracle, with the oracle's
ids.  Meshes as test_gpu_occupancy.py builds them: 400 triangles (two tiles, the second partly filled), 7 000 triangles and
7 020 quads under RDYHIP_PGRID=8 (several tiles per workgroup: both call sites of load_streams run, the last tile is partial),
and one RCB part whose owned cells are not a prefix.  Every case has a dry disc and one boundary of each type."""
import dataclasses
import functools

import numpy as np
import pytest

from rdycore_amd import _lib
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd import partition as P
from rdycore_amd.operator import (PHASE_ALL, PHASE_HALO, PHASE_INTERIOR, SOURCE_IMPLICIT_XQ2018, UNIFORM_FLAT_BED, UNIFORM_MANNINGS,
                                  UNIFORM_SOURCE, RDyFlowConfig, _ptr, _stream)

from helpers import oracle_from_case, rel_linf
from test_gpu_kernel_matrix import _KNOB_VARS

pytestmark = pytest.mark.gpu
TOL = 1e-10
K = 2 * np.pi / 50
# name -> (sloped bed, environment)
MESHES = {"tri400": (True, {}), "tri7000_flat": (False, {"RDYHIP_PGRID": "8"}), "tri7000": (True, {"RDYHIP_PGRID": "8"}),
          "quad7020_flat": (False, {"RDYHIP_PGRID": "8"}), "rcb_part": (True, {})}
OPERATORS = ["first", "hr", "xq"]
CALLS = [("rhs", False), ("apply", False), ("euler", False), ("rhs", True), ("euler", True)]   # (call, INTERIOR + HALO phases)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _mesh(name, project_2d):
    zf = CS.mms_bathymetry(K=K) if MESHES[name][0] else None
    if name == "tri400":
        return M.structured_tri_mesh(20, 10, 1.0, zfunc=zf, project_2d=project_2d), 20.0, 10.0
    if name.startswith("tri7000"):
        mesh = M.structured_tri_mesh(70, 50, 1.0, zfunc=zf, project_2d=project_2d)
        if zf is None:
            # the plane through three vertices at z = 0 has slopes of +0.0 in some triangles and -0.0 in others: not ONE pattern
            # (test_mixed_zero_slopes_are_not_a_flat_bed); this mesh is the flat one, +0.0 throughout
            assert (mesh.cell_dz_dx == 0).all() and (mesh.cell_dz_dy == 0).all() and np.signbit(mesh.cell_dz_dy).any()
            mesh.cell_dz_dx = np.zeros_like(mesh.cell_dz_dx)
            mesh.cell_dz_dy = np.zeros_like(mesh.cell_dz_dy)
        return mesh, 70.0, 50.0
    if name == "quad7020_flat":
        return M.structured_quad_mesh(90, 78, 1.0, 1.0, zfunc=zf, project_2d=project_2d), 90.0, 78.0
    # rank 1 of 3 of an RCB partition, ghosts interleaved with the owned cells in the source order
    xyz, conn, _, _ = M.structured_tri_connectivity(48, 30)
    xyz[:, 2] = zf(xyz[:, 0], xyz[:, 1])
    cent = xyz[conn, :2].mean(axis=1)
    mesh = M.extract_local_mesh(xyz, conn, P.rcb_owned_mask(cent, 3, 1), boundary_classifier=M.box_side_boundaries(0.0, 48.0, 0.0, 30.0),
                                ghosts="interleaved", project_2d=project_2d)
    return mesh, 48.0, 30.0


@functools.lru_cache(maxsize=None)
def _case(name, operator, second_order=False):
    """the friction / slope case (water source 1e-5 in every cell, a dry disc, Dirichlet / critical outflow / reflecting
    boundaries) with ONE Manning's n: every field that can be uniform is"""
    hr = operator == "hr"
    mesh, lx, ly = _mesh(name, hr)
    case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2, K=K, source_method=SOURCE_IMPLICIT_XQ2018 if operator == "xq" else 0)
    case.config = RDyFlowConfig(source_method=case.config.source_method, well_balancing=2 if hr else 0, second_order=second_order)
    case.mannings = np.full(mesh.num_owned_cells, 0.015)
    rng = np.random.default_rng(len(name) + 7 * OPERATORS.index(operator))
    f0 = rng.normal(size=(mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0])
    return case, f0


def _env(monkeypatch, env, uniform=True, kernel=None):
    for k in _KNOB_VARS + ("RDYHIP_UNIFORM_FIELDS", "RDYHIP_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not uniform:
        monkeypatch.setenv("RDYHIP_UNIFORM_FIELDS", "0")
    if kernel:
        monkeypatch.setenv("RDYHIP_KERNEL", kernel)


def _courant(op):
    op.update_diagnostics()
    d = op.get_diagnostics()
    return (d.max_courant_num, d.global_edge_id, d.global_cell_id)


def _evaluate(op, case, call, phased, f0, u=None):
    """one evaluation on an operator that exists: (F, u_out or None, Courant) on the host"""
    torch = _torch()
    no = case.mesh.num_owned_cells
    if u is None:
        u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    phases = (PHASE_INTERIOR, PHASE_HALO) if phased else (PHASE_ALL,)
    out = None
    if call == "apply":
        f = torch.tensor(f0, dtype=torch.float64, device="cuda")
    else:
        f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
    if call == "euler":
        out = torch.full_like(u, -7.0)
        for k, ph in enumerate(phases):
            op.euler_step(case.dt, u, out, f, phase=ph, reset_diagnostics=k == 0)
    elif phased:
        for k, ph in enumerate(phases):
            op.apply_phase(ph, call == "rhs", case.dt, u, f, reset_diagnostics=k == 0)
    elif call == "rhs":
        op.rhs_function(case.dt, u, f)
    else:
        op.reset_diagnostics()
        op.apply(case.dt, u, f)
    torch.cuda.synchronize()
    return f.cpu().numpy(), (out.cpu().numpy() if out is not None else None), _courant(op)


def _check_oracle(case, call, f0, res, what):
    """F, u_out and the Courant struct of one evaluation against the oracle holding the case's fields"""
    f, out, c = res
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local, f0.copy() if call == "apply" else None)
    assert np.isfinite(fr).all()
    err = rel_linf(f, fr)
    print(f"{what}: F rel L-inf vs oracle {err:.3e}")
    assert err <= TOL, (what, err)
    if out is not None:
        own = case.mesh.cell_owned_to_local
        err = rel_linf(out[own], case.u_local[own] + case.dt * fr)
        print(f"{what}: u_out rel L-inf vs oracle {err:.3e}")
        assert err <= TOL, (what, err)
        assert np.all(out[case.mesh.cell_is_owned == 0] == -7.0), "ghost rows of u_out were written"
    cref = orc.diagnostics()
    ctol = 1e-10 if case.config.second_order else 1e-12
    assert abs(c[0] - cref[0]) <= ctol * max(1.0, cref[0]) and c[1:] == tuple(cref[1:]), (what, c, cref)
    return fr


def _same_bits(a, b, what):
    assert np.array_equal(a[0], b[0], equal_nan=True), f"{what}: F differs between the modes"
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1], equal_nan=True)), f"{what}: u_out differs between the modes"
    assert a[2] == b[2], f"{what}: the Courant struct differs between the modes: {a[2]} / {b[2]}"


def _on_and_off(monkeypatch, case, env, calls, f0, expect, what, kernel=None):
    """every call with the modes on and with RDYHIP_UNIFORM_FIELDS=0: the same bits, the oracle's values"""
    for call, phased in calls:
        res = {}
        for uniform in (True, False):
            _env(monkeypatch, env, uniform, kernel)
            op = CS.create_operator(case)
            assert op.uniform_fields() == (expect if uniform else 0), (what, uniform, op.uniform_fields())
            assert op.source_is_water_only()
            res[uniform] = _evaluate(op, case, call, phased, f0)
            assert op.uniform_fields() == (expect if uniform else 0) and op.source_is_water_only()
            op.destroy()
        tag = f"{what} {call}{' phased' if phased else ''}"
        _same_bits(res[True], res[False], tag)
        _check_oracle(case, call, f0, res[True], tag)


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("name", list(MESHES))
def test_modes_on_and_off_agree_bit_for_bit_and_with_the_oracle(name, operator, monkeypatch):
    case, f0 = _case(name, operator)
    sloped, env = MESHES[name]
    _env(monkeypatch, env)
    op = CS.create_operator(case)
    info = op.layout_info()
    op.destroy()
    assert info["tiled_kernel"] == 1
    if name == "tri400":
        assert info["num_tiles"] == 2 and case.mesh.num_owned_cells % 256 != 0
    elif name == "rcb_part":
        assert info["owned_is_prefix"] == 0 and case.mesh.num_cells > case.mesh.num_owned_cells
    else:
        assert info["persistent_grid"] == 8 and info["num_tiles"] >= 3 * 8 and case.mesh.num_owned_cells % 256 != 0
    expect = UNIFORM_SOURCE | UNIFORM_MANNINGS | (0 if sloped else UNIFORM_FLAT_BED)
    _on_and_off(monkeypatch, case, env, CALLS, f0, expect, f"{name} {operator}")


def test_mixed_zero_slopes_are_not_a_flat_bed(monkeypatch):
    """-0.0 is not +0.0: a bed whose slopes are zeros of both signs is read cell by cell"""
    mesh = M.structured_tri_mesh(20, 10, 1.0)
    assert (mesh.cell_dz_dy == 0).all() and np.signbit(mesh.cell_dz_dy).any() and not np.signbit(mesh.cell_dz_dy).all()
    case = CS.friction_slope_case(mesh, 20.0, 10.0, dt=1e-2, K=K)
    case.mannings = np.full(mesh.num_owned_cells, 0.015)
    f0 = np.zeros((mesh.num_owned_cells, 3))
    _on_and_off(monkeypatch, case, {}, [("rhs", False)], f0, UNIFORM_SOURCE | UNIFORM_MANNINGS, "mixed zero slopes")


@pytest.mark.parametrize("which", ["second_order", "cell"])
def test_second_order_and_cell_kernels_are_unaffected(which, monkeypatch):
    """they always read the arrays, which stay current whatever the modes are"""
    case, f0 = _case("tri7000_flat", "first", second_order=which == "second_order")
    _on_and_off(monkeypatch, case, MESHES["tri7000_flat"][1], [("rhs", False), ("euler", False)], f0,
                UNIFORM_SOURCE | UNIFORM_MANNINGS | UNIFORM_FLAT_BED, which, kernel="cell" if which == "cell" else None)


def test_minus_zero_source_is_a_uniform_value_of_its_own(monkeypatch):
    case, f0 = _case("tri7000", "first")
    case = dataclasses.replace(case, ext_src=np.zeros_like(case.ext_src))
    case.ext_src[:, 0] = -0.0
    _on_and_off(monkeypatch, case, MESHES["tri7000"][1], [("rhs", False), ("apply", False)], f0, UNIFORM_SOURCE | UNIFORM_MANNINGS, "source -0.0")


@pytest.mark.parametrize("where", ["cell0", "last_owned_cell"])
def test_arrays_that_differ_in_one_cell_run_in_array_mode(where, monkeypatch):
    """all cells but the first / the last owned one hold one value: element 0 must not stand for the rest"""
    base, f0 = _case("tri7000", "first")
    i = 0 if where == "cell0" else base.mesh.num_owned_cells - 1
    case = dataclasses.replace(base, mannings=base.mannings.copy(), ext_src=base.ext_src.copy())
    case.mannings[i] = 0.05
    case.ext_src[i, 0] = 3e-3
    _on_and_off(monkeypatch, case, MESHES["tri7000"][1], [("rhs", False), ("euler", False)], f0, 0, where)


def test_restart_partial_writes_and_escape(monkeypatch):
    """the transitions on a live operator: after every write the mask is the expected one and the next launch computes with
    what the arrays hold; the water-only mode of the source is the same throughout"""
    torch = _torch()
    base, f0 = _case("tri7000", "first")
    _env(monkeypatch, MESHES["tri7000"][1])
    no = base.mesh.num_owned_cells
    cur = dataclasses.replace(base, mannings=base.mannings.copy(), ext_src=base.ext_src.copy())
    op = CS.create_operator(cur)
    both = UNIFORM_SOURCE | UNIFORM_MANNINGS
    rng = np.random.default_rng(5)

    def step(what, expect):
        assert op.uniform_fields() == expect, (what, op.uniform_fields())
        assert op.source_is_water_only(), what
        res = _evaluate(op, cur, "rhs", False, f0)
        _check_oracle(cur, "rhs", f0, res, what)
        return res[0]

    step("after create", both)
    # a restart with a NEW uniform value, through each kind of whole-domain write
    cur.mannings[:] = 0.03
    op.set_domain_mannings_n(cur.mannings)
    cur.ext_src[:, 0] = 4e-4
    op.set_domain_external_source(0, cur.ext_src[:, 0], ordered=True)
    step("new values by the setters", both)
    cur.mannings[:] = 0.02
    op.refresh_field(2, cur.mannings)
    cur.ext_src[:, 0] = -2e-5
    op.refresh_field(1, cur.ext_src)
    step("new values by refresh_field", both)
    cur.ext_src[:, 0] = 7e-5
    _lib.check(_lib.load().rdyhip_forcing_fill_source(op._h, 0, no, None, 7e-5, _stream()))
    f_before = step("new source by forcing_fill_source", both)
    # a partial write of the SAME value keeps the mode ...
    ids = np.sort(rng.permutation(no)[:17]).astype(np.int32)
    op.set_regional_mannings_n(ids, np.full(ids.size, 0.02), ordered=True)
    op.set_regional_external_source(ids, 0, np.full(ids.size, 7e-5))
    f_same = step("partial writes of the value", both)
    assert np.array_equal(f_before, f_same)
    # ... of another value ends it, and exactly those cells change
    cur.ext_src[ids, 0] = 9e-5
    op.set_regional_external_source(ids, 0, cur.ext_src[ids, 0], ordered=True)
    f_src = step("partial write of another source", UNIFORM_MANNINGS)
    changed = np.nonzero((f_src != f_before).any(axis=1))[0]
    assert np.array_equal(changed, ids), (changed, ids)
    uo = cur.u_local[cur.mesh.cell_owned_to_local]      # friction acts where water moves: cells whose F it changes beyond a doubt
    wet = np.sort(rng.permutation(np.nonzero((uo[:, 0] > 0.5) & (np.abs(uo[:, 1]) > 0.1) & (np.abs(uo[:, 2]) > 0.1))[0])[:13]).astype(np.int32)
    assert wet.size == 13
    cur.mannings[wet] = 0.06
    op.set_regional_mannings_n(wet, cur.mannings[wet])
    f_n = step("partial write of another Manning's n", 0)
    changed = np.nonzero((f_n != f_src).any(axis=1))[0]
    assert np.array_equal(changed, wet), (changed, wet)
    # whole writes of unequal values stay in array mode; of equal values they restart
    op.set_domain_mannings_n(cur.mannings, ordered=True)
    op.set_domain_external_source(0, cur.ext_src[:, 0])
    step("whole writes of unequal values", 0)
    cur.mannings[:] = 0.025
    op.set_domain_mannings_n(cur.mannings, ordered=True)
    cur.ext_src[:, 0] = 1e-5
    op.set_domain_external_source(0, cur.ext_src[:, 0])
    step("whole writes of equal values", both)
    # values the host cannot see end the mode
    op.refresh_field(2, torch.tensor(cur.mannings, dtype=torch.float64, device="cuda"))
    d_data = torch.tensor(cur.ext_src[:, 0].copy(), dtype=torch.float64, device="cuda")
    d_map = torch.arange(no, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().rdyhip_forcing_gather_source(op._h, 0, no, None, _ptr(d_data), _ptr(d_map), 1, 0, 1.0, _stream()))
    step("device-side writes", 0)
    op.refresh_field(2, cur.mannings)
    op.set_domain_external_source(0, cur.ext_src[:, 0], ordered=True)
    step("host writes again", both)
    # the writable pointer ends a field's mode for good
    assert op.mannings_n.shape[0] == no
    assert op.uniform_fields() == UNIFORM_SOURCE
    op.set_domain_mannings_n(cur.mannings)
    step("Manning's n has escaped", UNIFORM_SOURCE)
    op.destroy()


def test_stream_ordered_setters_between_launches(monkeypatch):
    """launch, set_*_on with a new value, launch -- on one stream with nothing between them that waits: each launch computes with
    its own value (the first must not see the second's element 0)"""
    torch = _torch()
    base, f0 = _case("tri7000", "first")
    _env(monkeypatch, MESHES["tri7000"][1])
    no = base.mesh.num_owned_cells
    second = dataclasses.replace(base, mannings=np.full(no, 0.04), ext_src=base.ext_src.copy())
    second.ext_src[:, 0] = 6e-4
    op = CS.create_operator(base)
    u = torch.tensor(base.u_local, dtype=torch.float64, device="cuda")
    f1 = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
    f2 = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
    both = UNIFORM_SOURCE | UNIFORM_MANNINGS
    torch.cuda.synchronize()
    op.rhs_function(base.dt, u, f1)
    op.set_domain_mannings_n(second.mannings, ordered=True)
    op.set_domain_external_source(0, second.ext_src[:, 0], ordered=True)
    assert op.uniform_fields() == both
    op.rhs_function(base.dt, u, f2)
    torch.cuda.synchronize()
    c2 = _courant(op)
    r1 = _check_oracle(base, "rhs", f0, (f1.cpu().numpy(), None, oracle_courant(base)), "first launch")
    r2 = _check_oracle(second, "rhs", f0, (f2.cpu().numpy(), None, c2), "second launch")
    assert not np.array_equal(r1, r2)
    # and bit for bit what operators that never saw the other value compute
    for case, f in ((base, f1), (second, f2)):
        ref = CS.create_operator(case)
        assert np.array_equal(_evaluate(ref, case, "rhs", False, f0, u)[0], f.cpu().numpy())
        ref.destroy()
    op.destroy()


def oracle_courant(case):
    orc = oracle_from_case(case)
    orc.apply(case.dt, case.u_local)
    return tuple(orc.diagnostics())
