"""GPU: ensembles (rdyhip_ensemble_*, csrc/ensemble_kernels.h) against the C oracle, one oracle per member.

Every member's inputs come from random_case(np.random.default_rng(seed_m), mesh, cfg): the condition types depend on the boundary
index only and are shared, the state, Manning's n, sources, Dirichlet values and dt differ per member.  The meshes are those of
test_gpu_tracers.py, chosen where the indexing can go wrong: 30 cells (under one wave), 270 (two workgroups and a partial wave),
the 44 quads of planar_dam_10x5.msh, the mixed mesh (empty fourth slots), one rank's part of a random partition (about 1 000
owned cells, ghosts interleaved), 8 192 triangles for a member count that the group count chosen at enable does not divide, and
38 448 quads and triangles with 50 members, where a thread walks eight of them.
Bars: 1e-10 (helpers.rel_linf, what test_gpu_parity.py holds the RHS to) for F and the boundary fluxes, 1e-12 for the Courant
number, exact ids, bits for the Euler step, for a member among others and for the undisturbed SWE path."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

from helpers import interior_courant_numbers, oracle_from_case, rel_linf
from random_cases import random_case, random_mixed_mesh
from rdycore_amd import _lib
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import (COMPONENT_H, COMPONENT_HV, Operator, RDyFlowConfig, RDyHipError, SOURCE_IMPLICIT_XQ2018, SOURCE_SEMI_IMPLICIT,
                                  WELL_BALANCING_HR)
from rdycore_amd.timestep import EnsembleEulerStepper
from test_gpu_tracers import _bathymetry, _empty_mesh, _mesh

pytestmark = pytest.mark.gpu

TOL = 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MESHES = ["tri-30", "tri-270", "quad-44", "mixed", "part-o2l"]
SOURCES = [SOURCE_SEMI_IMPLICIT, SOURCE_IMPLICIT_XQ2018]
GRAVITY = 9.806


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(a):
    return _torch().tensor(np.ascontiguousarray(a), dtype=_torch().float64, device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _big_mesh():
    mesh = M.structured_tri_mesh(64, 64, 1.0, zfunc=_bathymetry)
    assert mesh.num_owned_cells == 8192
    return mesh


@functools.lru_cache(maxsize=None)
def _big_mixed_mesh():
    mesh = random_mixed_mesh(np.random.default_rng(3), 160, 160)
    assert 128 * 256 < mesh.num_owned_cells < 160 * 256 and (mesh.cell_nverts == 3).any() and (mesh.cell_nverts == 4).any()
    return mesh


def _get_mesh(name):
    return {"tri-8192": _big_mesh, "mixed-38k": _big_mixed_mesh}[name]() if name in ("tri-8192", "mixed-38k") else _mesh(name)


def _config(name, src):
    return RDyFlowConfig(source_method=src, h_anuga_regular=1e-3 if name == "quad-44" else 0.0)


def boundary_courant_numbers(case):
    """Per boundary edge (in the order of the boundaries' edge lists): the Courant number the reference's boundary-flux loop forms
    (src/swe/swe_petsc.c:549-603), restated in numpy like helpers.interior_courant_numbers -- only the largest wave speed is
    needed.  NaN where the edge is skipped (both sides dry)."""
    m, cfg = case.mesh, case.config
    out = []

    def vel(h, hu, hv):
        den = h * h + cfg.h_anuga_regular ** 2
        with np.errstate(all="ignore"):
            return np.where(h < cfg.tiny_h, 0.0, hu * h / den), np.where(h < cfg.tiny_h, 0.0, hv * h / den)
    for b, bnd in enumerate(m.boundaries):
        e = np.asarray(bnd.edge_ids)
        l = m.edge_cell_ids[2 * e]
        cn, sn = m.edge_cn[e], m.edge_sn[e]
        hl = case.u_local[l, 0].copy()
        ul, vl = vel(hl, case.u_local[l, 1], case.u_local[l, 2])
        t = case.condition_types[b]
        if t == M.CONDITION_DIRICHLET:
            bv = case.boundary_values[b]
            hr = bv[:, 0]
            ur, vr = vel(hr, bv[:, 1], bv[:, 2])
        elif t == M.CONDITION_REFLECTING:
            d1, d2 = sn * sn - cn * cn, 2.0 * sn * cn
            hr, ur, vr = hl, ul * d1 - vl * d2, -ul * d2 - vl * d1
        else:
            uperp = ul * cn + vl * sn
            back = uperp < 0.0
            q = hl * np.abs(uperp)
            hr = np.where(back, 0.0, np.cbrt(q * q / GRAVITY))
            cr = np.sqrt(GRAVITY * hr)
            ur, vr = cr * cn, cr * sn
            hl, ul, vl = np.where(back, 0.0, hl), np.where(back, 0.0, ul), np.where(back, 0.0, vl)
        skip = (hl < cfg.tiny_h) & (hr < cfg.tiny_h)
        with np.errstate(all="ignore"):
            dl, dr = np.sqrt(hl), np.sqrt(hr)
            uhat, vhat = (dl * ul + dr * ur) / (dl + dr), (dl * vl + dr * vr) / (dl + dr)
            amax = np.sqrt(0.5 * GRAVITY * (hl + hr)) + np.abs(uhat * cn + vhat * sn)
            c = amax * m.edge_lengths[e] / m.cell_areas[l] * case.dt
        out.append(np.where(skip, np.nan, c))
    return np.concatenate(out) if out else np.zeros(0)


@functools.lru_cache(maxsize=None)
def _member(name, src, seed):
    """(case, F, boundary fluxes, (Courant number, edge, cell)) of one member from the oracle: computed once, shared, left unchanged"""
    mesh = _get_mesh(name)
    case = random_case(np.random.default_rng(seed), mesh, _config(name, src), region_block=16 if name == "tri-270" else 0)
    orc = oracle_from_case(case)
    F = orc.apply(case.dt, case.u_local)
    assert np.isfinite(F).all()
    bf = [np.array(b) for b in orc.boundary_fluxes]
    diag = orc.diagnostics()
    assert diag[0] > 0.0
    if mesh.num_cells == mesh.num_owned_cells:
        # no near tie: the restated Courant numbers reproduce the oracle's maximum, and the runner-up is clearly below it
        c = np.concatenate([interior_courant_numbers(case), boundary_courant_numbers(case)])
        c = np.sort(c[np.isfinite(c)])
        assert abs(c[-1] - diag[0]) <= 1e-12 * max(1.0, diag[0]), (name, src, seed, c[-1], diag[0])
        assert c[-1] - c[-2] > 1e-9 * c[-1], f"{name} seed {seed}: the state has a near tie: choose another seed"
    orc.close()
    for a in [case.u_local, case.mannings, case.ext_src, F] + bf:
        a.setflags(write=False)
    return case, F, bf, diag


# seeds whose state has two edges at the largest Courant number (on the regular quads of planar_dam_10x5.msh a wet cell between
# two dry ones sees the same wave speed through two opposite edges): _member refuses them, the members skip them
TIED_SEEDS = {7705}


def _seeds(name, src, B, first=0):
    base = 7000 + 100 * len(name) + 10 * src + first
    return [s for s in range(base, base + B + len(TIED_SEEDS)) if s not in TIED_SEEDS][:B]


def _members(name, src, B, first=0):
    return [_member(name, src, s) for s in _seeds(name, src, B, first)]


def _set_member(op, m, case):
    op.ensemble_set_mannings_n(m, case.mannings)
    for comp in range(3):
        op.ensemble_set_external_source(m, comp, case.ext_src[:, comp])
    for b, vals in case.boundary_values.items():
        op.ensemble_set_boundary_values(m, b, vals)


def _operator(name, src, members):
    """an operator on the members' mesh with none of its own inputs set, the ensemble enabled and every member's inputs set"""
    case0 = members[0][0]
    op = Operator.create(case0.config, case0.mesh, case0.condition_types)
    op.enable_ensemble(len(members))
    assert op.ensemble_info() == len(members)
    for m, (case, _, _, _) in enumerate(members):
        assert case.condition_types == case0.condition_types
        _set_member(op, m, case)
    return op


def _groups(B, num_owned):
    """the rule of rdyhip_ensemble_enable: (groups, members per group) for B members on a mesh of num_owned cells
    (from 64 workgroups on, the cell-centric launch rounds its workgroup count up to a multiple of 8)"""
    blocks = (num_owned + 255) // 256
    if blocks >= 64:
        blocks = 8 * ((blocks + 7) // 8)
    g0 = min(B, max(1, (1024 + blocks - 1) // blocks))
    per = min((B + g0 - 1) // g0, 8)
    return (B + per - 1) // per, per


def _check_euler_sample(op, members, ud, Fd, rows=40):
    """the fused Euler step of all members against one exact fused multiply-add of the F just evaluated, on `rows` owned rows per
    member (every row on the small meshes is test_euler_step_is_one_fused_multiply_add_of_the_rhs); F stored by it: the same bits"""
    torch = _torch()
    mesh = members[0][0].mesh
    B = len(members)
    own = np.asarray(mesh.cell_owned_to_local)
    out = torch.full((B, mesh.num_cells, 3), -777.0, dtype=torch.float64, device="cuda")
    f2 = torch.full((B, mesh.num_owned_cells, 3), float("nan"), dtype=torch.float64, device="cuda")
    op.ensemble_euler_step([c.dt for c, _, _, _ in members], ud, out, f2)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(_bits(f2.cpu().numpy()), _bits(Fd))
    assert np.isfinite(o[:, own]).all()
    pick = np.random.default_rng(11).choice(mesh.num_owned_cells, size=min(rows, mesh.num_owned_cells), replace=False)
    for m, (case, _, _, _) in enumerate(members):
        want = np.array([[float(Fraction(case.dt) * Fraction(float(Fd[m, r, k])) + Fraction(float(case.u_local[own[r], k]))) for k in range(3)]
                         for r in pick])
        assert np.array_equal(_bits(o[m, own[pick]]), _bits(want)), m


def _check_parity(name, src, B, euler=False):
    torch = _torch()
    members = _members(name, src, B)
    mesh = members[0][0].mesh
    op = _operator(name, src, members)
    u = _dev(np.stack([c.u_local for c, _, _, _ in members]))
    dts = [c.dt for c, _, _, _ in members]
    f = torch.full((B, mesh.num_owned_cells, 3), float("nan"), dtype=torch.float64, device="cuda")   # every owned row of every member is written
    op.ensemble_rhs_function(dts, u, f)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    assert np.isfinite(got).all()
    op.ensemble_update_diagnostics()
    diags = op.ensemble_get_diagnostics()
    assert len(diags) == B
    for m, (case, F, bf, (cmax, edge, cell)) in enumerate(members):
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
        _check_euler_sample(op, members, u, got)
    op.destroy()


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("B", [1, 3, 7])
@pytest.mark.parametrize("name", MESHES)
def test_rhs_boundary_fluxes_and_courant_of_every_member(name, B, src):
    _check_parity(name, src, B)


@pytest.mark.parametrize("src", SOURCES)
def test_sixty_four_members_under_one_wave(src):
    _check_parity("tri-30", src, 64)


def test_a_member_count_the_group_count_does_not_divide():
    """33 members on 32 workgroups of cells: 32 groups would do, two members each make 17, and the last group holds one"""
    groups, per = _groups(33, 8192)
    assert (groups, per) == (17, 2) and 33 % groups != 0 and 33 - (groups - 1) * per == 1
    _check_parity("tri-8192", SOURCE_SEMI_IMPLICIT, 33, euler=True)


def test_eight_members_per_thread_on_quads_and_triangles():
    """50 members on 152 workgroups of a mixed mesh (quads, and triangles with an empty fourth slot), XQ2018: seven groups would
    give 1024 workgroups, eight members each is the cap, so six groups walk eight members and the seventh two.  F, boundary
    fluxes, Courant numbers and ids of all 50 against their oracles, then the fused Euler step"""
    groups, per = _groups(50, _big_mixed_mesh().num_owned_cells)
    assert (groups, per) == (7, 8) and 50 - (groups - 1) * per == 2
    _check_parity("mixed-38k", SOURCE_IMPLICIT_XQ2018, 50, euler=True)


def test_a_member_does_not_feel_the_others():
    """the same inputs as member 0 of B = 1 and as member 5 of B = 7: F, boundary fluxes and the Courant value are the same bits"""
    torch = _torch()
    name, src = "tri-270", SOURCE_SEMI_IMPLICIT
    seven = _members(name, src, 7)
    case = seven[5][0]
    mesh = case.mesh
    res = []
    for members, m in (([seven[5]], 0), (seven, 5)):
        op = _operator(name, src, members)
        B = len(members)
        f = torch.full((B, mesh.num_owned_cells, 3), float("nan"), dtype=torch.float64, device="cuda")
        op.ensemble_rhs_function([c.dt for c, _, _, _ in members], _dev(np.stack([c.u_local for c, _, _, _ in members])), f)
        torch.cuda.synchronize()
        op.ensemble_update_diagnostics()
        d = op.ensemble_get_diagnostics()[m]
        res.append((f[m].cpu().numpy(), [op.ensemble_boundary_fluxes(m, b) for b in range(len(mesh.boundaries))],
                    (d.max_courant_num, d.global_edge_id, d.global_cell_id)))
        op.destroy()
    a, b = res
    assert np.isfinite(a[0]).all() and np.array_equal(_bits(a[0]), _bits(b[0]))
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(_bits(x), _bits(y))
    assert a[2] == b[2] and a[2][0] > 0.0


@pytest.mark.parametrize("name,B,src", [("tri-270", 3, SOURCE_SEMI_IMPLICIT), ("part-o2l", 3, SOURCE_IMPLICIT_XQ2018), ("mixed", 7, SOURCE_SEMI_IMPLICIT)])
def test_euler_step_is_one_fused_multiply_add_of_the_rhs(name, B, src):
    torch = _torch()
    members = _members(name, src, B)
    mesh = members[0][0].mesh
    op = _operator(name, src, members)
    u = np.stack([c.u_local for c, _, _, _ in members])
    dts = [c.dt for c, _, _, _ in members]
    ud = _dev(u)
    f = torch.empty((B, mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.ensemble_rhs_function(dts, ud, f)
    Fd = f.cpu().numpy()
    own = np.asarray(mesh.cell_owned_to_local)
    want = np.array([[[float(Fraction(dts[m]) * Fraction(float(Fd[m, o, k])) + Fraction(float(u[m, c, k]))) for k in range(3)]
                      for o, c in enumerate(own)] for m in range(B)])
    ghost = np.setdiff1d(np.arange(mesh.num_cells), own)
    for with_f in (True, False):
        out = torch.full((B, mesh.num_cells, 3), -777.0, dtype=torch.float64, device="cuda")
        f2 = torch.full((B, mesh.num_owned_cells, 3), float("nan"), dtype=torch.float64, device="cuda") if with_f else None
        op.ensemble_euler_step(dts, ud, out, f2)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(_bits(o[:, own]), _bits(want))
        assert (o[:, ghost] == -777.0).all()                                    # ghost rows are left alone
        if with_f:
            assert np.array_equal(_bits(f2.cpu().numpy()), _bits(Fd))
    assert np.array_equal(_bits(ud.cpu().numpy()), _bits(u))                    # not in place
    with pytest.raises(RDyHipError) as e:
        op.ensemble_euler_step(dts, ud, ud)
    assert e.value.code == 83
    op.destroy()


def test_members_start_with_the_operators_own_inputs():
    """enable copies Manning's n, the source and the boundary values of the operator into every member, and counts its bytes"""
    torch = _torch()
    name, src, B = "tri-270", SOURCE_SEMI_IMPLICIT, 3
    case, F, bf, (cmax, edge, cell) = _member(name, src, _seeds(name, src, 1)[0])
    mesh = case.mesh
    op = CS.create_operator(case)
    assert op.ensemble_info() == 0
    before = op.layout_info()["device_bytes"]
    op.enable_ensemble(B)
    no, K = mesh.num_owned_cells, sum(b.num_edges for b in mesh.boundaries)
    W = 4 * ((no + 255) // 256)                        # one Courant bucket per wave of the cell-centric launch
    assert op.layout_info()["device_bytes"] == before + B * (32 * no + 48 * K + 12 * W + 16)
    f = torch.full((B, no, 3), float("nan"), dtype=torch.float64, device="cuda")
    op.ensemble_rhs_function([case.dt] * B, _dev(np.stack([case.u_local] * B)), f)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    op.ensemble_update_diagnostics()
    for m, d in enumerate(op.ensemble_get_diagnostics()):
        assert rel_linf(got[m], F) <= TOL
        assert np.array_equal(_bits(got[m]), _bits(got[0]))
        for b in range(len(mesh.boundaries)):
            ok = np.isfinite(bf[b]).all(axis=1)
            assert rel_linf(op.ensemble_boundary_fluxes(m, b)[ok], bf[b][ok]) <= TOL
        assert abs(d.max_courant_num - cmax) <= 1e-12 * max(1.0, cmax) and (d.global_edge_id, d.global_cell_id) == (edge, cell)
    # a later change of the operator's own inputs does not reach the members, and an override reaches its member alone
    op.set_domain_mannings_n(np.full(no, 0.5))
    other = _member(name, src, _seeds(name, src, 2)[1])[0]
    _set_member(op, 1, other)
    op.ensemble_rhs_function([case.dt, other.dt, case.dt], _dev(np.stack([case.u_local, other.u_local, case.u_local])), f)
    torch.cuda.synchronize()
    again = f.cpu().numpy()
    assert np.array_equal(_bits(again[0]), _bits(got[0])) and np.array_equal(_bits(again[2]), _bits(got[0]))
    assert rel_linf(again[1], _member(name, src, _seeds(name, src, 2)[1])[1]) <= TOL
    op.destroy()


def test_refusals(rdyhip_kernel):
    _torch()
    lib = _lib.load()
    mesh = _mesh("tri-30")
    case = _member("tri-30", SOURCE_SEMI_IMPLICIT, _seeds("tri-30", SOURCE_SEMI_IMPLICIT, 1)[0])[0]
    no = mesh.num_owned_cells
    vals = np.zeros((64, 3))
    vp = vals.ctypes.data_as(_lib.c_double_p)
    cs = (_lib.RDyHipCourant * 64)()
    b = next(i for i, bnd in enumerate(mesh.boundaries) if bnd.num_edges)
    ne = mesh.boundaries[b].num_edges
    # not enabled: every other call refuses
    op = CS.create_operator(case)
    for rc in (lib.rdyhip_ensemble_set_mannings(op._h, 0, 1, None, vp), lib.rdyhip_ensemble_set_external_source(op._h, 0, 0, 1, None, vp),
               lib.rdyhip_ensemble_set_boundary_values(op._h, 0, b, ne, vp), lib.rdyhip_ensemble_rhs_function(op._h, vp, vp, vp, None),
               lib.rdyhip_ensemble_euler_step(op._h, vp, vp, vp, None, None), lib.rdyhip_ensemble_get_boundary_fluxes(op._h, 0, b, ne, vp),
               lib.rdyhip_ensemble_update_diagnostics(op._h, None), lib.rdyhip_ensemble_get_diagnostics(op._h, cs)):
        assert rc == 83 and b"not enabled" in lib.rdyhip_last_error()
    with pytest.raises(RDyHipError) as e:
        op.ensemble_set_mannings_n(0, np.zeros(no))
    assert e.value.code == 83 and "not enabled" in e.value.message
    # num_members outside 1..64
    for n in (0, -1, 65):
        with pytest.raises(RDyHipError) as e:
            op.enable_ensemble(n)
        assert e.value.code == 83 and op.ensemble_info() == 0
    # a second enable
    op.enable_ensemble(2)
    with pytest.raises(RDyHipError) as e:
        op.enable_ensemble(2)
    assert e.value.code == 83 and "already" in e.value.message and op.ensemble_info() == 2
    # a member, boundary or component index out of range, a wrong num_edges, null arrays
    for m in (-1, 2):
        assert lib.rdyhip_ensemble_set_mannings(op._h, m, 1, None, vp) == 83
        assert lib.rdyhip_ensemble_set_external_source(op._h, m, 0, 1, None, vp) == 83
        assert lib.rdyhip_ensemble_set_boundary_values(op._h, m, b, ne, vp) == 83
        assert lib.rdyhip_ensemble_get_boundary_fluxes(op._h, m, b, ne, vp) == 83
    for comp in (-1, 3):
        assert lib.rdyhip_ensemble_set_external_source(op._h, 0, comp, 1, None, vp) == 83
    for bad in (-1, len(mesh.boundaries)):
        assert lib.rdyhip_ensemble_set_boundary_values(op._h, 0, bad, ne, vp) == 83
        assert lib.rdyhip_ensemble_get_boundary_fluxes(op._h, 0, bad, ne, vp) == 83
    assert lib.rdyhip_ensemble_set_boundary_values(op._h, 0, b, ne + 1, vp) == 83
    assert lib.rdyhip_ensemble_get_boundary_fluxes(op._h, 0, b, ne - 1, vp) == 83
    assert lib.rdyhip_ensemble_set_boundary_values(op._h, 0, b, ne, None) == 83
    assert lib.rdyhip_ensemble_get_boundary_fluxes(op._h, 0, b, ne, None) == 83
    assert lib.rdyhip_ensemble_set_mannings(op._h, 0, 1, None, None) == 83
    assert lib.rdyhip_ensemble_set_external_source(op._h, 0, 0, 1, None, None) == 83
    assert lib.rdyhip_ensemble_rhs_function(op._h, None, vp, vp, None) == 83
    assert lib.rdyhip_ensemble_rhs_function(op._h, vp, None, None, None) == 83
    assert lib.rdyhip_ensemble_euler_step(op._h, None, vp, vp, None, None) == 83
    assert lib.rdyhip_ensemble_euler_step(op._h, vp, None, None, None, None) == 83
    assert lib.rdyhip_ensemble_get_diagnostics(op._h, None) == 83
    # the Python mirror's shape checks
    torch = _torch()
    u = torch.zeros((2, mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    f = torch.zeros((2, no, 3), dtype=torch.float64, device="cuda")
    for args in (([0.1], u, f), ([0.1, 0.1], u[:1], f), ([0.1, 0.1], u, f[:1]), ([0.1, 0.1], u.float(), f), ([0.1, 0.1], u.cpu(), f)):
        with pytest.raises(RDyHipError) as e:
            op.ensemble_rhs_function(*args)
        assert e.value.code == 83
    op.destroy()
    # hydrostatic reconstruction and second order (they exist in the tiled form only: RDYHIP_KERNEL=cell refuses at create)
    pmesh = M.structured_tri_mesh(5, 3, 1.0, zfunc=_bathymetry, project_2d=True)
    for cfg, m in ((RDyFlowConfig(well_balancing=WELL_BALANCING_HR), pmesh), (RDyFlowConfig(second_order=True), mesh)):
        try:
            op = Operator.create(cfg, m)
        except RDyHipError as err:
            assert rdyhip_kernel == "cell" and err.code == 83
            continue
        with pytest.raises(RDyHipError) as e:
            op.enable_ensemble(2)
        assert e.value.code == 83 and op.ensemble_info() == 0
        op.destroy()


@pytest.mark.parametrize("name", ["tri-270", "part-o2l"])
def test_the_swe_path_is_undisturbed(name, rdyhip_kernel):
    """After enable_ensemble -- and an ensemble evaluation -- rdyhip_rhs_function gives the bits of a fresh operator: F, primitive
    variables, boundary fluxes and the Courant struct, under both kernels."""
    torch = _torch()
    src, B = SOURCE_SEMI_IMPLICIT, 3
    members = _members(name, src, B)
    case = members[0][0]
    mesh = case.mesh
    plain = CS.create_operator(case)
    op = CS.create_operator(case)
    op.enable_ensemble(B)
    for m, (c, _, _, _) in enumerate(members):
        _set_member(op, m, c)
    op.ensemble_rhs_function([c.dt for c, _, _, _ in members], _dev(np.stack([c.u_local for c, _, _, _ in members])),
                             torch.empty((B, mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda"))
    u3 = _dev(case.u_local)
    res = []
    for o in (plain, op):
        pv = o.primitive_variables
        f = torch.full((mesh.num_owned_cells, 3), float("nan"), dtype=torch.float64, device="cuda")
        o.rhs_function(case.dt, u3, f)
        torch.cuda.synchronize()
        o.update_diagnostics()
        d = o.get_diagnostics()
        res.append((f.cpu().numpy(), pv.cpu().numpy(), [o.boundary_fluxes(b) for b in range(len(mesh.boundaries))],
                    [o.boundary_fluxes(b, accumulated=True) for b in range(len(mesh.boundaries))],
                    (d.max_courant_num, d.global_edge_id, d.global_cell_id)))
    a, b = res
    assert np.isfinite(a[0]).all() and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        assert np.array_equal(_bits(x), _bits(y))
    assert a[4] == b[4] and a[4][0] > 0.0
    plain.destroy()
    op.destroy()


def test_a_rank_that_owns_nothing():
    torch = _torch()
    mesh = _empty_mesh()
    op = Operator.create(RDyFlowConfig(), mesh)
    op.enable_ensemble(3)
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


def test_the_reference_ensemble_deck():
    """driver/tests/swe_roe/ex2b-ensemble.yaml: two members on planar_dam_10x5.msh with Manning 0.015 and 0.030, the boundaries and
    initial state of ex2b, the semi-implicit source (the deck names none: src/yaml_input.c:859), dt = 0.018 s, 1000 steps through
    EnsembleEulerStepper, against two Euler loops of the oracle at steps 100 and 1000.  The members differ by more than 1e-3 (on
    the CPU the oracle gives 3.8e-3 after 1000 steps), so a kernel that mixes them up cannot pass."""
    torch = _torch()
    base = CS.ex2b_case(os.path.join(GOLDEN, "planar_dam_10x5.msh"))
    mesh = base.mesh
    cfg = RDyFlowConfig(source_method=SOURCE_SEMI_IMPLICIT)
    dt, mann = 0.018, (0.015, 0.030)
    assert abs(base.dt - dt) < 1e-15
    want = {100: [], 1000: []}
    for n in mann:
        case = CS.Case("ex2b-ensemble", mesh, cfg, base.condition_types, base.u_local, np.full(mesh.num_owned_cells, n), base.ext_src, {}, dt)
        orc = oracle_from_case(case)
        u = base.u_local.copy()
        for step in range(1, 1001):
            u = u + dt * orc.apply(dt, u)
            if step in want:
                want[step].append(u.copy())
        orc.close()
    assert rel_linf(want[1000][0], want[1000][1]) > 1e-3
    op = Operator.create(cfg, mesh, base.condition_types)
    op.set_domain_mannings_n(np.full(mesh.num_owned_cells, mann[0]))
    op.enable_ensemble(2)
    op.ensemble_set_mannings_n(1, np.full(mesh.num_owned_cells, mann[1]))      # member 1 overrides the one material that differs
    st = EnsembleEulerStepper(op)
    u = _dev(np.stack([base.u_local, base.u_local]))
    done = 0
    for step in (100, 1000):
        u = st.advance(u, [dt, dt], 1)                   # odd counts, the result handed back: 1 + 99, then 1 + 899
        u = st.advance(u, [dt, dt], step - done - 1)
        done = step
        torch.cuda.synchronize()
        got = u.cpu().numpy()
        for m in range(2):
            err = rel_linf(got[m], want[step][m])
            print(f"step {step} member {m} (n = {mann[m]}): state vs oracle {err:.3e}")
            assert np.isfinite(got[m]).all() and err <= TOL
    assert rel_linf(got[0], got[1]) > 1e-3 and st.step == 1000
    op.destroy()


def test_a_member_slice_is_an_ordinary_state():
    """op.state_planes on member m's slice of the [B, num_cells, 3] array equals the planes of the same rows in an array of their own"""
    torch = _torch()
    name, src, B = "part-o2l", SOURCE_SEMI_IMPLICIT, 3
    members = _members(name, src, B)
    mesh = members[0][0].mesh
    op = _operator(name, src, members)
    u = _dev(np.stack([c.u_local for c, _, _, _ in members]))
    own = np.asarray(mesh.cell_owned_to_local)
    for m in range(B):
        alone = u[m].clone()
        a = op.state_planes(u[m], COMPONENT_H | COMPONENT_HV).cpu().numpy()
        b = op.state_planes(alone, COMPONENT_H | COMPONENT_HV).cpu().numpy()
        assert a.shape == (2, mesh.num_owned_cells) and np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(a), _bits(members[m][0].u_local[own][:, [0, 2]].T))
    op.destroy()
