"""The tile loop's addresses: every unit-stride access of the first-order / HR tiled kernels is a 64-bit scalar base (array + the
tile's first cell / record / halo entry, masked where a field is uniform) plus a 32-bit lane offset (lane_ptr, swe_kernels.h);
lanes without a cell carry undefined rows into the store phase (rows_unset); the Courant tie bounds are read inside the tie
branch.  None of it may change a bit of any result.

Shapes, the smallest at which this can go wrong: 8 triangles (one tile, one partly filled wave), 400 triangles (256 + 144: wave 2
of the second tile holds 16 cells, wave 3 none), 7 000 triangles and 7 020 quads on an 8-workgroup grid (workgroups walk several
tiles: prologue and loop call sites, second record round, partial last tile), 17 000 triangles (175 tiles: XCD chunks, so that
RDYHIP_TILE_WALK chooses between two walks), and one RCB part whose owned cells are not a prefix (o2l, scattered u_out) with
momentum sources (the [owned][3] source rows: the other base and lane stride of the source load).

Each call form -- rhs_function, apply onto a random f, euler_step with and without F; plain, with the primitive variables asked
for, with the flux divergence asked for -- gives F, u_out, pv, fdiv and the Courant struct.  They are the SAME BITS with the
uniform-field modes on and off, on the default grid, under RDYHIP_BLOCKS_PER_CU=3 and under both RDYHIP_TILE_WALK values, and
within 1e-10 (rel L-inf against max(1, |ref|), the bar of test_gpu_parity.py) of the oracle with the oracle's Courant ids.  A
state with exact ties in every tile (the two flat pools of test_gpu_cell_family_numbering.py, 10 tiles) names the oracle's edge
and cell."""
import dataclasses
import functools

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import SOURCE_IMPLICIT_XQ2018, RDyFlowConfig

from helpers import interior_courant_numbers, oracle_from_case, rel_linf
from test_gpu_cell_family_numbering import _assert_a_real_tie, _uniform_case
from test_gpu_kernel_matrix import _KNOB_VARS
from test_gpu_uniform_fields import K, MESHES, _mesh

pytestmark = pytest.mark.gpu
TOL = 1e-10
OPERATORS = ["first", "hr", "xq"]
ENV = {"tri8": {}, "tri400": {}, "tri7000": {"RDYHIP_PGRID": "8"}, "quad7020_flat": {"RDYHIP_PGRID": "8"}, "rcb_part": {},
       "tri17000": {"RDYHIP_PGRID": "8"}}
CALLS = ["rhs", "apply", "euler", "euler_no_f"]
WANTS = ["plain", "pv", "fdiv"]
ALL_VARS = _KNOB_VARS + ("RDYHIP_UNIFORM_FIELDS", "RDYHIP_TILE_WALK")


@pytest.fixture(autouse=True)
def _tiled_kernels_only(rdyhip_kernel):
    if rdyhip_kernel == "cell":
        pytest.skip("a test of the tiled kernels (RDYHIP_KERNEL)")


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _the_mesh(name, project_2d):
    zf = CS.mms_bathymetry(K=K)
    if name == "tri8":
        return M.structured_tri_mesh(2, 2, 1.0, zfunc=zf, project_2d=project_2d), 2.0, 2.0
    if name == "tri17000":
        return M.structured_tri_mesh(100, 85, 1.0, zfunc=zf, project_2d=project_2d), 100.0, 85.0
    assert name in MESHES
    return _mesh(name, project_2d)


@functools.lru_cache(maxsize=None)
def _case(name, operator):
    """the friction / slope case (a dry disc, one boundary of each type) with ONE Manning's n and ONE water source, so that the
    uniform modes are on unless switched off; the RCB part has momentum sources as well (no mode for the source there)"""
    hr = operator == "hr"
    mesh, lx, ly = _the_mesh(name, hr)
    case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2, K=K, source_method=SOURCE_IMPLICIT_XQ2018 if operator == "xq" else 0)
    case.config = RDyFlowConfig(source_method=case.config.source_method, well_balancing=2 if hr else 0)
    case.mannings = np.full(mesh.num_owned_cells, 0.015)
    rng = np.random.default_rng(len(name) + 11 * OPERATORS.index(operator))
    if name == "rcb_part":
        case = dataclasses.replace(case, ext_src=case.ext_src.copy())
        case.ext_src[:, 1:] = rng.normal(size=(mesh.num_owned_cells, 2)) * 1e-3
    f0 = rng.normal(size=(mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0])
    return case, f0


@functools.lru_cache(maxsize=None)
def _oracle(name, operator, accumulate):
    """(F, pv, fdiv, Courant) of the oracle: computed once per case, shared and left unchanged"""
    case, f0 = _case(name, operator)
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local, f0.copy() if accumulate else None)
    assert np.isfinite(fr).all()
    out = (fr.copy(), orc.primitive_variables.copy(), orc.flux_divergence.copy(), tuple(orc.diagnostics()))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _set_env(monkeypatch, env):
    for k in ALL_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _evaluate(case, f0, call, want):
    """one evaluation on a new operator: {F, u_out, pv, fdiv, courant} on the host (None where the call leaves none)"""
    torch = _torch()
    no = case.mesh.num_owned_cells
    op = CS.create_operator(case)
    assert op.layout_info()["tiled_kernel"] == 1
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    pv = None
    if want == "pv":
        pv = op.primitive_variables          # asked for: evaluations store them from here on
        pv.fill_(555.0)
    if want == "fdiv":
        op.enable_flux_divergence(True)
    f = torch.tensor(f0, dtype=torch.float64, device="cuda") if call == "apply" else torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
    out = None
    if call in ("euler", "euler_no_f"):
        out = torch.full_like(u, -7.0)
        if call == "euler_no_f":
            f = None
        op.euler_step(case.dt, u, out, f)
    elif call == "rhs":
        op.rhs_function(case.dt, u, f)
    else:
        op.reset_diagnostics()
        op.apply(case.dt, u, f)
    torch.cuda.synchronize()
    op.update_diagnostics()
    d = op.get_diagnostics()
    res = {"F": f.cpu().numpy() if f is not None else None, "u_out": out.cpu().numpy() if out is not None else None,
           "pv": pv.cpu().numpy() if pv is not None else None,
           "fdiv": op.flux_divergence.cpu().numpy() if want == "fdiv" else None,
           "courant": (d.max_courant_num, d.global_edge_id, d.global_cell_id)}
    op.destroy()
    return res


def _same_bits(a, b, what):
    for k in ("F", "u_out", "pv", "fdiv"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs, first at row {np.nonzero((a[k] != b[k]).any(axis=1))[0][:5]}"
    assert a["courant"] == b["courant"], f"{what}: the Courant struct differs: {a['courant']} / {b['courant']}"


def _check_oracle(name, operator, call, res, what):
    case, f0 = _case(name, operator)
    fr, pvr, fdr, cref = _oracle(name, operator, call == "apply")
    if res["F"] is not None:
        err = rel_linf(res["F"], fr)
        print(f"{what}: F rel L-inf vs oracle {err:.3e}")
        assert err <= TOL, (what, err)
    if res["u_out"] is not None:
        own = case.mesh.cell_owned_to_local
        err = rel_linf(res["u_out"][own], case.u_local[own] + case.dt * fr)
        print(f"{what}: u_out rel L-inf vs oracle {err:.3e}")
        assert err <= TOL, (what, err)
        assert np.all(res["u_out"][case.mesh.cell_is_owned == 0] == -7.0), f"{what}: ghost rows of u_out were written"
    if res["pv"] is not None:
        err = rel_linf(res["pv"], pvr)
        print(f"{what}: pv rel L-inf vs oracle {err:.3e}")
        assert err <= TOL, (what, err)
    if res["fdiv"] is not None:
        # (of an apply onto f it holds f as well, here and in the oracle: the copy is taken before the source terms)
        err = rel_linf(res["fdiv"], fdr)
        print(f"{what}: fdiv rel L-inf vs oracle {err:.3e}")
        assert err <= TOL, (what, err)
    c = res["courant"]
    assert abs(c[0] - cref[0]) <= 1e-12 * max(1.0, cref[0]) and c[1:] == tuple(cref[1:]), (what, c, cref)


def _variants(name):
    """environment of the base configuration and of everything that must give its bits"""
    base = dict(ENV[name])
    free = {k: v for k, v in base.items() if k != "RDYHIP_PGRID"}
    return base, {"uniform fields off": {**base, "RDYHIP_UNIFORM_FIELDS": "0"}, "default grid": free,
                  "three workgroups per CU": {**free, "RDYHIP_BLOCKS_PER_CU": "3"},
                  "static walk": {**base, "RDYHIP_TILE_WALK": "static"}, "dynamic walk": {**base, "RDYHIP_TILE_WALK": "dynamic"}}


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("name", ["tri8", "tri400", "tri7000", "quad7020_flat", "rcb_part"])
def test_every_call_form_same_bits_in_every_configuration_and_the_oracles_values(name, operator, monkeypatch):
    case, f0 = _case(name, operator)
    base, variants = _variants(name)
    _set_env(monkeypatch, base)
    op = CS.create_operator(case)
    info = op.layout_info()
    op.destroy()
    no = case.mesh.num_owned_cells
    if name == "tri8":
        assert no == 8 and info["num_tiles"] == 1
    elif name == "tri400":
        assert no == 400 and info["num_tiles"] == 2
    elif name == "rcb_part":
        assert info["owned_is_prefix"] == 0 and case.mesh.num_cells > no and np.any(case.ext_src[:, 1:] != 0)
    else:
        assert no == (7000 if name == "tri7000" else 7020) and info["persistent_grid"] == 8 and info["num_tiles"] >= 3 * 8 and no % 256 != 0
    for call in CALLS:
        for want in WANTS:
            _set_env(monkeypatch, base)
            ref = _evaluate(case, f0, call, want)
            what = f"{name} {operator} {call} {want}"
            _check_oracle(name, operator, call, ref, what)
            for tag, env in variants.items():
                _set_env(monkeypatch, env)
                _same_bits(ref, _evaluate(case, f0, call, want), f"{what} / {tag}")


@pytest.mark.parametrize("operator", ["first", "hr"])
def test_both_tile_walks_same_bits_on_xcd_chunks(operator, monkeypatch):
    """175 tiles in eight XCD ranges on eight workgroups: under RDYHIP_TILE_WALK=dynamic each workgroup draws its tiles from its
    range's counter after its first three (the kernels that have the walk: rhs_function and apply; plain, with pv, with fdiv)"""
    case, f0 = _case("tri17000", operator)
    res = {}
    for walk in ("static", "dynamic"):
        _set_env(monkeypatch, {**ENV["tri17000"], "RDYHIP_TILE_WALK": walk})
        op = CS.create_operator(case)
        info = op.layout_info()
        op.destroy()
        assert info["num_tiles"] == 175 and info["persistent_grid"] == 8      # >= 64 tiles: XCD ranges; not a multiple of 8
        res[walk] = {(call, want): _evaluate(case, f0, call, want) for call in ("rhs", "apply") for want in WANTS}
    for key in res["static"]:
        call, want = key
        _same_bits(res["static"][key], res["dynamic"][key], f"tri17000 {operator} {call} {want}: static / dynamic walk")
        _check_oracle("tri17000", operator, call, res["dynamic"][key], f"tri17000 {operator} {call} {want} dynamic walk")


@pytest.mark.parametrize("call", ["rhs", "euler"])
def test_exact_ties_in_every_tile_name_the_oracles_edge_and_cell(call, monkeypatch):
    """two flat pools at rest on 2 400 renumbered triangles (10 tiles): hundreds of edges reach the maximum bit for bit, every
    tile runs the tie branch -- which now reads its own two bounds -- and the winner is the reference's first edge in loop order"""
    case = _uniform_case("tri-small", "pools", 1e-3)
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local)
    cmax, edge, cell = orc.diagnostics()
    ties = _assert_a_real_tie(case.mesh, interior_courant_numbers(case), cmax, edge, cell)
    print(f"{ties} internal edges tie at {cmax!r}; the oracle's edge {edge}, cell {cell}")
    f0 = np.zeros((case.mesh.num_owned_cells, 3))
    got = {}
    for tag, env in {"default": {}, "two workgroups": {"RDYHIP_PGRID": "2"}, "uniform fields off": {"RDYHIP_UNIFORM_FIELDS": "0"}}.items():
        _set_env(monkeypatch, env)
        got[tag] = _evaluate(case, f0, call, "plain")
        c = got[tag]["courant"]
        assert abs(c[0] - cmax) <= 1e-12 * max(1.0, cmax) and c[1:] == (edge, cell), (tag, c, (cmax, edge, cell))
        assert rel_linf(got[tag]["F"], fr) <= TOL
    _same_bits(got["default"], got["two workgroups"], "ties: default / two workgroups")
    _same_bits(got["default"], got["uniform fields off"], "ties: modes on / off")
