"""The normal table: where the tile edge records of an operator have at most 64 distinct normals, its first-order / HR launches
run the table family (swe_rhs_ntab_kernel: the (cn, sn) pairs of the table's entries in LDS, a record's index in bits 26-31 of
its word, e_cs not read) instead of the streamed one (swe_rhs_tiled_kernel).  The table's pairs come from the same edge_normal
on the same operands, so nothing may change a bit: every case here compares the table family against the same operator created
with streamed_normals=True BIT FOR BIT -- F, u_out, pv, fdiv, the Courant struct -- and holds it to the oracle (rel L-inf <=
1e-10 against max(1, |ref|), the bar of test_gpu_parity.py, with the oracle's Courant ids).

Shapes and configurations are those of test_gpu_tile_loop_addressing.py (its cases, oracle values and evaluation are imported):
8 triangles (one tile, fewer records than lanes and than table entries' 64), 400, 7 000 triangles and 7 020 quads on an
8-workgroup grid (both record rounds, >= 28 tiles), an RCB part with o2l, ghosts and momentum sources in one call and in the
INTERIOR + HALO phases; first order, HR, XQ2018; rhs_function, apply onto a random f, euler_step with and without F; plain,
with pv, with fdiv; uniform fields on / off, RDYHIP_BLOCKS_PER_CU=3; 17 000 triangles under both RDYHIP_TILE_WALK values; exact
ties in every tile of 2 400 renumbered triangles.

The table's limits: a strip whose rows have different heights has its own diagonal normals in every row -- 64 keys (counted
here in numpy by the rule of the layout pass) run the table, 65 stream; a randomly perturbed mesh streams.

The streamed family keeps a GPU check of its own now that structured meshes run the table: every row of
test_gpu_kernel_matrix.ROWS that names a tiled kernel runs once more with streamed_normals=True, on a structured mesh -- where
the default would be the table -- against the oracle."""
import dataclasses
import functools

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig

from helpers import interior_courant_numbers, oracle_from_case, rel_linf
from random_cases import random_case, random_tri_mesh
from test_gpu_cell_family_numbering import _assert_a_real_tie, _uniform_case
from test_gpu_kernel_matrix import ROWS, check_against_oracle, row_kernel, run_device, run_oracle
from test_gpu_tile_loop_addressing import CALLS, ENV, OPERATORS, WANTS, _case, _check_oracle, _evaluate, _same_bits, _set_env
import test_gpu_uniform_fields as UF

pytestmark = pytest.mark.gpu
TOL = 1e-10
NORMAL_TABLE_MAX = 64


@pytest.fixture(autouse=True)
def _tiled_kernels_only(rdyhip_kernel):
    if rdyhip_kernel == "cell":
        pytest.skip("a test of the tiled kernels (RDYHIP_KERNEL)")


def key_count(mesh):
    """distinct (bit pattern of the stored component, CS_IS_CN, OTHER_NEG) over all edges: the rule of the layout pass (the
    stored component is the one of smaller magnitude, cn on a tie; the other one's sign bit is kept)"""
    cn, sn = np.ascontiguousarray(mesh.edge_cn, dtype=np.float64), np.ascontiguousarray(mesh.edge_sn, dtype=np.float64)
    is_cn = np.abs(cn) <= np.abs(sn)
    cs, other = np.where(is_cn, cn, sn), np.where(is_cn, sn, cn)
    return len(set(zip(cs.view(np.uint64).tolist(), is_cn.tolist(), np.signbit(other).tolist())))


def _streamed(case):
    return dataclasses.replace(case, config=dataclasses.replace(case.config, streamed_normals=True))


def _table_info(case):
    op = CS.create_operator(case)
    info = op.normal_table_info()
    op.destroy()
    return info


# ---- every call form, every configuration ----------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("name", ["tri8", "tri400", "tri7000", "quad7020_flat", "rcb_part"])
def test_table_and_streamed_normals_same_bits_and_the_oracles_values(name, operator, monkeypatch):
    case, f0 = _case(name, operator)
    streamed = _streamed(case)
    base = dict(ENV[name])
    free = {k: v for k, v in base.items() if k != "RDYHIP_PGRID"}
    _set_env(monkeypatch, base)
    entries, active = _table_info(case)
    # every edge of these meshes touches an owned cell, except on the part, whose records are a subset
    nkeys = key_count(case.mesh)
    assert active and (entries == nkeys if name != "rcb_part" else 1 <= entries <= nkeys) and nkeys <= 8, (entries, active, nkeys)
    assert _table_info(streamed) == (0, False)
    if name == "tri8":
        op = CS.create_operator(case)
        assert op.layout_info()["num_tiles"] == 1 and op.layout_info()["num_edge_records"] < NORMAL_TABLE_MAX
        op.destroy()
    for call in CALLS:
        for want in WANTS:
            what = f"{name} {operator} {call} {want}"
            _set_env(monkeypatch, base)
            tab = _evaluate(case, f0, call, want)
            _check_oracle(name, operator, call, tab, what + " / table")
            _same_bits(tab, _evaluate(streamed, f0, call, want), what + ": table / streamed")
            for tag, env in {"uniform fields off": {**base, "RDYHIP_UNIFORM_FIELDS": "0"}, "three workgroups per CU": {**free, "RDYHIP_BLOCKS_PER_CU": "3"}}.items():
                _set_env(monkeypatch, env)
                _same_bits(tab, _evaluate(case, f0, call, want), f"{what}: table / table, {tag}")


@pytest.mark.parametrize("operator", OPERATORS)
def test_interior_and_halo_phases_on_a_part_with_ghosts(operator, monkeypatch):
    """the RCB part (o2l, scattered u_out, momentum sources): INTERIOR then HALO launches -- the tile-skipping static walk and the
    halo tile list -- of the table family against the streamed one and the oracle"""
    case, f0 = _case("rcb_part", operator)
    assert case.mesh.num_cells > case.mesh.num_owned_cells and np.any(case.ext_src[:, 1:] != 0)
    for call in ("rhs", "apply", "euler"):
        res = {}
        for tag, c in {"table": case, "streamed": _streamed(case)}.items():
            _set_env(monkeypatch, {})
            op = CS.create_operator(c)
            assert op.normal_table_info()[1] == (tag == "table") and op.layout_info()["owned_is_prefix"] == 0
            res[tag] = UF._evaluate(op, c, call, True, f0)
            op.destroy()
        UF._same_bits(res["table"], res["streamed"], f"rcb_part {operator} {call} phased: table / streamed")
        UF._check_oracle(case, call, f0, res["table"], f"rcb_part {operator} {call} phased / table")


@pytest.mark.parametrize("operator", ["first", "hr"])
def test_both_tile_walks_on_xcd_chunks(operator, monkeypatch):
    """175 tiles in eight XCD ranges on eight workgroups, static and dynamic walk"""
    case, f0 = _case("tri17000", operator)
    streamed = _streamed(case)
    for walk in ("static", "dynamic"):
        _set_env(monkeypatch, {**ENV["tri17000"], "RDYHIP_TILE_WALK": walk})
        assert _table_info(case) == (key_count(case.mesh), True)
        for call in ("rhs", "apply"):
            for want in WANTS:
                what = f"tri17000 {operator} {call} {want} {walk} walk"
                tab = _evaluate(case, f0, call, want)
                _check_oracle("tri17000", operator, call, tab, what + " / table")
                _same_bits(tab, _evaluate(streamed, f0, call, want), what + ": table / streamed")


@pytest.mark.parametrize("call", ["rhs", "euler"])
def test_exact_ties_in_every_tile_name_the_oracles_edge_and_cell(call, monkeypatch):
    """two flat pools at rest on 2 400 renumbered triangles: every tile runs the tie branch; the oracle's edge and cell come out"""
    case = _uniform_case("tri-small", "pools", 1e-3)
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local)
    cmax, edge, cell = orc.diagnostics()
    _assert_a_real_tie(case.mesh, interior_courant_numbers(case), cmax, edge, cell)
    f0 = np.zeros((case.mesh.num_owned_cells, 3))
    _set_env(monkeypatch, {})
    assert _table_info(case) == (key_count(case.mesh), True)
    got = {tag: _evaluate(c, f0, call, "plain") for tag, c in {"table": case, "streamed": _streamed(case)}.items()}
    for tag, r in got.items():
        c = r["courant"]
        assert abs(c[0] - cmax) <= 1e-12 * max(1.0, cmax) and c[1:] == (edge, cell), (tag, c, (cmax, edge, cell))
        assert rel_linf(r["F"], fr) <= TOL
    _same_bits(got["table"], got["streamed"], "ties: table / streamed")


# ---- the table's limits -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _strip_mesh(nx, ny):
    """nx x ny squares cut into triangles, row j stretched to the height 1 + j / 32: its diagonals have normals of their own"""
    xyz, conn, _, _ = M.structured_tri_connectivity(nx, ny)
    y = np.concatenate([[0.0], np.cumsum(1.0 + np.arange(ny) / 32.0)])
    xyz[:, 1] = y[np.round(xyz[:, 1]).astype(int)]
    xyz[:, 2] = 0.05 * np.sin(0.3 * xyz[:, 0]) * np.cos(0.2 * xyz[:, 1])
    return M.build_mesh(xyz, conn, boundary_classifier=M.box_side_boundaries(0.0, float(nx), 0.0, float(y[-1]))), float(nx), float(y[-1])


def _limit_case(mesh, lx, ly):
    case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2, K=UF.K)
    case.config = RDyFlowConfig()
    return case


@pytest.mark.parametrize("shape,keys", [((3, 30), 64), ((1, 60), 64), ((1, 61), 65), ((3, 31), 66)])
def test_sixty_four_normals_are_a_table_and_sixty_five_are_streamed(shape, keys, monkeypatch):
    _set_env(monkeypatch, {})
    mesh, lx, ly = _strip_mesh(*shape)
    assert key_count(mesh) == keys
    case = _limit_case(mesh, lx, ly)
    f0 = np.zeros((mesh.num_owned_cells, 3))
    assert _table_info(case) == ((keys, True) if keys <= NORMAL_TABLE_MAX else (0, False))
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local)
    cref = tuple(orc.diagnostics())
    got = {tag: _evaluate(c, f0, "rhs", "plain") for tag, c in {"default": case, "streamed": _streamed(case)}.items()}
    for tag, r in got.items():
        err = rel_linf(r["F"], fr)
        print(f"strip {shape} {tag}: F rel L-inf vs oracle {err:.3e}")
        assert err <= TOL, (tag, err)
        assert abs(r["courant"][0] - cref[0]) <= 1e-12 * max(1.0, cref[0]) and r["courant"][1:] == cref[1:], (tag, r["courant"], cref)
    _same_bits(got["default"], got["streamed"], f"strip {shape}: default / streamed")


def test_a_perturbed_mesh_takes_the_streamed_path(monkeypatch):
    _set_env(monkeypatch, {})
    rng = np.random.default_rng(31)
    mesh = random_tri_mesh(rng, 24, 18)
    assert key_count(mesh) > NORMAL_TABLE_MAX
    case = random_case(rng, mesh, RDyFlowConfig(tiny_h=1e-5))
    assert _table_info(case) == (0, False)
    op, f, out = run_device(case, "rhs", False)
    fr, orc = run_oracle(case)
    check_against_oracle(case, "rhs", op, f, out, fr, orc)
    op.destroy()


def test_second_order_and_the_cell_kernel_have_no_table(monkeypatch):
    _set_env(monkeypatch, {})
    mesh = M.structured_tri_mesh(20, 10, 1.0)
    case = CS.friction_slope_case(mesh, 20.0, 10.0, dt=1e-2, K=UF.K)
    case.config = RDyFlowConfig(second_order=True)
    assert _table_info(case) == (0, False)
    case.config = RDyFlowConfig()
    monkeypatch.setenv("RDYHIP_KERNEL", "cell")
    assert _table_info(case) == (0, False)
    monkeypatch.setenv("RDYHIP_KERNEL", "tiled")
    assert _table_info(case) == (6, True)


# ---- the streamed family on the meshes where the default is now the table ---------------------------------------------------
TILED_ROWS = [r for r in ROWS if r.kernel[0] == "tiled"]


@functools.lru_cache(maxsize=None)
def _matrix_structured_mesh(kind, project_2d):
    zf = CS.mms_bathymetry(K=UF.K)
    if kind == "tri":
        return M.structured_tri_mesh(36, 30, 1.0, zfunc=zf, project_2d=project_2d)
    return M.structured_quad_mesh(50, 44, 1.0, 1.0, zfunc=zf, project_2d=project_2d)


@pytest.mark.parametrize("row", TILED_ROWS, ids=[r.id for r in TILED_ROWS])
def test_streamed_instantiation_against_the_oracle_where_the_table_is_the_default(row, monkeypatch):
    """one streamed launch per (S, SRC, OVW, HR, EULER, FNT) of the table of test_gpu_kernel_matrix.py, its random states and
    fields on a structured mesh of the row's slot count (prefix layout, one call)"""
    assert row_kernel(row) == row.kernel
    _set_env(monkeypatch, {} if row.uout_cached is None else {"RDYHIP_UOUT_CACHED": str(row.uout_cached)})
    rng = np.random.default_rng(7000 + ROWS.index(row))
    mesh = _matrix_structured_mesh("tri" if row.mesh == "tri" else "quad", row.well_balancing == 2)
    cfg = RDyFlowConfig(tiny_h=float(rng.choice([1e-7, 1e-5])), h_anuga_regular=float(rng.choice([0.0, 0.0, 1e-3])),
                        source_method=row.source_method, well_balancing=row.well_balancing, cached_f_stores=row.cached_f_stores,
                        streamed_normals=True)
    case = random_case(rng, mesh, cfg, region_block=int(rng.choice([0, 32, 256])))
    assert _table_info(case) == (0, False)
    assert _table_info(dataclasses.replace(case, config=dataclasses.replace(cfg, streamed_normals=False)))[1]
    f0 = rng.normal(size=(mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0]) if row.call == "apply" else None
    op, f, out = run_device(case, row.call, False, f0=f0, with_f=row.call != "euler" or bool(rng.integers(0, 2)))
    assert op.layout_info()["slots_per_cell"] == row.kernel[1] and op.layout_info()["num_tiles"] >= 4
    fr, orc = run_oracle(case, f0)
    check_against_oracle(case, row.call, op, f, out, fr, orc)
    op.destroy()
