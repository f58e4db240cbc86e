"""GPU: the tracer kernel (csrc/tracer_kernels.h) and the ensemble kernels (csrc/ensemble_kernels.h: the RHS with its shuffle-only
Courant reduction, and the finalize kernel that merges the buckets) under what the drop-in really hands over and in the states
a run really starts from -- what test_gpu_numbering.py and test_gpu_fuzz.py hold the SWE kernels to.

  A  the DMPlex-like numbering (mesh.dmplex_like_numbering and its two halves): Hilbert-permuted cells, edges numbered
     independently of the cells and flipped, so "left" is not the lower-numbered cell and the loop position of an edge owes
     nothing to its cells.
  B  exact ties: a lake at rest and two flat pools, where thousands of edges reach the largest Courant number bit for bit and
     the reference keeps the FIRST in loop order (src/swe/swe_petsc.c:289-296).  85 and 71 workgroups of cells: the XCD-swizzled
     launch, whose workgroup count -- and the ensembles' bucket count -- is padded to a multiple of 8; 10 workgroups: the plain one.
  C  a rank with ghosts: the stated difference of include/rdyhip.h (edges of owned cells with len / area_self only) pinned by
     helpers.owned_side_courant_numbers, and the property an adaptive dt needs: the maximum over the ranks is the whole mesh's.
  D  every branch of the arithmetic on jittered meshes with random diagonals, and the Roe entropy fix.

References: one C oracle per ensemble member; tests/tracer_reference.py for the tracers (its edge_courant is in loop order and
nanargmax keeps the first maximum).  Bars, the project's own: helpers.rel_linf <= 1e-10 for F, primitive variables and boundary
fluxes, 1e-12 relative to max(1, value) for the Courant number, ids exact.  Another edge than the reference's is accepted only
in parts A and D and only by the rule of test_gpu_parity.check_all(near_tie_ok=True): the reference's own number of the
device's edge is within 1e-13 of the maximum without being bit-equal to the number of the reference's edge, and the cell is the
one of the smaller area.

No test here asks for the rdyhip_kernel fixture (neither kernel depends on RDYHIP_KERNEL); conftest.py's autouse form of it still
runs each test under both values.  The meshes are built once (functools.lru_cache) and shared; the whole module takes about
four seconds on an MI355X."""
import functools

import numpy as np
import pytest

import tracer_reference as TR
from helpers import interior_courant_numbers, loop_edges, oracle_from_case, owned_side_courant_numbers, rel_linf
from random_cases import random_case, random_tri_mesh
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd import partition as P
from rdycore_amd.operator import (Operator, RDyFlowConfig, SOURCE_IMPLICIT_XQ2018, SOURCE_SEMI_IMPLICIT, TRACER_RIEMANN_ROE,
                                  TRACER_RIEMANN_UPWIND_ROE)
from test_gpu_ensemble import _check_euler_sample, _groups, boundary_courant_numbers
from test_gpu_numbering import _mixed_mesh
from test_tracers_cpu import tracer_case

pytestmark = pytest.mark.gpu

TOL = 1e-10
SOURCES = [SOURCE_SEMI_IMPLICIT, SOURCE_IMPLICIT_XQ2018]
RIEMANNS = [TRACER_RIEMANN_ROE, TRACER_RIEMANN_UPWIND_ROE]
G = 9.806


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(a):
    return _torch().tensor(np.ascontiguousarray(a), dtype=_torch().float64, device="cuda")


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(1.0, b)


# ---- ids ----------------------------------------------------------------------------------------------------------------------

def _check_ids(mesh, got, want, c_loop, near_tie_ok):
    """got, want: (global edge id, global cell id) of the device and of the reference; c_loop: the reference's Courant number per
    loop position (internal edges, then the boundaries' edges; NaN where skipped)"""
    if got == want:
        return
    assert near_tie_ok, (got, want)
    edges, cells = loop_edges(mesh)
    p, pw = (np.nonzero(mesh.edge_global_ids[edges] == g)[0] for g in (got[0], want[0]))
    assert p.size == 1 and pw.size == 1, (got, want)
    p, pw = int(p[0]), int(pw[0])
    cmax = float(np.nanmax(c_loop))
    assert c_loop[p] != c_loop[pw], f"the reference ties exactly on the two edges: {got} is not its first, {want}"
    assert abs(c_loop[p] - cmax) <= 1e-13 * cmax, (got, want, c_loop[p], cmax)
    assert got[1] == int(mesh.cell_global_ids[cells[p]]), (got, want)


def _global_ids(mesh, edge, cell):
    return int(mesh.edge_global_ids[edge]), int(mesh.cell_global_ids[cell])


# ---- ensembles ------------------------------------------------------------------------------------------------------------------

def _oracle_member(case):
    """(case, F, boundary fluxes, (Courant number, global edge, global cell)) from the C oracle, left unchanged"""
    orc = oracle_from_case(case)
    F = orc.apply(case.dt, case.u_local)
    assert np.isfinite(F).all()
    bf = [np.array(b) for b in orc.boundary_fluxes]
    diag = orc.diagnostics()
    orc.close()
    assert diag[0] > 0.0
    for a in [case.u_local, case.mannings, case.ext_src, F] + bf:
        a.setflags(write=False)
    return case, F, bf, diag


def _ensemble_operator(members):
    case0 = members[0][0]
    op = Operator.create(case0.config, case0.mesh, case0.condition_types)
    op.enable_ensemble(len(members))
    for m, (case, _, _, _) in enumerate(members):
        assert case.condition_types == case0.condition_types and case.mesh is case0.mesh
        op.ensemble_set_mannings_n(m, case.mannings)
        for comp in range(3):
            op.ensemble_set_external_source(m, comp, case.ext_src[:, comp])
        for b, vals in case.boundary_values.items():
            if len(vals):
                op.ensemble_set_boundary_values(m, b, vals)
    return op


def _ensemble_evaluate(members):
    """one launch for all members: (operator, device state, F [B, owned, 3], one CourantNumberDiagnostics per member)"""
    torch = _torch()
    mesh = members[0][0].mesh
    B = len(members)
    op = _ensemble_operator(members)
    u = _dev(np.stack([c.u_local for c, _, _, _ in members]))
    f = torch.full((B, mesh.num_owned_cells, 3), float("nan"), dtype=torch.float64, device="cuda")   # every owned row of every member is written
    op.ensemble_rhs_function([c.dt for c, _, _, _ in members], u, f)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    assert np.isfinite(got).all()
    op.ensemble_update_diagnostics()
    diags = op.ensemble_get_diagnostics()
    assert len(diags) == B
    return op, u, got, diags


def _check_member_diagnostics(tag, members, diags, near_tie_ok):
    for m, (case, _, _, (cmax, edge, cell)) in enumerate(members):
        d = diags[m]
        print(f"{tag} member {m}: Courant {d.max_courant_num!r} (oracle {cmax!r}, rel {abs(d.max_courant_num - cmax) / max(1.0, cmax):.2e}), "
              f"ids device {(d.global_edge_id, d.global_cell_id)} oracle {(edge, cell)}")
        assert _close(d.max_courant_num, cmax), (m, d.max_courant_num, cmax)
        c_loop = np.concatenate([interior_courant_numbers(case), boundary_courant_numbers(case)]) if near_tie_ok else None
        _check_ids(case.mesh, (d.global_edge_id, d.global_cell_id), (edge, cell), c_loop, near_tie_ok)


def _check_ensemble(tag, members, near_tie_ok, euler=False):
    """F, boundary fluxes, Courant value and ids of every member against its own oracle, on a mesh without ghosts"""
    mesh = members[0][0].mesh
    assert mesh.num_cells == mesh.num_owned_cells
    op, u, got, diags = _ensemble_evaluate(members)
    worst = 0.0
    for m, (case, F, bf, _) in enumerate(members):
        err = rel_linf(got[m], F)
        worst = max(worst, err)
        assert err <= TOL, (m, err)
        for b in range(len(mesh.boundaries)):
            have, want = op.ensemble_boundary_fluxes(m, b), bf[b]
            ok = np.isfinite(want).all(axis=1)          # an edge dry on both sides: 0 / 0 in the reference's flux, which it then discards
            assert rel_linf(have[ok], want[ok]) <= TOL, (m, b)
    print(f"{tag}: largest F error {worst:.3e}")
    _check_member_diagnostics(tag, members, diags, near_tie_ok)
    if euler:
        # the fused step leaves the same struct behind, and u_out = fma(dt_m, F, u) on a sample of rows
        _check_euler_sample(op, members, u, got)
        op.ensemble_update_diagnostics()
        after = op.ensemble_get_diagnostics()
        assert [(d.max_courant_num, d.global_edge_id, d.global_cell_id) for d in after] == \
               [(d.max_courant_num, d.global_edge_id, d.global_cell_id) for d in diags]
    op.destroy()
    return diags


def _random_members(mesh, src, seeds, tiny_h=1e-7, h_anuga=0.0):
    cfg = RDyFlowConfig(source_method=src, tiny_h=tiny_h, h_anuga_regular=h_anuga)
    return [_oracle_member(random_case(np.random.default_rng(s), mesh, cfg)) for s in seeds]


# ---- tracers --------------------------------------------------------------------------------------------------------------------

def _tracer_operator(case, ref, nt, riemann):
    op = CS.create_operator(case)
    op.enable_tracers(nt, riemann)
    for j in range(nt):
        op.tracers_set_source(j, ref.tracer_sources[:, j])
    for b in range(len(case.mesh.boundaries)):
        if case.mesh.boundaries[b].num_edges:
            op.tracers_set_boundary_values(b, ref.boundary_values[b])
    return op


def _tracer_evaluate(case, ref, u, nt, riemann):
    """(operator, F [owned, 3 + nt], primitive variables, CourantNumberDiagnostics) of one launch"""
    torch = _torch()
    mesh = case.mesh
    op = _tracer_operator(case, ref, nt, riemann)
    pv = op.tracers_primitive_variables()
    f = torch.full((mesh.num_owned_cells, 3 + nt), float("nan"), dtype=torch.float64, device="cuda")   # every owned row is written
    op.tracers_rhs_function(case.dt, _dev(u), f)
    torch.cuda.synchronize()
    got = f.cpu().numpy()
    assert np.isfinite(got).all()
    op.update_diagnostics()
    return op, got, pv.cpu().numpy(), op.get_diagnostics()


def _check_tracers(tag, case, ref, u, nt, riemann, near_tie_ok):
    """F, primitive variables, boundary fluxes, Courant value and ids against tracer_reference, on a mesh without ghosts"""
    mesh = case.mesh
    assert mesh.num_cells == mesh.num_owned_cells
    F = ref.apply(case.dt, u)
    assert np.isfinite(F).all() and np.abs(F[:, 3:]).max() > 0.0
    op, got, pv, d = _tracer_evaluate(case, ref, u, nt, riemann)
    err, perr = rel_linf(got, F), rel_linf(pv, ref.primitive_variables)
    assert err <= TOL and perr <= TOL, (err, perr)
    for b in range(len(mesh.boundaries)):
        have, want = op.tracers_boundary_fluxes(b), ref.boundary_fluxes[b]
        ok = np.isfinite(want).all(axis=1)
        assert rel_linf(have[ok], want[ok]) <= TOL, b
    cmax, edge, cell = ref.courant
    want_ids = _global_ids(mesh, edge, cell)
    print(f"{tag}: F {err:.3e}, pv {perr:.3e}, Courant {d.max_courant_num!r} (reference {cmax!r}, rel {abs(d.max_courant_num - cmax) / max(1.0, cmax):.2e}), "
          f"ids device {(d.global_edge_id, d.global_cell_id)} reference {want_ids}")
    assert cmax > 0.0 and _close(d.max_courant_num, cmax), (d.max_courant_num, cmax)
    _check_ids(mesh, (d.global_edge_id, d.global_cell_id), want_ids, ref.edge_courant, near_tie_ok)
    op.destroy()
    return d


# ---- A. the drop-in's numbering -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _numbered_mesh(name):
    if name == "tri":
        m = M.dmplex_like_numbering(M.structured_tri_mesh(61, 47, 1.0, zfunc=CS.mms_bathymetry(K=2 * np.pi / (0.8 * 61))), seed=5)
    elif name == "quad":
        m = M.dmplex_like_numbering(M.structured_quad_mesh(45, 37, 1.0, 1.5, zfunc=CS.mms_bathymetry(K=2 * np.pi / 30)), seed=9)
    elif name == "mixed":
        m = M.dmplex_like_numbering(_mixed_mesh(36, 28), seed=21)
        assert (m.cell_nverts == 3).any() and (m.cell_nverts == 4).any()
    else:
        m = M.structured_tri_mesh(53, 31, 1.0, zfunc=CS.mms_bathymetry(K=2 * np.pi / 40))
        if name == "edges_only":
            m = M.renumber_edges(m, np.random.default_rng(17).permutation(m.num_edges))
        else:
            assert name == "cells_only"
            m = M.renumber_cells(m, M.hilbert_cell_order(m.cell_centroids))
    if name == "edges_only":
        # (no flip in this half: the lower-numbered cell stays on the left, but the loop order owes nothing to the cells)
        first_seen = np.minimum(m.edge_cell_ids[0::2], np.where(m.edge_cell_ids[1::2] < 0, m.num_cells, m.edge_cell_ids[1::2]))
        assert (np.diff(first_seen[m.edge_internal_ids]) < 0).any()
    else:
        el, er = m.edge_cell_ids[0::2], m.edge_cell_ids[1::2]
        assert (el > er)[er >= 0].any()                                     # left is not the lower-numbered cell
    return m


NUMBERINGS = ["tri", "quad", "mixed", "edges_only", "cells_only"]


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("name", NUMBERINGS)
def test_ensemble_on_the_drop_ins_numbering(name, src):
    mesh = _numbered_mesh(name)
    base = 8000 + 100 * NUMBERINGS.index(name) + 10 * src
    _check_ensemble(f"A {name} src={src}", _random_members(mesh, src, range(base, base + 3)), near_tie_ok=True)


@pytest.mark.parametrize("riemann", RIEMANNS)
@pytest.mark.parametrize("nt", [2, 7])
@pytest.mark.parametrize("name", NUMBERINGS)
def test_tracers_on_the_drop_ins_numbering(name, nt, riemann):
    mesh = _numbered_mesh(name)
    rng = np.random.default_rng(8500 + 100 * NUMBERINGS.index(name) + 10 * nt + riemann)
    case, ref, u = tracer_case(rng, mesh, nt, riemann)
    assert {M.CONDITION_DIRICHLET, M.CONDITION_REFLECTING} == set(case.condition_types)
    _check_tracers(f"A {name} nt={nt} riemann={riemann}", case, ref, u, nt, riemann, near_tie_ok=True)


# ---- B. exact ties --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tie_mesh(shape):
    """(mesh, domain length in x) of test_gpu_numbering.test_courant_ids_on_exact_ties, and the 40 x 30 triangles of the plain launch"""
    if shape == "tri":
        return M.dmplex_like_numbering(M.structured_tri_mesh(120, 90, 1.0), seed=33), 120.0
    if shape == "quad":
        return M.dmplex_like_numbering(M.structured_quad_mesh(150, 120, 1.0, 1.0), seed=33), 150.0
    assert shape == "tri-small"
    return M.dmplex_like_numbering(M.structured_tri_mesh(40, 30, 1.0), seed=33), 40.0


WORKGROUPS = {"tri": 85, "quad": 71, "tri-small": 10}


def _uniform_case(shape, kind, dt, depth=10.0):
    """lake: h = depth everywhere, at rest; pools: h = 10 | 5, at rest.  Flat bed, reflecting walls, Manning 0.015."""
    mesh, lx = _tie_mesh(shape)
    assert (mesh.num_owned_cells + 255) // 256 == WORKGROUPS[shape]
    case = CS.dam_break_case(mesh, 1e9 if kind == "lake" else lx, dt=dt, perturb=0.0)
    if kind == "lake":
        case.u_local[:, 0] = depth
    else:
        assert set(np.unique(case.u_local[:, 0])) == {5.0, 10.0}
    return case


def _assert_a_real_tie(mesh, c_interior, cmax, edge, cell):
    """the conditions that keep a tie test from passing for the wrong reason: at least 100 internal edges reach the reference's
    maximum bit for bit, and the reference's cell is neither local cell 0 nor among the first workgroup's 256 owned cells.
    edge, cell: global ids.  Returns the number of tying internal edges."""
    ties = int((c_interior == cmax).sum())
    assert ties >= 100, ties
    lc = np.nonzero(mesh.cell_global_ids == cell)[0]
    assert lc.size == 1 and lc[0] != 0 and mesh.cell_local_to_owned[lc[0]] >= 256, (cell, lc)
    return ties


@pytest.mark.parametrize("shape,B", [("tri", 16), ("quad", 3), ("tri-small", 5)])
def test_ensemble_courant_ids_on_exact_ties(shape, B):
    """members cycle through a lake of 10 m, two flat pools and a lake of 7 m, each with a dt of its own; every member against
    its own oracle, no near-tie allowance; then the fused Euler step on the same inputs"""
    mesh, _ = _tie_mesh(shape)
    if shape == "tri":
        # 85 workgroups -> 88 on the swizzled launch: twelve groups would give 1056 workgroups, two members each make 8 groups
        assert _groups(B, mesh.num_owned_cells) == (8, 2)
    states = [("lake", 10.0), ("pools", 10.0), ("lake", 7.0)]
    members = []
    for m in range(B):
        kind, depth = states[m % 3]
        members.append(_oracle_member(_uniform_case(shape, kind, 1e-3 * (1.0 + 0.25 * m), depth)))
    for m, (case, _, _, (cmax, edge, cell)) in enumerate(members[:3]):
        ties = _assert_a_real_tie(mesh, interior_courant_numbers(case), cmax, edge, cell)
        print(f"B ensemble {shape} {states[m]}: {ties} internal edges tie at {cmax!r}; the oracle's edge {edge}, cell {cell}")
    assert members[0][3][1:] != members[1][3][1:]            # the winners of two members with different states differ
    _check_ensemble(f"B ensemble {shape} B={B}", members, near_tie_ok=False, euler=True)


CONC = {10.0: (0.3, 0.05), 5.0: (0.2, 0.1)}       # uniform concentrations, different per pool


@pytest.mark.parametrize("riemann", RIEMANNS)
@pytest.mark.parametrize("kind", ["lake", "pools"])
@pytest.mark.parametrize("shape", ["tri", "quad"])
def test_tracer_courant_ids_on_exact_ties(shape, kind, riemann):
    """the same states with two tracers of uniform concentration per pool (h c_i = const x h), Manning 0.015, a uniform tracer
    source: at rest the bed stress is zero, so erosion - deposition is -0.001 - 0.01 c_i, and F is finite"""
    case = _uniform_case(shape, kind, 1e-3)
    mesh = case.mesh
    ref = TR.TracerReference(mesh, case.condition_types, 2, riemann, case.config.tiny_h, case.config.h_anuga_regular)
    ref.mannings[:] = case.mannings
    ref.tracer_sources[:] = np.array([2e-3, 5e-4])
    h = case.u_local[:, 0]
    conc = np.array([CONC[float(x)] for x in h])
    u = np.concatenate([case.u_local, h[:, None] * conc], axis=1)
    ref.apply(case.dt, u)
    cmax, edge, cell = ref.courant
    ni = mesh.edge_internal_ids.size
    ties = _assert_a_real_tie(mesh, ref.edge_courant[:ni], cmax, *_global_ids(mesh, edge, cell))
    print(f"B tracers {shape} {kind} riemann={riemann}: {ties} internal edges tie at {cmax!r}")
    _check_tracers(f"B tracers {shape} {kind} riemann={riemann}", case, ref, u, 2, riemann, near_tie_ok=False)


def test_the_seed_the_ensemble_suite_steps_round():
    """seed 7705 on the 44 quads of planar_dam_10x5.msh (test_gpu_ensemble.TIED_SEEDS): a wet cell between two dry ones sees the
    same wave speed through two opposite edges.  One member; ids by the near-tie rule, which demands the oracle's edge where
    the two numbers are bit-equal."""
    from test_gpu_ensemble import TIED_SEEDS, _config, _get_mesh
    assert 7705 in TIED_SEEDS
    src = SOURCE_SEMI_IMPLICIT
    mesh = _get_mesh("quad-44")
    case = random_case(np.random.default_rng(7705), mesh, _config("quad-44", src))
    c = np.concatenate([interior_courant_numbers(case), boundary_courant_numbers(case)])
    top = np.sort(c[np.isfinite(c)])[-2:]
    assert top[1] - top[0] <= 1e-9 * top[1], "the seed no longer ties"
    print(f"B seed 7705: the two largest Courant numbers {top[1]!r}, {top[0]!r} (bit-equal: {top[0] == top[1]})")
    _check_ensemble("B seed 7705", [_oracle_member(case)], near_tie_ok=True)


# ---- C. a rank with ghosts ------------------------------------------------------------------------------------------------------

WORLD = 3
# lx, ly and the wave number of the bed and the state: no whole number of periods fits the domain, or the ranks' maxima would tie
PARTS = {"strips": (120.0, 48.0, 2 * np.pi / 97), "rcb_quads": (96.0, 48.0, 2 * np.pi / 71)}


@functools.lru_cache(maxsize=None)
def _part_meshes(kind, flat):
    """([the three ranks' local meshes, each through dmplex_like_numbering(seed=50 + rank)], the whole mesh) of
    test_gpu_numbering.test_courant_ids_per_rank_without_tilting; flat: no bathymetry (the ties of a uniform state are exact only
    where equal edges have bit-equal lengths and areas).  Both helpers number cells and edges independently of the cut (the
    edge id is made of the two global vertex ids), so the ranks' global cell AND edge ids are the whole mesh's."""
    z = None if flat else CS.mms_bathymetry(K=PARTS[kind][2])

    def build(rank, world):
        if kind == "strips":
            return M.strip_partition_tri_mesh(120 // world, 48, rank, world, 1.0, zfunc=z, order="tiled", tile=8)
        return P.partitioned_structured_mesh("quad", 192, 96, (0.5, 0.5), rank, world, zfunc=z, keep=CS.dam_break_keep(192, 96))
    ranks = []
    for rank in range(WORLD):
        m = M.dmplex_like_numbering(build(rank, WORLD), seed=50 + rank)
        assert m.num_cells > m.num_owned_cells
        el, er = m.edge_cell_ids[0::2], m.edge_cell_ids[1::2]
        assert ((er >= 0) & (m.cell_is_owned[el] == 0) & (m.cell_is_owned[np.maximum(er, 0)] == 0)).any()   # edges between two ghosts exist
        ranks.append(m)
    whole = build(0, 1)
    assert whole.num_cells == whole.num_owned_cells == sum(m.num_owned_cells for m in ranks)
    return ranks, whole


def _part_case(kind, state, mesh, variant):
    """the state as a function of the centroid, so that every rank and the whole mesh hold the same values.  variant 1: another
    member of the ensemble (other momenta or depth, Manning's n and dt)"""
    lx, ly, K = PARTS[kind]
    if state == "lake":
        case = CS.dam_break_case(mesh, 1e9, dt=1e-3 * (1 + 0.5 * variant), perturb=0.0)
        case.u_local[:, 0] = 10.0 - 3.0 * variant
        return case
    case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2 * (1 + 0.5 * variant), K=K)
    # friction_slope_case's fields are mirror-symmetric about the crests of sin(K x) sin(K y), and mirror-image edges tie to
    # rounding: a smooth tilt, again a function of the position alone, leaves one edge on top
    x, y = mesh.cell_centroids[:, 0], mesh.cell_centroids[:, 1]
    case.u_local = case.u_local * np.stack([1.0 + 0.10 * np.sin(0.037 * x + 0.023 * y + 0.3), 1.0 + 0.20 * np.cos(0.029 * x - 0.041 * y),
                                            1.0 + 0.15 * np.sin(0.031 * x + 0.047 * y + 1.1)], axis=1)
    if variant:
        case.u_local = case.u_local * np.array([1.0, -1.5, 0.5])
        case.mannings = case.mannings * 1.3
    return case


def _reduce(rows):
    """FindCourantNumberDiagnostics over the ranks in order: strictly larger replaces (timestep.reduce_courant)"""
    best = None
    for r in rows:
        if best is None or r.max_courant_num > best.max_courant_num:
            best = r
    return best


def _check_rank_struct(tag, mesh, d, restated, local_cmax):
    """checks 1 - 3 of a rank: the device's value is the restated owned-side maximum, it does not exceed what the rank-local
    reference (which also sees ghost-ghost edges and len / min(area)) reports, the cell is owned and the edge touches it"""
    c = restated[0]
    want = float(c.max())
    print(f"{tag}: Courant device {d.max_courant_num!r}, owned-side restatement {want!r} (rel {abs(d.max_courant_num - want) / max(1.0, want):.2e}), "
          f"rank-local reference {local_cmax!r}, ids device {(d.global_edge_id, d.global_cell_id)}")
    assert _close(d.max_courant_num, want), (d.max_courant_num, want)
    assert d.max_courant_num <= local_cmax * (1 + 1e-12), (d.max_courant_num, local_cmax)
    lc = np.nonzero(mesh.cell_global_ids == d.global_cell_id)[0]
    le = np.nonzero(mesh.edge_global_ids == d.global_edge_id)[0]
    assert lc.size == 1 and le.size == 1, (d, lc, le)
    assert mesh.cell_is_owned[lc[0]] != 0, f"{tag}: the reported cell {d.global_cell_id} is a ghost"
    assert lc[0] in mesh.edge_cell_ids[2 * le[0]: 2 * le[0] + 2], (d, mesh.edge_cell_ids[2 * le[0]: 2 * le[0] + 2])


def _check_against_the_whole_mesh(tag, state, got, cmax, ids, c_loop):
    """checks 4 and 5: the maximum over the ranks is the whole mesh's Courant number; where the whole mesh's maximum stands alone
    (asserted for the non-uniform state), the surviving struct carries the whole mesh's cell and edge ids"""
    best = _reduce(got)
    print(f"{tag}: over the ranks {best.max_courant_num!r} ids {(best.global_edge_id, best.global_cell_id)}; whole mesh {cmax!r} ids {ids}")
    assert _close(best.max_courant_num, cmax), (best.max_courant_num, cmax)
    if state != "lake":
        top = np.sort(c_loop[np.isfinite(c_loop)])[-2:]
        assert top[1] - top[0] > 1e-9 * top[1], "the whole mesh's state has a near tie"
        assert (best.global_edge_id, best.global_cell_id) == ids, (best, ids)


@pytest.mark.parametrize("state", ["friction_slope", "lake"])
@pytest.mark.parametrize("kind", ["strips", "rcb_quads"])
def test_ensemble_courant_on_ranks_with_ghosts(kind, state):
    ranks, whole = _part_meshes(kind, state == "lake")
    B = 2
    got = [[] for _ in range(B)]
    for rank, mesh in enumerate(ranks):
        members = [_oracle_member(_part_case(kind, state, mesh, v)) for v in range(B)]
        op, _, f, diags = _ensemble_evaluate(members)
        for v, (case, F, _, (local_cmax, _, _)) in enumerate(members):
            err = rel_linf(f[v], F)                                           # 6: F of the owned rows against the rank-local oracle
            assert err <= TOL, (rank, v, err)
            restated = owned_side_courant_numbers(mesh, interior_courant_numbers(case), boundary_courant_numbers(case))
            _check_rank_struct(f"C ensemble {kind} {state} rank {rank} member {v} (F {err:.3e})", mesh, diags[v], restated, local_cmax)
            got[v].append(diags[v])
        op.destroy()
    for v in range(B):
        case, _, _, (cmax, edge, cell) = _oracle_member(_part_case(kind, state, whole, v))
        c_loop = np.concatenate([interior_courant_numbers(case), boundary_courant_numbers(case)])
        _check_against_the_whole_mesh(f"C ensemble {kind} {state} member {v}", state, got[v], cmax, (edge, cell), c_loop)


def _part_tracer_case(kind, state, mesh, riemann):
    """_part_case with its critical-outflow boundary made reflecting and two tracers whose concentrations, sources and Dirichlet
    values are functions of the position"""
    case = _part_case(kind, state, mesh, 0)
    case.condition_types = [M.CONDITION_REFLECTING if t == M.CONDITION_CRITICAL_OUTFLOW else t for t in case.condition_types]
    ref = TR.TracerReference(mesh, case.condition_types, 2, riemann, case.config.tiny_h, case.config.h_anuga_regular)
    ref.mannings[:] = case.mannings
    ref.external_sources[:] = case.ext_src

    def conc(xy):
        if state == "lake":
            return np.tile([0.3, 0.05], (xy.shape[0], 1))
        return np.stack([0.3 + 0.2 * np.sin(0.11 * xy[:, 0]), 0.1 + 0.05 * np.cos(0.07 * xy[:, 1] + 0.02 * xy[:, 0])], axis=1)
    oc = mesh.owned_centroids()
    ref.tracer_sources[:] = 1e-3 * np.stack([np.sin(0.05 * oc[:, 0]), np.cos(0.04 * oc[:, 1])], axis=1)
    for b, vals in case.boundary_values.items():
        ref.boundary_values[b][:, :3] = vals
        ref.boundary_values[b][:, 3:] = vals[:, :1] * conc(mesh.edge_centroids[mesh.boundaries[b].edge_ids])
    u = np.concatenate([case.u_local, case.u_local[:, :1] * conc(mesh.cell_centroids)], axis=1)
    return case, ref, u


@pytest.mark.parametrize("riemann", RIEMANNS)
@pytest.mark.parametrize("state", ["friction_slope", "lake"])
@pytest.mark.parametrize("kind", ["strips", "rcb_quads"])
def test_tracer_courant_on_ranks_with_ghosts(kind, state, riemann):
    ranks, whole = _part_meshes(kind, state == "lake")
    got = []
    for rank, mesh in enumerate(ranks):
        case, ref, u = _part_tracer_case(kind, state, mesh, riemann)
        F = ref.apply(case.dt, u)
        op, f, pv, d = _tracer_evaluate(case, ref, u, 2, riemann)
        err, perr = rel_linf(f, F), rel_linf(pv, ref.primitive_variables)     # 6: against the rank-local reference
        assert np.isfinite(F).all() and err <= TOL and perr <= TOL, (rank, err, perr)
        ni = mesh.edge_internal_ids.size
        restated = owned_side_courant_numbers(mesh, ref.edge_courant[:ni], ref.edge_courant[ni:])
        _check_rank_struct(f"C tracers {kind} {state} riemann={riemann} rank {rank} (F {err:.3e})", mesh, d, restated, ref.courant[0])
        got.append(d)
        op.destroy()
    case, ref, u = _part_tracer_case(kind, state, whole, riemann)
    ref.apply(case.dt, u)
    cmax, edge, cell = ref.courant
    _check_against_the_whole_mesh(f"C tracers {kind} {state} riemann={riemann}", state, got, cmax, _global_ids(whole, edge, cell), ref.edge_courant)


# ---- D. the branches, on irregular meshes ----------------------------------------------------------------------------------------

def _fuzz_draw(seed):
    """the configuration and the mesh as test_gpu_fuzz.py draws them; the four seeds used here cover both values of tiny_h and
    h_anuga_regular = 1e-3"""
    rng = np.random.default_rng(2000 + seed)
    tiny_h, h_anuga = float(rng.choice([1e-7, 1e-5])), float(rng.choice([0.0, 0.0, 1e-3]))
    assert (tiny_h, h_anuga) == [(1e-7, 0.0), (1e-7, 0.0), (1e-5, 1e-3), (1e-5, 0.0)][seed]
    mesh = random_tri_mesh(rng, int(rng.integers(9, 30)), int(rng.integers(7, 22)))
    return rng, tiny_h, h_anuga, mesh


@pytest.mark.parametrize("seed", range(4))
def test_ensemble_on_random_meshes_and_states(seed):
    _, tiny_h, h_anuga, mesh = _fuzz_draw(seed)
    members = _random_members(mesh, int(seed % 2), range(9000 + 10 * seed, 9003 + 10 * seed), tiny_h, h_anuga)
    _check_ensemble(f"D ensemble seed {seed} tiny_h={tiny_h} h_anuga={h_anuga}", members, near_tie_ok=True)


@pytest.mark.parametrize("seed", range(4))
def test_tracers_on_random_meshes_and_states(seed):
    """h_anuga_regular enters the tracers' primitive variables only, not their Riemann states (include/rdyhip.h), and
    tracer_reference says the same"""
    rng, tiny_h, h_anuga, mesh = _fuzz_draw(seed)
    riemann = RIEMANNS[seed % 2]
    case, ref, u = tracer_case(rng, mesh, 2, riemann, h_anuga=h_anuga, tiny_h=tiny_h)
    assert (case.config.tiny_h, case.config.h_anuga_regular) == (tiny_h, h_anuga) == (ref.tiny_h, ref.h_anuga)
    _check_tracers(f"D tracers seed {seed} tiny_h={tiny_h} h_anuga={h_anuga} riemann={riemann}", case, ref, u, 2, riemann, near_tie_ok=True)


def _entropy_fix_edges(mesh, u):
    """per internal edge: does the inequality of test_gpu_fuzz.test_entropy_fix_branch_is_exercised hold, |lambda| < d(lambda)
    for the first or the third wave (src/swe/swe_roe_flux_petsc.h:56-67)?"""
    e = mesh.edge_internal_ids
    l, r = mesh.edge_cell_ids[2 * e], mesh.edge_cell_ids[2 * e + 1]
    cn, sn = mesh.edge_cn[e], mesh.edge_sn[e]
    hl, hr = u[l, 0], u[r, 0]
    upl = (u[l, 1] * cn + u[l, 2] * sn) / hl
    upr = (u[r, 1] * cn + u[r, 2] * sn) / hr
    cl, cr, chat = np.sqrt(G * hl), np.sqrt(G * hr), np.sqrt(0.5 * G * (hl + hr))
    uhat = (np.sqrt(hl) * upl + np.sqrt(hr) * upr) / (np.sqrt(hl) + np.sqrt(hr))
    return (np.abs(uhat - chat) < np.maximum(0.0, 2 * ((upr - cr) - (upl - cl)))) | (np.abs(uhat + chat) < np.maximum(0.0, 2 * ((upr + cr) - (upl + cl))))


@functools.lru_cache(maxsize=None)
def _transcritical():
    """the stepped state of test_gpu_fuzz.test_transcritical_edges: depth falls and velocity rises along x in steps, so every
    x-facing edge between two steps is a strong rarefaction.  Returns (mesh, state, step index of every cell)."""
    rng = np.random.default_rng(9)
    mesh = random_tri_mesh(rng, 24, 16)
    step = np.floor(mesh.cell_centroids[:, 0] / 1.5)
    h = 2.0 * 0.75 ** step
    u = np.stack([h, h * (0.5 + 1.6 * step), h * 0.1 * rng.normal(size=h.size)], axis=1)
    assert _entropy_fix_edges(mesh, u).sum() >= 20
    u.setflags(write=False)
    return mesh, u, step


def _transcritical_case(variant=0):
    mesh, u, _ = _transcritical()
    u = u * np.array([1.0, 1.0 + 0.05 * variant, 1.0 - 0.5 * variant])
    assert _entropy_fix_edges(mesh, u).sum() >= 20
    return CS.Case("transcritical", mesh, RDyFlowConfig(), [M.CONDITION_REFLECTING] * len(mesh.boundaries), u,
                   np.full(mesh.num_cells, 0.02 + 0.01 * variant), np.zeros((mesh.num_cells, 3)), {}, 1e-3 * (1 + variant))


def test_ensemble_on_transcritical_edges():
    _check_ensemble("D ensemble transcritical", [_oracle_member(_transcritical_case(v)) for v in range(3)], near_tie_ok=True)


@pytest.mark.parametrize("riemann", RIEMANNS)
def test_tracers_on_transcritical_edges(riemann):
    """the concentrations step where depth and velocity do"""
    case = _transcritical_case()
    mesh, _, step = _transcritical()
    ref = TR.TracerReference(mesh, case.condition_types, 2, riemann, case.config.tiny_h, case.config.h_anuga_regular)
    ref.mannings[:] = case.mannings
    ref.tracer_sources[:] = np.array([1e-3, -5e-4])
    conc = np.stack([0.6 * 0.8 ** step, 0.05 + 0.03 * step], axis=1)
    u = np.concatenate([case.u_local, case.u_local[:, :1] * conc], axis=1)
    _check_tracers(f"D tracers transcritical riemann={riemann}", case, ref, u, 2, riemann, near_tie_ok=True)
