"""CPU: the numpy restatements of the Courant diagnostic that the GPU tests of the tracer and ensemble kernels lean on
(helpers.loop_edges, helpers.owned_side_courant_numbers) against the C oracle and against each other."""
import numpy as np

from helpers import interior_courant_numbers, loop_edges, oracle_from_case, owned_side_courant_numbers
from random_cases import random_case, random_mesh, random_partition_mesh
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig
from test_gpu_ensemble import boundary_courant_numbers


def _numbers(case):
    return interior_courant_numbers(case), boundary_courant_numbers(case)


def test_loop_positions_name_the_oracles_edge_and_cell():
    """the oracle's (value, edge, cell) is the first maximum of the restated numbers, read through loop_edges -- on meshes as
    build_mesh numbers them and on the drop-in's numbering (flipped edges: the cell is the smaller one, not the left one)"""
    for seed, kind in enumerate(("tri", "quad", "mixed")):
        rng = np.random.default_rng(300 + seed)
        mesh = random_mesh(rng, kind, 11, 8)
        for m in (mesh, M.dmplex_like_numbering(mesh, seed=seed)):
            case = random_case(rng, m, RDyFlowConfig())
            orc = oracle_from_case(case)
            orc.apply(case.dt, case.u_local)
            cmax, edge, cell = orc.diagnostics()
            c = np.concatenate(_numbers(case))
            top = np.sort(c[np.isfinite(c)])[-2:]
            assert top[1] - top[0] > 1e-9 * top[1]
            p = int(np.nanargmax(c))
            edges, cells = loop_edges(m)
            assert abs(c[p] - cmax) <= 1e-12 * max(1.0, cmax)
            assert (int(m.edge_global_ids[edges[p]]), int(m.cell_global_ids[cells[p]])) == (edge, cell)


def test_owned_side_numbers_are_the_references_on_a_mesh_without_ghosts():
    """every internal edge gives two rows, every boundary edge one; the larger of an edge's two rows IS the reference's number,
    bit for bit, and it stands in the row of the cell loop_edges names (or both rows hold it: equal areas)"""
    rng = np.random.default_rng(41)
    for kind in ("tri", "mixed"):
        mesh = M.dmplex_like_numbering(random_mesh(rng, kind, 13, 9), seed=3)
        case = random_case(rng, mesh, RDyFlowConfig(h_anuga_regular=1e-3))
        ci, cb = _numbers(case)
        c, pos, edge, cell = owned_side_courant_numbers(mesh, ci, cb)
        ni = mesh.edge_internal_ids.size
        assert np.isfinite(ci).sum() > 50 and np.isnan(ci).any()                  # some edges dry on both sides: they give no row
        assert c.size == 2 * np.isfinite(ci).sum() + np.isfinite(cb).sum()
        per_pos = np.full(ni + cb.size, -np.inf)
        np.maximum.at(per_pos, pos, c)
        want = np.concatenate([ci, cb])
        ok = np.isfinite(want)
        assert np.array_equal(per_pos[ok], want[ok]) and np.isinf(per_pos[~ok]).all()
        edges, cells = loop_edges(mesh)
        assert np.array_equal(edge, edges[pos])
        at_max = c == per_pos[pos]
        named = cell == cells[pos]
        assert at_max[named].all()                                                # the smaller cell's row holds the reference's number
        assert (c.max() == np.nanmax(want)) and (c <= per_pos[pos]).all()


def test_owned_side_numbers_on_a_rank_with_ghosts():
    """rows belong to owned cells only; an edge between two ghosts gives none; a cut edge gives one, scaled down by
    min(area) / area_owned where the ghost is the smaller cell; boundary edges behind ghosts give none"""
    rng = np.random.default_rng(415)
    mesh = M.dmplex_like_numbering(random_partition_mesh(rng, "tri", 14, 15), seed=8)
    case = random_case(rng, mesh, RDyFlowConfig())
    case.u_local[:, 0] = np.maximum(case.u_local[:, 0], 0.05)                     # wet everywhere: every edge counts
    ci, cb = _numbers(case)
    assert np.isfinite(ci).all()
    c, pos, edge, cell = owned_side_courant_numbers(mesh, ci, cb)
    owned = mesh.cell_is_owned != 0
    assert owned[cell].all()
    e = mesh.edge_internal_ids
    l, r = mesh.edge_cell_ids[2 * e], mesh.edge_cell_ids[2 * e + 1]
    n_rows = owned[l].astype(int) + owned[r].astype(int)
    assert (n_rows == 0).any() and (n_rows == 1).any() and (n_rows == 2).any()
    assert np.array_equal(np.bincount(pos[pos < e.size], minlength=e.size), n_rows)
    area = mesh.cell_areas
    cut = np.nonzero(n_rows == 1)[0]
    mine = np.where(owned[l[cut]], l[cut], r[cut])
    ghost = np.where(owned[l[cut]], r[cut], l[cut])
    row_of = {int(p): k for k, p in enumerate(pos) if p < e.size and n_rows[p] == 1}
    got = np.array([c[row_of[int(p)]] for p in cut])
    smaller_ghost = area[ghost] < area[mine]
    assert smaller_ghost.any() and (~smaller_ghost).any()
    assert np.array_equal(got[~smaller_ghost], ci[cut][~smaller_ghost])
    assert (got[smaller_ghost] < ci[cut][smaller_ghost]).all()
    assert np.allclose(got, ci[cut] * np.minimum(area[ghost], area[mine]) / area[mine], rtol=1e-14, atol=0.0)
    be = np.concatenate([b.edge_ids for b in mesh.boundaries])
    nb_rows = int((pos >= e.size).sum())
    assert nb_rows == int((owned[mesh.edge_cell_ids[2 * be]] & np.isfinite(cb)).sum()) and nb_rows > 0
