"""Meshes, states and exchange patterns of the tracer tests on several ranks (a plain module: test_tracers_multirank_cpu.py
checks the seeds without a device, test_gpu_tracers_multirank.py runs them).  Everything is numpy; every case is computed once,
shared and left unchanged.

  * `rcb(nt, riemann)`: a jittered 24 x 24 triangle mesh (1 152 cells, distinct areas), a random tracer case on it with its
    reference results, and its three RCB parts (partition.partition_mesh: owned cells first, ghosts grouped by owner), each
    with the inputs of the undivided case restricted to it and the exchange pattern the three ranks would agree on.
  * `single(name, nt, riemann)`: one rank's mesh on its own -- "part-o2l" (ghosts interleaved), "band" (one row of squares:
    every owned cell has a ghost neighbour), "tri-30" (no ghost at all) -- with a pattern of two made-up peers.
  * `owned_side_courant`: the Courant numbers as the tracer kernel sees them on a rank with ghosts (include/rdyhip.h: the
    edges of the owned cells with len / area_self), per owned cell and per edge.
"""
import dataclasses
import functools
from typing import List

import numpy as np

import random_cases as RC
import tracer_reference as TR
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd import partition as P
from test_tracers_cpu import tracer_case

NX = NY = 24
NPARTS = 3


@dataclasses.dataclass
class Part:
    mesh: object
    case: object                  # CS.Case of the part (what CS.create_operator takes)
    ref: object                   # TR.TracerReference of the part with the inputs set (not applied)
    u: np.ndarray                 # [num_cells, 3 + nt] the complete local state: the owners' rows in the ghost rows
    peers: List[int]
    send_counts: np.ndarray
    send_ids: np.ndarray          # local ids of owned cells, peer by peer
    recv_counts: np.ndarray
    recv_ids: np.ndarray          # local ids of ghost cells, peer by peer
    bpos: list = None             # parts of an undivided case: per boundary, the undivided boundary's edge of every local edge


def edge_keys(mesh, vertex_global_ids=None, num_vertices_global=None):
    """a partition-independent id of every edge: its two global vertex ids"""
    g = np.arange(mesh.num_vertices, dtype=np.int64) if vertex_global_ids is None else np.asarray(vertex_global_ids, dtype=np.int64)
    nvg = mesh.num_vertices if num_vertices_global is None else num_vertices_global
    a, b = g[mesh.edge_vertex_ids[:, 0]], g[mesh.edge_vertex_ids[:, 1]]
    return np.minimum(a, b) * nvg + np.maximum(a, b)


def ghost_adjacent(mesh):
    """[num_owned] bool: the owned cell has a ghost neighbour (RDYHIP_PHASE_HALO), by edges"""
    owned, l2o = mesh.cell_is_owned != 0, mesh.cell_local_to_owned
    e = mesh.edge_internal_ids
    l, r = mesh.edge_cell_ids[2 * e], mesh.edge_cell_ids[2 * e + 1]
    out = np.zeros(mesh.num_owned_cells, dtype=bool)
    out[l2o[l[owned[l] & ~owned[r]]]] = True
    out[l2o[r[owned[r] & ~owned[l]]]] = True
    return out


def owned_side_courant(mesh, ref, u, dt):
    """(per owned cell, per edge in the reference's loop order -- NaN where no owned cell evaluates it): amax len / area_self dt
    over the edges of the owned cells, both sides dry skipped"""
    tiny, owned, l2o, area = ref.tiny_h, mesh.cell_is_owned != 0, mesh.cell_local_to_owned, mesh.cell_areas
    cell = np.zeros(mesh.num_owned_cells)
    e = mesh.edge_internal_ids
    l, r = mesh.edge_cell_ids[2 * e], mesh.edge_cell_ids[2 * e + 1]
    _, amax = TR.edge_flux(TR.riemann_states(u[l], tiny), TR.riemann_states(u[r], tiny), mesh.edge_sn[e], mesh.edge_cn[e], ref.riemann)
    use = ~((u[r, 0] < tiny) & (u[l, 0] < tiny))
    edge = np.full(e.size, np.nan)
    for side in (l, r):
        sel = use & owned[side]
        val = amax[sel] * mesh.edge_lengths[e][sel] / area[side[sel]] * dt
        np.maximum.at(cell, l2o[side[sel]], val)
        edge[sel] = np.fmax(edge[sel], val)
    edges = [edge]
    for b, bnd in enumerate(mesh.boundaries):
        e = bnd.edge_ids
        l = mesh.edge_cell_ids[2 * e]
        sn, cn = mesh.edge_sn[e], mesh.edge_cn[e]
        L = TR.riemann_states(u[l], tiny)
        if ref.types[b] == M.CONDITION_DIRICHLET:
            R = TR.riemann_states(ref.boundary_values[b], tiny)
        else:
            d1, d2 = sn * sn - cn * cn, 2.0 * sn * cn
            R = (L[0], L[1] * d1 - L[2] * d2, -L[1] * d2 - L[2] * d1, L[3])
        _, amax = TR.edge_flux(L, R, sn, cn, ref.riemann)
        use = owned[l] & ~((L[0] < tiny) & (R[0] < tiny))
        val = np.where(use, amax * mesh.edge_lengths[e] / area[l] * dt, np.nan)
        np.maximum.at(cell, l2o[l[use]], val[use])
        edges.append(val)
    return cell, np.concatenate(edges)


def top_gap(values):
    """relative gap between the largest and the second largest finite value"""
    v = np.sort(values[np.isfinite(values)])
    return (v[-1] - v[-2]) / v[-1]


def _restrict(g_mesh, g_case, g_ref, g_u, mesh, vertex_gids):
    """the undivided case's inputs on a local mesh cut from it"""
    gid = np.asarray(mesh.cell_global_ids)
    own = gid[mesh.cell_owned_to_local]
    nt = g_ref.nt
    ref = TR.TracerReference(mesh, g_ref.types, nt, g_ref.riemann, g_ref.tiny_h, g_ref.h_anuga)
    ref.mannings[:] = g_ref.mannings[own]
    ref.external_sources[:] = g_ref.external_sources[own]
    ref.tracer_sources[:] = g_ref.tracer_sources[own]
    gkey = edge_keys(g_mesh)
    lkey = edge_keys(mesh, vertex_gids, g_mesh.num_vertices)
    bvals, bpos = {}, []
    assert len(mesh.boundaries) == len(g_mesh.boundaries)
    for b, bnd in enumerate(mesh.boundaries):
        ge = g_mesh.boundaries[b].edge_ids
        order = np.argsort(gkey[ge])
        pos = order[np.searchsorted(gkey[ge][order], lkey[bnd.edge_ids])]
        assert (gkey[ge][pos] == lkey[bnd.edge_ids]).all()
        bpos.append(pos)
        ref.boundary_values[b][:] = g_ref.boundary_values[b][pos]
        if b in g_case.boundary_values:
            bvals[b] = g_case.boundary_values[b][pos]
    case = CS.Case("part", mesh, g_case.config, list(g_case.condition_types), np.ascontiguousarray(g_u[gid, :3]), ref.mannings.copy(),
                   ref.external_sources.copy(), bvals, g_case.dt)
    return case, ref, np.ascontiguousarray(g_u[gid]), bpos


def split(g_mesh, g_case, g_ref, g_u, nparts=NPARTS, boundary_classifier=None):
    """the parts of an undivided case (RCB of the cell centroids) with the exchange pattern between them"""
    xyz, conn = g_mesh.xyz, g_mesh.cell_conn
    meshes = [P.partition_mesh(xyz, conn, nparts, r, boundary_classifier=boundary_classifier) for r in range(nparts)]
    parts = []
    for r, mesh in enumerate(meshes):
        used = np.unique(conn[mesh._cell_sel][conn[mesh._cell_sel] >= 0])      # extract_local_mesh's vertex numbering
        case, ref, u, bpos = _restrict(g_mesh, g_case, g_ref, g_u, mesh, used)
        owner, gid = mesh.cell_owner_rank, np.asarray(mesh.cell_global_ids)
        ghost = np.nonzero(mesh.cell_is_owned == 0)[0]
        local_of = {int(g): i for i, g in enumerate(gid)}
        needs = {}                                                             # q -> the cells of r that q has as ghosts, in q's order
        for q, mq in enumerate(meshes):
            if q != r:
                gq = np.nonzero((mq.cell_is_owned == 0) & (mq.cell_owner_rank == r))[0]
                if gq.size:
                    needs[q] = np.array([local_of[int(g)] for g in np.asarray(mq.cell_global_ids)[gq]], dtype=np.int32)
        peers = sorted(set(int(q) for q in owner[ghost]) | set(needs))
        recv = [ghost[owner[ghost] == q].astype(np.int32) for q in peers]
        send = [needs.get(q, np.zeros(0, dtype=np.int32)) for q in peers]
        parts.append(Part(mesh, case, ref, u, peers, np.array([s.size for s in send], dtype=np.int32), np.concatenate(send).astype(np.int32),
                          np.array([x.size for x in recv], dtype=np.int32), np.concatenate(recv).astype(np.int32), bpos))
    return parts


@functools.lru_cache(maxsize=None)
def rcb(nt, riemann):
    """(undivided mesh, case, reference with the results of ONE apply, state, F, parts)"""
    rng = np.random.default_rng(7300 + 10 * nt + riemann)
    xyz, conn = RC.random_connectivity(rng, "tri", NX, NY)
    classifier = M.box_side_boundaries(0, NX, 0, NY)
    g_mesh = M.build_mesh(xyz, conn, boundary_classifier=classifier)
    case, ref, u = tracer_case(rng, g_mesh, nt, riemann)
    F = ref.apply(case.dt, u)
    parts = split(g_mesh, case, ref, u, NPARTS, classifier)
    for a in (u, F, ref.primitive_variables):
        a.setflags(write=False)
    return g_mesh, case, ref, u, F, parts


def band_mesh():
    """one row of squares between two rows of ghosts: every owned triangle has its vertical neighbour on another rank"""
    xyz, conn, _, _ = M.structured_tri_connectivity(40, 3)
    cy = xyz[conn, 1].mean(axis=1)
    return M.extract_local_mesh(xyz, conn, (cy > 1.0) & (cy < 2.0), boundary_classifier=M.box_side_boundaries(0, 40, 0, 3))


@functools.lru_cache(maxsize=None)
def single(name, nt, riemann):
    """a Part for one rank's mesh on its own: the ghost rows are received from two made-up peers (first and second half of the
    ghosts), the ghost-adjacent owned cells are sent to them"""
    from test_gpu_tracers import _mesh
    mesh = band_mesh() if name == "band" else _mesh(name)
    rng = np.random.default_rng(2100 + 10 * nt + riemann + len(name))
    case, ref, u = tracer_case(rng, mesh, nt, riemann)
    ghost = np.nonzero(mesh.cell_is_owned == 0)[0].astype(np.int32)
    send = np.asarray(mesh.cell_owned_to_local)[ghost_adjacent(mesh)].astype(np.int32)
    if ghost.size == 0:
        z = np.zeros(0, dtype=np.int32)
        return Part(mesh, case, ref, u, [], z, z, z, z)
    cut = lambda a: np.array([a.size // 2, a.size - a.size // 2], dtype=np.int32)
    u.setflags(write=False)
    return Part(mesh, case, ref, u, [1, 2], cut(send), send, cut(ghost), ghost)


def courant_states(part):
    """two states of a part for the merge of the Courant record: the momentum of one cell raised so that the largest number is
    at an INTERIOR cell all of whose neighbours are INTERIOR cells too (a), at a HALO cell (b); returns ((state, cell) x 2)"""
    mesh, u = part.mesh, part.u
    halo = ghost_adjacent(mesh)
    o2l, l2o, owned = np.asarray(mesh.cell_owned_to_local), mesh.cell_local_to_owned, mesh.cell_is_owned != 0
    e = mesh.edge_internal_ids
    l, r = mesh.edge_cell_ids[2 * e], mesh.edge_cell_ids[2 * e + 1]
    near_halo = halo.copy()                      # a HALO cell or the neighbour of one
    smallest = np.ones(mesh.num_owned_cells, dtype=bool)   # smaller than every owned neighbour: its own len / area is the edge's largest
    for a, b in ((l, r), (r, l)):
        sel = owned[a] & owned[b]
        np.logical_or.at(near_halo, l2o[a[sel]], halo[l2o[b[sel]]])
        np.logical_and.at(smallest, l2o[a[sel]], mesh.cell_areas[a[sel]] < mesh.cell_areas[b[sel]])
    deep = u[o2l, 0] > 0.5
    out = []
    for pick in (np.nonzero(~near_halo & deep)[0], np.nonzero(halo & deep & smallest)[0]):
        o = int(pick[len(pick) // 2])
        s = np.array(u)
        s[o2l[o], 1:3] = s[o2l[o], 0] * np.array([70.0, 45.0])
        s.setflags(write=False)
        out.append((s, o))
    return out
