"""CPU: the tracer path on several ranks (rdyhip_tracer_phase_*, rdyhip_halo_tracers_*) as far as it goes without a device --
the new entry points report a null operator before any device call, the ctypes table matches the header, and the
PRECONDITIONS of every case of tests/test_gpu_tracers_multirank.py hold for the seeds it uses, computed with
tests/tracer_reference.py alone: F is finite, the largest edge Courant number stands clear of the runner-up, and every mesh has
the mix of INTERIOR and HALO cells its case is about.  A seed that fails here is replaced; no GPU case skips an assertion."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tracer_parts as TP
import tracer_reference as TR
from rdycore_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rdyhip_tracer_phase_rhs", "rdyhip_tracer_phase_euler_step", "rdyhip_halo_tracers_rhs", "rdyhip_halo_tracers_euler_step"]
# (NT, tracer Riemann solver) of the GPU cases
COMBOS = [(1, TR.RIEMANN_ROE), (2, TR.RIEMANN_UPWIND_ROE), (7, TR.RIEMANN_ROE)]
GAP = 1e-9


def test_every_new_entry_point_reports_a_null_operator():
    lib = _lib.load()
    calls = {
        "rdyhip_tracer_phase_rhs": (None, 0, 2, 0.1, None, None, None),
        "rdyhip_tracer_phase_euler_step": (None, 0, 2, 0.1, None, None, None, None),
        "rdyhip_halo_tracers_rhs": (None, None, 0.1, None, None, None),
        "rdyhip_halo_tracers_euler_step": (None, None, 0.1, None, None, None, None),
    }
    assert sorted(calls) == sorted(NEW)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())
    assert lib.rdyhip_version() == 110 == _lib.ABI_VERSION


def test_argtypes_match_the_header():
    """every parameter of the four declarations, by its C type: a pointer is passed as void*, int32_t and double as themselves"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdyhip.h")).read(), flags=re.S)
    kinds = {"int32_t": C.c_int32, "double": C.c_double}
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        want = []
        for p in m.group(1).split(","):
            p = p.strip()
            want.append(C.c_void_p if ("*" in p or p.startswith(("RDyHipOperator", "RDyHipHalo"))) else kinds[p.split()[0]])
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and list(args) == want, name
    for k, v in (("RDYHIP_HALO_STEP_TRACERS_RHS", 2), ("RDYHIP_HALO_STEP_TRACERS_EULER", 3)):
        assert re.search(r"#define\s+" + k + r"\s+" + str(v) + r"\b", src)
    from rdycore_amd.halo import HaloExchange
    assert HaloExchange.STEP_KINDS == {"rhs": 0, "euler": 1, "tracers_rhs": 2, "tracers_euler": 3}


@pytest.mark.parametrize("nt,riemann", COMBOS)
def test_rcb_parts_have_both_kinds_of_cell_and_a_clear_maximum(nt, riemann):
    g_mesh, case, ref, u, F, parts = TP.rcb(nt, riemann)
    assert g_mesh.num_cells == 2 * TP.NX * TP.NY and np.isfinite(F).all() and np.abs(F[:, 3:]).max() > 0.0
    assert (u[:, 0] == 0.0).any() and ((u[:, 0] > 0.0) & (u[:, 0] < case.config.tiny_h)).any()
    cmax, edge, cell = ref.courant
    assert cmax > 0.0 and TP.top_gap(ref.edge_courant) > GAP
    # the two cells of the maximal edge differ in area: the cell id of the maximum is then the owned-side rule's too
    l, r = g_mesh.edge_cell_ids[2 * edge], g_mesh.edge_cell_ids[2 * edge + 1]
    assert r < 0 or g_mesh.cell_areas[l] != g_mesh.cell_areas[r]
    assert len(np.unique(g_mesh.cell_areas)) == g_mesh.num_cells
    owned = np.zeros(g_mesh.num_cells, dtype=int)
    best = []
    for p in parts:
        m = p.mesh
        halo = TP.ghost_adjacent(m)
        assert halo.any() and (~halo).any() and m.num_owned_cells > 256            # both kinds of cell, more than one workgroup
        assert (np.asarray(m.cell_owned_to_local) == np.arange(m.num_owned_cells)).all()   # owned cells first
        assert (np.diff(p.recv_ids) == 1).all() and p.recv_ids[0] == m.num_owned_cells     # ghosts grouped by owner: direct receive
        assert p.recv_ids.size == m.num_cells - m.num_owned_cells and (m.cell_is_owned[p.send_ids] != 0).all()
        assert len(p.peers) == 2 and (p.send_counts > 0).all() and (p.recv_counts > 0).all()
        owned[np.asarray(m.cell_global_ids)[m.cell_owned_to_local]] += 1
        c, e = TP.owned_side_courant(m, p.ref, p.u, case.dt)
        assert TP.top_gap(e) > GAP
        best.append(c.max())
    assert (owned == 1).all()                                                       # every cell has exactly one owner
    # the maximum over the ranks is the whole mesh's: the smaller cell of every edge is owned by someone
    assert abs(max(best) - cmax) <= 1e-12 * max(1.0, cmax)
    assert sorted(best)[-1] - sorted(best)[-2] > GAP * max(best)                    # reduce_courant has no tie to break


@pytest.mark.parametrize("nt,riemann", COMBOS)
@pytest.mark.parametrize("name", ["part-o2l", "band", "tri-30"])
def test_single_meshes_have_the_cells_their_case_needs(name, nt, riemann):
    p = TP.single(name, nt, riemann)
    m = p.mesh
    halo = TP.ghost_adjacent(m)
    if name == "part-o2l":
        assert halo.any() and (~halo).any()
        assert (np.asarray(m.cell_owned_to_local) != np.arange(m.num_owned_cells)).any()   # the owned -> local table is used
        assert not (np.diff(p.recv_ids) == 1).all()                                         # ghosts interleaved: the unpack path
        blocks = [halo[i:i + 256] for i in range(0, m.num_owned_cells, 256)]
        assert len(blocks) == 4 and all(b.any() and (~b).any() for b in blocks)             # every workgroup holds both kinds
    elif name == "band":
        assert halo.all() and m.num_owned_cells == 80                                       # INTERIOR is empty
    else:
        assert not halo.any() and m.num_cells == m.num_owned_cells == 30 and not p.peers    # HALO is empty
    F = p.ref.apply(p.case.dt, p.u)
    assert np.isfinite(F).all() and np.abs(F[:, 3:]).max() > 0.0
    c, e = TP.owned_side_courant(m, p.ref, p.u, p.case.dt)
    assert c.max() > 0.0 and TP.top_gap(e) > GAP


def test_courant_states_put_the_maximum_in_either_phase():
    p = TP.single("part-o2l", 2, TR.RIEMANN_UPWIND_ROE)
    halo = TP.ghost_adjacent(p.mesh)
    (sa, oa), (sb, ob) = TP.courant_states(p)
    assert not halo[oa] and halo[ob]
    for s, in_halo in ((sa, False), (sb, True)):
        assert np.isfinite(p.ref.apply(p.case.dt, s)).all()
        c, e = TP.owned_side_courant(p.mesh, p.ref, s, p.case.dt)
        assert TP.top_gap(e) > GAP
        hi, lo = (c[halo].max(), c[~halo].max()) if in_halo else (c[~halo].max(), c[halo].max())
        assert lo > 0.0 and hi > lo * (1.0 + GAP)
        assert TP.top_gap(np.where(halo, c, np.nan)) > GAP                                  # the HALO cells' own maximum is clear too


def test_sediment_parts_of_the_mms_mesh():
    """case 6: one RCB part of the sediment MMS mesh at the base refinement level has both kinds of cell and two peers"""
    import mms
    from rdycore_amd import partition as P
    g = mms.level_mesh(1)
    m = P.partition_mesh(g.xyz, g.cell_conn, 3, 1, boundary_classifier=P.owned_cell_boundaries())
    halo = TP.ghost_adjacent(m)
    assert halo.any() and (~halo).any() and len(m.boundaries) == 1 and m.boundaries[0].num_edges > 0
    assert len(set(m.cell_owner_rank[m.cell_is_owned == 0])) == 2
